#!/usr/bin/env python3
"""Golden vectors for the GPTQ solve with an activation order and static groups, produced by the REAL reference (amq/quantization/gptq.py:
GPTQ_METHOD.add_batch / fasterquant(actorder=True, static_groups=True) with its Quantizer, asymmetric, percdamp 0.01) on the CPU -- data only; no
reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_gptq_actorder.py

One file per shape and group size, ``gptqact_{N}x{K}_g{G}.npz`` (and ``gptqact_edge.npz``), each under 500 KB and holding
  W         fp16 [N, K]   the dense weights (a dead column still holds its values: the caller zeroes it, as gptq.py:226-228 does)
  X         fp16 [T, K]   the calibration rows (gen_golden_gptq.calibration without its grid, the column energies respaced: below)
  perm      int64 [K]     the reference's order: argsort(diag(H), descending) with a dead column's diagonal set to 1
  U_p       fp32 [K, K]   the upper Cholesky factor of the damped inverse of H[perm][:, perm], from the reference's own three linalg calls
  dead      bool [K]      columns whose Hessian diagonal is 0 (W's own order)
  bits      int32 [3]     2, 3, 4
  group     int32
  Q_b{bits}      fp32 [N, K]  the reference's fake-quantized weights under actorder=True, static_groups=True (W's own column order)
  loss_b{bits}   fp64         its printed `error`
  Qplain_b{bits} fp32 [N, K]  the reference's plain result (actorder=False, static_groups=False) on the same data
The order must be unambiguous: fp32 sums of T <= 512 squares differ between accumulation orders by about T * 2^-24 = 3e-5 relative, so the sorted
diagonal's neighbours are kept at least 1e-3 apart (asserted).  calibration()'s 1/16 grid makes exact ties; here the sorted column energies are
pushed onto a ladder -- each at most (1 - 2e-3) x the one before -- before the fp16 rounding, which keeps the hot channels' spread.  The generator
also asserts that on every non-edge file the reference's own act-order / plain proxy-loss ratio is below 0.8, so the inputs can show the effect.
The edge file (32 x 256, group 128) holds in group 0 an all-zero group (row 0), an all-positive group (row 1), a group of {0, 2^-24} whose scale
underflows fp16 (row 2: the 2^-24 floor), and a dead column (X[:, 37] = 0).
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import HERE      # noqa: E402
from gen_golden_gptq import BITS, REF_AMQ      # noqa: E402

LADDER, GAP, LIMIT = 2e-3, 1e-3, 500 * 1024


def calibration(torch, g, T, K, dead=()):
    """gen_golden_gptq.calibration's correlated activations with hot channels, off the grid, the sorted column energies at least LADDER apart"""
    r = K // 8
    x = torch.randn(T, r, generator=g) @ (torch.randn(r, K, generator=g) / r ** 0.5) + 0.3 * torch.randn(T, K, generator=g)
    hot = torch.randperm(K, generator=g)[:max(2, K // 64)]
    x[:, hot] *= 12.0
    e = (x.double() ** 2).sum(0)
    order = torch.argsort(e, descending=True)
    target = e.clone()
    for a, b in zip(order[:-1].tolist(), order[1:].tolist()):
        target[b] = min(float(e[b]), float(target[a]) * (1.0 - LADDER))
    x = (x.double() * (target / e).sqrt()).float()
    for c in dead:
        x[:, c] = 0.0
    return x.half()


def reference(torch, GPTQ_METHOD, Quantizer, W, X, bits, group, variant):
    """(Q, loss, perm, U_p, dead) of the reference's fasterquant; perm and U_p (variant only) by the lines fasterquant itself runs, on the same H"""
    import gptq_solver_ref as ref
    lin = torch.nn.Linear(W.shape[1], W.shape[0], bias=False)
    with torch.no_grad():
        lin.weight.copy_(W.float())
    m = GPTQ_METHOD(lin)
    m.quantizer = Quantizer()
    m.quantizer.configure(bits, perchannel=True, sym=False, mse=False)
    for lo in range(0, X.shape[0], 64):                       # windows of 64 rows, as the hooks would deliver them
        m.add_batch(X[lo:lo + 64].unsqueeze(0), None)
    H = m.H.clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    d = torch.diag(H)
    perm = torch.argsort(d, descending=True)
    s = d[perm].double()
    gap = float(((s[:-1] - s[1:]) / s[:-1]).min())
    assert gap >= GAP, f"the sorted diagonal's closest neighbours are {gap:.3g} apart"
    U_p, none = ref.hinv_upper(H[perm][:, perm])
    assert not bool(none.any())
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        m.fasterquant(percdamp=0.01, groupsize=group, actorder=variant, static_groups=variant)
    err = float([ln for ln in buf.getvalue().splitlines() if ln.startswith("error")][0].split()[1])
    return lin.weight.data.clone(), err, perm, U_p, dead, gap


def case(torch, GPTQ_METHOD, Quantizer, W, X, G, path, ratio_below=None):
    import gptq_solver_ref as ref
    out = {"W": W.numpy(), "X": X.numpy(), "bits": np.array(BITS, np.int32), "group": np.int32(G)}
    H64 = ref.hessian(X)
    for bits in BITS:
        Q, err, perm, U_p, dead, gap = reference(torch, GPTQ_METHOD, Quantizer, W, X, bits, G, True)
        plain = reference(torch, GPTQ_METHOD, Quantizer, W, X, bits, G, False)[0]
        out["perm"], out["U_p"], out["dead"] = perm.numpy(), U_p.numpy(), dead.numpy()
        out[f"Q_b{bits}"], out[f"loss_b{bits}"], out[f"Qplain_b{bits}"] = Q.numpy(), np.float64(err), plain.numpy()
        W0 = W.clone()
        W0[:, dead] = 0
        ratio = ref.proxy_loss(W0, Q, H64) / ref.proxy_loss(W0, plain, H64)
        print(f"  b{bits}: act-order + static groups / plain = {ratio:.3f} (diagonal gap {gap:.3g})")
        assert ratio_below is None or ratio < ratio_below, ratio
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", os.path.basename(path), size, "bytes")
    assert size < LIMIT, size
    return out


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF_AMQ)
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    torch.cuda.synchronize = lambda *a, **k: None
    from quantization.gptq import GPTQ_METHOD, Quantizer

    cases = [(64, 256, 128, 256, 21), (64, 256, 64, 256, 22), (64, 256, 32, 256, 23), (64, 384, 128, 80, 24)]
    for N, K, G, T, seed in cases:                            # (K = 384: fewer rows than columns keep the file under the limit)
        g = torch.Generator().manual_seed(seed)
        W = (torch.randn(N, K, generator=g) * 0.02).half()
        X = calibration(torch, g, T, K)
        case(torch, GPTQ_METHOD, Quantizer, W, X, G, f"{HERE}/gptqact_{N}x{K}_g{G}.npz", ratio_below=0.8)

    N, K, G, T = 32, 256, 128, 256
    g = torch.Generator().manual_seed(25)
    W = (torch.randn(N, K, generator=g) * 0.02).half()
    W[0, 0:128] = 0.0
    W[1, 0:128] = W[1, 0:128].abs() + 0.004
    W[2, 0:128] = torch.tensor([0.0, 2.0 ** -24]).half().repeat(64)
    X = calibration(torch, g, T, K, dead=(37,))
    out = case(torch, GPTQ_METHOD, Quantizer, W, X, G, f"{HERE}/gptqact_edge.npz")
    assert bool(out["dead"][37]) and int(out["dead"].sum()) == 1


if __name__ == "__main__":
    main()
