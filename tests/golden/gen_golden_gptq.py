#!/usr/bin/env python3
"""Golden vectors for the GPTQ solve, produced by the REAL reference (amq/quantization/gptq.py: GPTQ_METHOD.add_batch / fasterquant with its
Quantizer, asymmetric, act_order=False, static_groups=False, percdamp 0.01) on the CPU -- data only; no reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_gptq.py

One file per shape and group size, ``gptqsolve_{N}x{K}_g{G}.npz`` (and ``gptqsolve_edge.npz``), each holding
  W         fp16 [N, K]   the dense weights (a dead column still holds its values: the caller zeroes it, as gptq.py:226-228 does)
  X         fp16 [T, K]   the calibration rows (correlated channels, a few hot ones; multiples of 1/16 so that the file compresses)
  U         fp32 [K, K]   the upper Cholesky factor of the damped inverse Hessian, from the reference's own three linalg calls on its own fp32 H
  dead      bool [K]      columns whose Hessian diagonal is 0
  bits      int32 [3]     2, 3, 4
  group     int32
  Q_b{bits} fp32 [N, K]   the reference's fake-quantized weights (an fp32 layer, so nothing is rounded on the way out)
  loss_b{bits} fp64       the reference's printed `error` (sum of its Losses)
``fasterquant`` calls torch.cuda.synchronize() unconditionally: stubbed here.  The edge file (32 x 256, group 128) holds in block 0 an all-zero
group (row 0), an all-positive group (row 1), a group of {0, 2^-24} whose scale underflows fp16 (row 2: the 2^-24 floor), a dead column (X[:, 37] = 0)
and hot channels in X.
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import REF, HERE      # noqa: E402

REF_AMQ = os.path.dirname(os.path.dirname(REF))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
BITS = (2, 3, 4)


def calibration(torch, g, T, K, dead=(), grid=16):
    """correlated activations (K / 8 common factors under channel noise of 0.3) with hot channels, on a 1/grid grid"""
    r = K // 8
    x = torch.randn(T, r, generator=g) @ (torch.randn(r, K, generator=g) / r ** 0.5) + 0.3 * torch.randn(T, K, generator=g)
    hot = torch.randperm(K, generator=g)[:max(2, K // 64)]
    x[:, hot] *= 12.0
    x = (x * grid).round() / grid
    for c in dead:
        x[:, c] = 0.0
    return x.half()


def reference(torch, GPTQ_METHOD, Quantizer, W, X, bits, group):
    import gptq_solver_ref as ref
    lin = torch.nn.Linear(W.shape[1], W.shape[0], bias=False)
    with torch.no_grad():
        lin.weight.copy_(W.float())
    m = GPTQ_METHOD(lin)
    m.quantizer = Quantizer()
    m.quantizer.configure(bits, perchannel=True, sym=False, mse=False)
    for lo in range(0, X.shape[0], 64):                       # windows of 64 rows, as the hooks would deliver them
        m.add_batch(X[lo:lo + 64].unsqueeze(0), None)
    U, dead = ref.hinv_upper(m.H.clone())                     # the same three calls fasterquant makes below, on the same H
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        m.fasterquant(percdamp=0.01, groupsize=group, actorder=False, static_groups=False)
    err = float([ln for ln in buf.getvalue().splitlines() if ln.startswith("error")][0].split()[1])
    return lin.weight.data.clone(), U, dead, err


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF_AMQ)
    import torch
    torch.cuda.synchronize = lambda *a, **k: None
    from quantization.gptq import GPTQ_METHOD, Quantizer

    cases = [(64, 256, 128, 256, 11), (64, 256, 64, 256, 12), (64, 256, 32, 256, 13), (64, 384, 128, 288, 14)]
    for N, K, G, T, seed in cases:
        g = torch.Generator().manual_seed(seed)
        W = (torch.randn(N, K, generator=g) * 0.02).half()
        X = calibration(torch, g, T, K, grid=16 if K <= 256 else 8)       # (K = 384: fewer rows than columns and a coarser grid keep the file small)
        out = {"W": W.numpy(), "X": X.numpy(), "bits": np.array(BITS, np.int32), "group": np.int32(G)}
        for bits in BITS:
            Q, U, dead, err = reference(torch, GPTQ_METHOD, Quantizer, W, X, bits, G)
            out["U"], out["dead"] = U.numpy(), dead.numpy()
            out[f"Q_b{bits}"], out[f"loss_b{bits}"] = Q.numpy(), np.float64(err)
        path = f"{HERE}/gptqsolve_{N}x{K}_g{G}.npz"
        np.savez_compressed(path, **out)
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")

    N, K, G, T = 32, 256, 128, 256
    g = torch.Generator().manual_seed(15)
    W = (torch.randn(N, K, generator=g) * 0.02).half()
    W[0, 0:128] = 0.0
    W[1, 0:128] = W[1, 0:128].abs() + 0.004
    W[2, 0:128] = torch.tensor([0.0, 2.0 ** -24]).half().repeat(64)
    X = calibration(torch, g, T, K, dead=(37,))
    out = {"W": W.numpy(), "X": X.numpy(), "bits": np.array(BITS, np.int32), "group": np.int32(G)}
    for bits in BITS:
        Q, U, dead, err = reference(torch, GPTQ_METHOD, Quantizer, W, X, bits, G)
        assert bool(dead[37]) and int(dead.sum()) == 1
        out["U"], out["dead"] = U.numpy(), dead.numpy()
        out[f"Q_b{bits}"], out[f"loss_b{bits}"] = Q.numpy(), np.float64(err)
    path = f"{HERE}/gptqsolve_edge.npz"
    np.savez_compressed(path, **out)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
