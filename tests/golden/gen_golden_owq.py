#!/usr/bin/env python3
"""Golden vectors for OWQ, produced by the REAL reference (amq/quantization/owq.py: GPTQ_OWQ.add_batch / hessian_sorting / fasterquant with its
Quantizer(mse=True), asymmetric, per channel, act_order=False, percdamp 0.01, groups of 128) on the CPU -- data only; no reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_owq.py

One file per case, ``owqsolve_{N}x{K}_o{n_out}.npz`` (and ``owqsolve_edge.npz``), each holding
  W          fp16 [N, K]   the dense weights (a dead column still holds its values: the solve zeroes it, as owq.py:332-334 does)
  X          fp16 [T, K]   the calibration rows (gen_golden_gptq.calibration: correlated channels, a few hot ones)
  H_diag     fp32 [K]      the diagonal of the reference's own accumulated Hessian (the whole matrix would double the file: the tests rebuild it
                           from X with ops.GPTQHessian, the reference's accumulation, and hold its diagonal against this one)
  n_out      int32
  bits       int32 [3]     2, 3, 4
and per bit-width b
  ids_b      int64 [K]     the reference's permutation (kept columns ascending, then the outliers in descending sensitivity)
  out_ids_b  int32 [n_out] the outliers ascending
  frob_b     fp32 [K]      frob_norm_error: the column sums of (W - W_quant)^2 of the whole-row search (num = 40)
  sens_b     fp32 [K]      diag(H) * frob_norm_error
  Q_b        fp32 [N, K]   the reference's fake-quantized result in the ORIGINAL column order, the updated outlier columns included
  scale_b, zero_b  fp32 [N, G]   the reference's per-group parameters (what find_params left before each group's first column)
The generator asserts that the n_out + 1 largest sens differ from one another by more than 1 % at every bit-width, so that the column choice and
the outliers' order in ids can be compared exactly: n_out = 4 is calibration()'s own four hot channels of K = 256; for 128 and 130 see ladder().  ``fasterquant`` calls torch.cuda.synchronize() unconditionally: stubbed here.
The edge file (32 x 256, n_out = 0) holds in block 0 an all-zero group (row 0), an all-positive group (row 1), a group of {0, 2^-24} whose step
underflows fp16 (row 2: the 2^-24 floor), and a dead column (X[:, 37] = 0).

``owq_n_out.json``: the reference's number of fp16 columns (owq.py:69-70, 146-153 with its own model_config.json ratios) for the Llama-2-7B shapes
at average 2.25 / 3.25 / 4.25 bits.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import REF, HERE      # noqa: E402
from gen_golden_gptq import calibration      # noqa: E402

REF_AMQ = os.path.dirname(os.path.dirname(REF))
BITS = (2, 3, 4)
GROUP = 128


def reference(torch, GPTQ_OWQ, Quantizer, W, X, bits, n_out):
    lin = torch.nn.Linear(W.shape[1], W.shape[0], bias=False)
    with torch.no_grad():
        lin.weight.copy_(W.float())
    m = GPTQ_OWQ(lin, n_out=n_out)
    m.quantizer = Quantizer(bits, perchannel=True, sym=False, mse=True)
    m.quantizer.n_out = n_out
    for lo in range(0, X.shape[0], 64):                       # windows of 64 rows, as the hooks would deliver them
        m.add_batch(X[lo:lo + 64].unsqueeze(0), None)
    H = m.H.clone()
    Wf = lin.weight.data.clone().to(torch.float)
    tq = Quantizer(bits, perchannel=True, sym=False, mse=True)
    tq.find_params(Wf, weight=True, num=40)
    frob = (Wf - tq.quantize(Wf)).pow(2).sum(dim=0)
    sens = torch.diag(H) * frob
    out_ids = m.hessian_sorting(actorder=False, frob_norm=frob)
    ids = m.ids.clone() if m.ids is not None else torch.arange(W.shape[1])
    groups = []
    inner = m.quantizer.find_params

    def recording(x, weight=False, num=100):
        inner(x, weight=weight, num=num)
        if num == 40:
            groups.append((m.quantizer.scale.clone().reshape(-1), m.quantizer.zero.clone().reshape(-1)))

    m.quantizer.find_params = recording
    m.fasterquant(percdamp=0.01, groupsize=GROUP, actorder=False)
    return {"ids": ids.numpy().astype(np.int64), "out_ids": out_ids.numpy().astype(np.int32), "frob": frob.numpy(), "sens": sens.numpy(),
            "Q": lin.weight.data.clone().numpy(), "scale": torch.stack([g[0] for g in groups], 1).numpy(),
            "zero": torch.stack([g[1] for g in groups], 1).numpy()}, H


def ladder(torch, g, W, X, n_out):
    """More outliers than calibration() made hot channels.  ids lists the outliers by descending sens, and the deployed rule moves a column's
    round-off by a fraction of a percent against the reference's, so n_out random sens values would not keep their order: the n_out chosen columns
    of W are made one and the same column (the whole-row search then leaves them the same round-off, in the reference and here), and their
    activations' energies a ladder of 2 % steps from 48 times the median column's upwards (calibration()'s hot channels are among the chosen; hotter still, and the fp16 rounding of the outlier columns, which the reference's fp32 layer does not have, would show in the loss) -- the order is the ladder's."""
    N, K = W.shape
    energy = X.float().pow(2).sum(0)
    base = float(energy.median())
    hot = torch.argsort(energy, descending=True)[:max(2, K // 64)]          # calibration()'s hot channels are among the chosen
    rest = torch.randperm(K, generator=g)
    chosen = torch.cat([hot, rest[~torch.isin(rest, hot)]])[:n_out]
    for rank, c in enumerate(chosen.tolist()):
        target = base * 48.0 * 1.02 ** (n_out - 1 - rank)
        X[:, c] = (X[:, c].float() * (target / float(energy[c])) ** 0.5).half()
    W[:, chosen] = (torch.randn(N, 1, generator=g) * 0.02).half()


def case(torch, GPTQ_OWQ, Quantizer, W, X, n_out):
    out = {"W": W.numpy(), "X": X.numpy(), "bits": np.array(BITS, np.int32), "n_out": np.int32(n_out)}
    for bits in BITS:
        got, H = reference(torch, GPTQ_OWQ, Quantizer, W, X, bits, n_out)
        out["H_diag"] = torch.diag(H).numpy()
        for k, v in got.items():
            out[f"{k}_b{bits}"] = v
        if n_out:                                                 # the choice AND the outliers' order (ids lists them by descending sens) are clear
            s = np.sort(got["sens"])[::-1]
            assert (s[:n_out] > 1.01 * s[1:n_out + 1]).all(), (n_out, bits, (s[:n_out] / s[1:n_out + 1]).min())
    return out


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF_AMQ)
    import torch
    torch.cuda.synchronize = lambda *a, **k: None
    from quantization.owq import GPTQ_OWQ, Quantizer, processing_meta

    cases = [(64, 256, 0, 256, 21), (64, 256, 4, 256, 22), (64, 256, 128, 256, 23), (64, 384, 130, 288, 24)]
    for N, K, n_out, T, seed in cases:
        g = torch.Generator().manual_seed(seed)
        W = (torch.randn(N, K, generator=g) * 0.02).half()
        X = calibration(torch, g, T, K, grid=16 if K <= 256 else 8)
        if n_out > max(2, K // 64):
            ladder(torch, g, W, X, n_out)
        out = case(torch, GPTQ_OWQ, Quantizer, W, X, n_out)
        path = f"{HERE}/owqsolve_{N}x{K}_o{int(out['n_out'])}.npz"
        np.savez_compressed(path, **out)
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")

    N, K, T = 32, 256, 256
    g = torch.Generator().manual_seed(25)
    W = (torch.randn(N, K, generator=g) * 0.02).half()
    W[0, 0:128] = 0.0
    W[1, 0:128] = W[1, 0:128].abs() + 0.004
    W[2, 0:128] = torch.tensor([0.0, 2.0 ** -24]).half().repeat(64)
    X = calibration(torch, g, T, K, dead=(37,))
    out = case(torch, GPTQ_OWQ, Quantizer, W, X, 0)
    assert float(out["H_diag"][37]) == 0.0 and int((out["H_diag"] == 0).sum()) == 1
    path = f"{HERE}/owqsolve_edge.npz"
    np.savez_compressed(path, **out)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")

    # the n_out rule (owq.py:69-70, 146-153) for the Llama-2-7B shapes
    meta = processing_meta("llama-2-7b-hf")
    shapes = {"self_attn.q_proj": 4096, "self_attn.k_proj": 4096, "self_attn.v_proj": 4096, "self_attn.o_proj": 4096, "mlp.up_proj": 4096,
              "mlp.gate_proj": 4096, "mlp.down_proj": 11008}
    rule = {}
    for avg in (2.25, 3.25, 4.25):
        avg_bits = avg - 32 / GROUP
        r = (12 / (16 - avg_bits)) * 0.1
        r /= sum(meta["owq_layers"].values())
        rule[str(avg)] = {}
        for name, K in shapes.items():
            n = round(K * r * meta["ratios"][name])
            if n % 2 == 1:
                n += 1
            rule[str(avg)][name] = [K, n]
    with open(f"{HERE}/owq_n_out.json", "w") as f:
        json.dump(rule, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote owq_n_out.json", rule)


if __name__ == "__main__":
    main()
