#!/usr/bin/env python3
"""Golden vectors for the quantizer's edge inputs, produced by the REAL reference on CPU -- same recipe, stubs and rules as gen_golden.py (data
only; no reference source travels).  Separate script so that the other fixtures are not regenerated.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_quant.py

One file, ``hqq_quant_edge.npz``: per input kind and bit-width (group 128, 64 x 512) the keys ``{kind}_W`` and ``{kind}_b{bits}_W_q | scale | zero |
W_deq``:
  grid     values on a 16-level grid, randint(0, 16) * 0.01 - 0.07: the solver's error RISES at its second iteration (stop = 1)
  flat     rows of constant groups (several constants, den <= 1e-4: scale 1) and all-zero groups (|e| = 0: the shrinkage's 0 - inf) among
           ordinary ones
  outlier  ordinary weights with a +65504 or a -65504 entry (the fp16 maximum) in some groups
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import _stubs, REF, HERE      # noqa: E402

N, K, G = 64, 512, 128


def inputs(torch):
    g = torch.Generator().manual_seed(777)
    grid = (torch.randint(0, 16, (N, K), generator=g).float() * 0.01 - 0.07).half()
    flat = (torch.randn(N, K, generator=g) * 0.02).half()
    flat[0:8] = 0.0                                        # all-zero groups
    flat[8:12, 0:128] = 0.03125                            # constant groups, next to ordinary ones in the same rows
    flat[12:16, 128:256] = -0.5
    flat[16:20, 256:384] = 3.0e-5                          # constant and tiny
    flat[20:24, 384:512] = torch.tensor([0.01, 0.01004]).half().repeat(64)      # two values 4e-5 apart: den <= 1e-4 with den != 0
    outlier = (torch.randn(N, K, generator=g) * 0.02).half()
    outlier[::7, 5] = 65504.0
    outlier[3::9, 300] = -65504.0
    # (no group holds BOTH signs: its 127 ordinary values would each be wrong by thousands, the tensor's mean error would sit near 36, where one
    # fp32 ulp is more than an iteration gains elsewhere -- the stop iteration is then an accident of the summation order, in the reference too)
    return {"grid": grid, "flat": flat, "outlier": outlier}


def main():
    sys.dont_write_bytecode = True
    sys.path[:0] = [_stubs(), REF]
    import torch
    from hqq.core.quantize import HQQLinear, BaseQuantizeConfig

    out = {"group_size": np.int32(G), "shape": np.array([N, K], np.int32)}
    for kind, W in inputs(torch).items():
        out[f"{kind}_W"] = W.numpy()
        for bits in (2, 3, 4):
            lin = torch.nn.Linear(K, N, bias=False).half()
            with torch.no_grad():
                lin.weight.copy_(W)
            h = HQQLinear(lin, BaseQuantizeConfig(nbits=bits, group_size=G, axis=1), compute_dtype=torch.float16, device="cpu", del_orig=False)
            assert int(h.meta["group_size"]) == G and int(h.meta["nbits"]) == bits
            p = f"{kind}_b{bits}_"
            out[p + "W_q"], out[p + "scale"], out[p + "zero"] = h.W_q.numpy(), h.meta["scale"].numpy(), h.meta["zero"].numpy()
            out[p + "W_deq"] = h.dequantize().numpy()
    np.savez_compressed(f"{HERE}/hqq_quant_edge.npz", **out)
    print("wrote hqq_quant_edge.npz", os.path.getsize(f"{HERE}/hqq_quant_edge.npz"), "bytes")


if __name__ == "__main__":
    main()
