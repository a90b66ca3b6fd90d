"""The three error-feedback solves (csrc/amq_solve_body.cuh: plain GPTQ, static groups under an order, OWQ) give, byte for byte, what the commit
recorded in tests/golden/solve_digests.json gave -- at every G x BITS instantiation, on a shape that takes every path of the shared body: N = 32
(two workgroups), K = 384 (block 0 without a previous tile, block 1 with 4, block 2 with 8: both LDS buffers, the prefetch under use).  The
restatement tests hold the arithmetic; this one reaches the instantiations they do not.  tests/golden/gen_solve_digests.py wrote the file."""
import hashlib
import json
import os
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_digests.json")
N, K = 32, 384
# OWQ with n_out = 130: nq = 254 and Kp = 256 -- a ragged last group, a last tile with 30 live rows and a block that is all outliers
CASES = ([("plain", g, b, 0) for g in (32, 64, 128) for b in (2, 3, 4)] + [("static", g, b, 0) for g in (32, 64, 128) for b in (2, 3, 4)]
         + [("owq", 128, b, n_out) for b in (2, 3, 4) for n_out in (0, 130)])
_INPUTS = []


def key(kind, group, bits, n_out):
    return f"{kind}_g{group}_b{bits}" + (f"_o{n_out}" if kind == "owq" else "")


def inputs():
    """(W fp16 [N, K], U fp32 [K, K]) -- the same bytes on any CPU: integers of a seeded CPU generator on binary grids (W: multiples of 2^-8 in
    [-0.375, 0.375]; U upper triangular, its diagonal 1 + j / 256 in [1, 2], the rest multiples of 2^-12 in [-2^-8, 2^-8]).  Drawn once."""
    if not _INPUTS:
        g = torch.Generator().manual_seed(20260384)
        W = (torch.randint(-96, 97, (N, K), generator=g).float() / 256.0).half()
        off = torch.randint(-16, 17, (K, K), generator=g).float() / 4096.0
        diag = 1.0 + torch.randint(0, 257, (K,), generator=g).float() / 256.0
        _INPUTS.append((W, torch.triu(off, 1) + torch.diag(diag)))
    return _INPUTS[0]


def interleave(group):
    """the group interleave of tests/test_gpu_gptq_actorder.py: a lane's 8 walk columns lie in different groups"""
    i = torch.arange(K)
    return (i % (K // group)) * group + i // (K // group)


def digest(kind, group, bits, n_out):
    """the sha256 of the bytes of W_q, scale, zero, row_loss and the info word of one solve (OWQ: of W_out and choice too); the info word is 0"""
    from amq_amd import ops
    W, U = inputs()
    Wd, Ud = W.to(DEV), U.to(DEV)
    extra = {}
    if kind == "owq":
        h, W_out, info = ops.owq_quantize(Wd, Ud, n_out, bits, group, return_info=True)
        extra = {"W_out": W_out.view(torch.int16), "choice": info.choice}
    elif kind == "static":
        h, info = ops.gptq_quantize(Wd, Ud, bits, group, return_info=True, perm=interleave(group).to(DEV), static_groups=True)
    else:
        h, info = ops.gptq_quantize(Wd, Ud, bits, group, return_info=True)
    assert info.nonfinite == 0, "the info word"
    parts = {"W_q": h.W_q, "scale": h.scale.view(torch.int16), "zero": h.zero.view(torch.int16), "row_loss": info.row_loss, **extra}
    out = {k: hashlib.sha256(v.cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in parts.items()}
    out["info"] = hashlib.sha256(struct.pack("<i", info.nonfinite)).hexdigest()
    return out


@pytest.mark.parametrize("kind,group,bits,n_out", CASES, ids=[key(*c) for c in CASES])
def test_bits_of_the_recorded_commit(kind, group, bits, n_out):
    doc = json.load(open(GOLDEN))
    got, want = digest(kind, group, bits, n_out), doc["cases"][key(kind, group, bits, n_out)]
    assert got == want, (f"{[k for k in want if got.get(k) != want[k]]} differ from commit {doc['commit'][:7]}; recorded under HIP {doc['hip']}, "
                         f"this run under HIP {torch.version.hip}")
