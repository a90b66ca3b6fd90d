"""CPU-only: the quantizer's arithmetic and its C entry point's host side.

(a) tests/hqq_solver_ref.py -- the solver restated in torch fp32 with the device kernels' summation orders -- against what the reference's own
    quantizer produced on the CPU: the 15 ``hqq_*.npz`` fixtures and the edge inputs of ``hqq_quant_edge.npz`` (tests/golden/gen_golden_quant.py).
    W_q and scale bit for bit; zero equal, or one fp16 ulp apart in at most one group of a case (the summation order of a group's mean is the
    restatement's tree, not torch's); the stop iterations as recorded.
(b) one refused call per validation rule of amq_hqq_quantize_f16, through the loaded library (made-up pointers: an accepted call would launch).
(c) amq_hqq_quantize_workspace_bytes against the formula include/amq_hip.h documents.
"""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from amq_amd import _lib
from amq_amd.hqq_format import pack_rows

import hqq_solver_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the iteration whose zero the reference kept (the restatement's, recorded when the fixtures were first reproduced): 19 = ran all 20
STOPS = {"hqq_b4_64x384": 18, "hqq_g32_b2_64x512": 13, "hqq_g32_b3_64x512": 11, "hqq_g32_b4_64x512": 13, "hqq_g64_b3_64x512": 16,
         "hqq_g64_b4_64x512": 17}
EDGE_KINDS = ("grid", "flat", "outlier")


def fixture_cases():
    """[(id, loader)]: loader() -> dict(W, W_q, scale, zero, W_deq, nbits, group_size) of numpy arrays"""
    cases = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "hqq_*.npz"))):
        name = os.path.basename(path)[:-4]
        if name == "hqq_quant_edge":
            continue

        def load(path=path):
            d = np.load(path)
            return {k: d[k] for k in ("W", "W_q", "scale", "zero", "W_deq")} | {
                "nbits": int(d["nbits"]), "group_size": int(d["group_size"]) if "group_size" in d.files else 128}
        cases.append((name, load))
    for kind in EDGE_KINDS:
        for bits in (2, 3, 4):
            def load(kind=kind, bits=bits):
                d = np.load(os.path.join(GOLDEN, "hqq_quant_edge.npz"))
                p = f"{kind}_b{bits}_"
                return {"W": d[f"{kind}_W"], "W_q": d[p + "W_q"], "scale": d[p + "scale"], "zero": d[p + "zero"], "W_deq": d[p + "W_deq"],
                        "nbits": bits, "group_size": int(d["group_size"])}
            cases.append((f"edge_{kind}_b{bits}", load))
    return cases


CASES = fixture_cases()


def test_the_fixture_list_is_complete():
    assert len([n for n, _ in CASES if not n.startswith("edge_")]) == 15
    assert len([n for n, _ in CASES if n.startswith("edge_")]) == 9
    assert set(STOPS) <= {n for n, _ in CASES}


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_restatement_reproduces_the_reference(name):
    d = dict(CASES)[name]()
    got = ref.solve(torch.from_numpy(d["W"]), d["nbits"], d["group_size"])
    assert torch.equal(pack_rows(got["q"], d["nbits"]), torch.from_numpy(d["W_q"])), "W_q"
    assert torch.equal(got["scale"].reshape(-1), torch.from_numpy(d["scale"]).reshape(-1)), "scale"
    z, zr = got["zero"].reshape(-1), torch.from_numpy(d["zero"]).reshape(-1)
    differ = (z.view(torch.int16) != zr.view(torch.int16)) & ~((z == 0) & (zr == 0))
    assert int(differ.sum()) <= 1, f"zero differs in {int(differ.sum())} groups"
    if differ.any():
        i = int(differ.nonzero()[0])
        assert abs(int(z.view(torch.int16)[i]) - int(zr.view(torch.int16)[i])) == 1, "zero more than one fp16 ulp apart"
    if name.startswith("edge_grid"):
        assert got["stop"] == 1
        if d["nbits"] == 2:                 # the error RISES there: a clear decision
            assert float(got["mean_err"][1]) > float(got["mean_err"][0]) * 1.005
    elif not name.startswith("edge_"):
        assert got["stop"] == STOPS.get(name, 19)
    assert torch.isfinite(got["mean_err"]).all()


# ------------------------------------------------------------------------------------------------------------------ (b) refusals
EINVAL, ESHAPE = -1, -2
one = ctypes.c_void_p(256)
NAMES = "W N K bits group round_zero W_q scale zero info workspace workspace_bytes stream"
GOOD = dict(W=one, N=64, K=512, bits=4, group=128, round_zero=1, W_q=one, scale=one, zero=one, info=one, workspace=one,
            workspace_bytes=ref.workspace_bytes(64, 512, 128), stream=None)
REFUSED = [(f"{n} null", {n: None}, EINVAL) for n in ("W", "W_q", "scale", "zero", "info", "workspace")] + [
    ("bits 5", dict(bits=5), EINVAL), ("bits 1", dict(bits=1), EINVAL),
    ("group 384 (a multiple of 128 the kernels are not built for)", dict(group=384, K=768), ESHAPE),
    ("group 512", dict(group=512), ESHAPE), ("group 16", dict(group=16), ESHAPE), ("group 0", dict(group=0), ESHAPE),
    ("N % 16", dict(N=72), ESHAPE), ("N 0", dict(N=0), ESHAPE),
    ("K % group", dict(K=384, group=256), ESHAPE), ("K % 128", dict(K=448, group=64), ESHAPE), ("K 0", dict(K=0), ESHAPE),
    ("workspace one byte short", dict(workspace_bytes=ref.workspace_bytes(64, 512, 128) - 1), EINVAL),
    ("workspace 0", dict(workspace_bytes=0), EINVAL),
]
# the order: a null pointer is answered before a bad shape, bits before the group, the group before N, the shape before the workspace
ORDER = [("null before bits", dict(W=None, bits=5), EINVAL, b"null"), ("bits before group", dict(bits=5, group=384), EINVAL, b"bits"),
         ("group before N", dict(group=384, N=72), ESHAPE, b"groups of"), ("N before K", dict(N=72, K=448), ESHAPE, b"N "),
         ("shape before workspace", dict(K=448, workspace_bytes=0), ESHAPE, b"K")]


def test_quantize_entry_refusals():
    lib = _lib.load()
    fn = lib.amq_hqq_quantize_f16
    wrong = []
    for label, change, code in REFUSED:
        assert not set(change) - set(GOOD), label
        args = dict(GOOD, **change)
        rc = fn(*(args[n] for n in NAMES.split()))
        assert rc != 0, f"{label}: ACCEPTED a call the table holds as refused"
        if rc != code:
            wrong.append((label, code, rc, lib.amq_last_error().decode()))
    assert not wrong, f"(rule, expected, got, message) {wrong}"
    for label, change, code, word in ORDER:
        args = dict(GOOD, **change)
        assert fn(*(args[n] for n in NAMES.split())) == code, label
        assert word in lib.amq_last_error(), (label, lib.amq_last_error())


# ------------------------------------------------------------------------------------------------------------------ (c) workspace
@pytest.mark.parametrize("N,K,group", [(64, 512, 128), (64, 512, 32), (64, 384, 128), (256, 1024, 64), (48, 11008, 64), (48, 11008, 128),
                                       (4096, 4096, 128), (11008, 4096, 128), (4096, 11008, 256), (32000, 4096, 32)])
def test_workspace_bytes_is_the_documented_formula(N, K, group):
    R = N * K // group
    P = R // 2 if group == 32 else R
    T = -(-P // 4096)
    wgs = -(-P // (4 * T))
    assert wgs <= 1024
    want = 4 * (21 * R + 21 * wgs)
    assert _lib.load().amq_hqq_quantize_workspace_bytes(N, K, group) == want == ref.workspace_bytes(N, K, group)


def test_workspace_bytes_of_a_refused_shape_is_zero():
    lib = _lib.load()
    assert lib.amq_hqq_quantize_workspace_bytes(64, 512, 384) == 0
    assert lib.amq_hqq_quantize_workspace_bytes(72, 512, 128) == 0
    assert lib.amq_hqq_quantize_workspace_bytes(64, 448, 64) == 0
