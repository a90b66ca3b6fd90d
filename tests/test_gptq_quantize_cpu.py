"""CPU-only: the GPTQ solve's arithmetic and its C entry point's host side.

(a) tests/gptq_solver_ref.py with ``deploy=False`` (fp32 scale, the reference's fake-quant weight) against what the reference's own ``fasterquant``
    produced on the CPU (tests/golden/gptqsolve_*.npz, gen_golden_gptq.py): the proxy loss tr(dW H dW^T), H formed from X in fp64, within 1e-3
    relative of the reference's -- the sequential trailing update is the reference's algorithm.
(b) ``deploy=True`` (the kernel's rule: fp16 scale, the error feedback sees the deployed weight): loss <= 1.05 x the reference's and < 0.5 x
    round-to-nearest's (hqq_format.quantize_rtn at the same bits and group).  The observed ratios are printed.
(c) zero integral in [0, maxq]; the scales pass ops.check_scale_range.
(d) one refused call per validation rule of amq_gptq_quantize_f16, through the loaded library (made-up pointers: an accepted call would launch).
(e) amq_gptq_quantize_workspace_bytes against the formula include/amq_hip.h documents.
(f) ops.gptq_hinv on the CPU reproduces the fixtures' U and dead columns.
"""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch

from amq_amd import _lib, ops
from amq_amd.hqq_format import quantize_rtn
from oracle import hqq_ref

import gptq_solver_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "gptqsolve_*.npz")))
CASES = [(name, bits) for name in FILES for bits in (2, 3, 4)]
IDS = [f"{n[len('gptqsolve_'):]}_b{b}" for n, b in CASES]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """dict of torch tensors: W fp16 with its dead columns zeroed (what the caller of the solve hands it), W_orig, X, U, dead, group, Q_b*, loss_b*"""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = {k: torch.from_numpy(d[k]) for k in d.files if d[k].ndim}
    out.update({k: d[k].item() for k in d.files if not d[k].ndim})
    out["W_orig"] = out["W"]
    out["W"] = out["W"].clone()
    out["W"][:, out["dead"]] = 0
    out["H"] = ref.hessian(out["X"])
    return out


@functools.lru_cache(maxsize=None)
def restated(name, bits, deploy):
    """the restatement of one case, computed once and shared (tests/test_gpu_gptq_quantize.py compares the device with it)"""
    f = fixture(name)
    return ref.solve(f["W"], f["U"], bits, int(f["group"]), deploy=deploy)


def rtn_weights(W, bits, group):
    """what hqq_format.quantize_rtn's layer dequantizes to (fp16 arithmetic of Quantizer.dequantize), fp32 [N, K]"""
    h = quantize_rtn(W, bits, group)
    w = hqq_ref.dequantize(h.W_q.numpy(), h.scale.numpy(), h.zero.numpy(), bits, tuple(W.shape), group)
    return torch.from_numpy(np.asarray(w)).float().reshape(W.shape)


def test_the_fixture_list_is_complete():
    assert FILES == ["gptqsolve_64x256_g128", "gptqsolve_64x256_g32", "gptqsolve_64x256_g64", "gptqsolve_64x384_g128", "gptqsolve_edge"]
    for name in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 500 * 1024
        assert list(fixture(name)["bits"]) == [2, 3, 4]
    e = fixture("gptqsolve_edge")
    assert int(e["dead"].sum()) == 1 and bool((e["X"][:, e["dead"]] == 0).all())
    assert bool((e["W_orig"][0, :128] == 0).all()) and bool((e["W_orig"][1, :128] > 0).all())
    assert float(e["W_orig"][2, :128].max()) == 2.0 ** -24 and float(e["W_orig"][2, :128].min()) == 0.0


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_the_algorithm_is_the_reference_s(name, bits):
    f = fixture(name)
    got = restated(name, bits, False)
    assert got["nonfinite"] == 0
    ours = ref.proxy_loss(f["W"], got["W_hat"], f["H"])
    theirs = ref.proxy_loss(f["W"], f[f"Q_b{bits}"], f["H"])
    print(f"{name} b{bits}: proxy loss {ours:.6g} (reference {theirs:.6g}, ratio {ours / theirs:.6f}); "
          f"solver loss {got['loss']:.6g} (reference printed {f[f'loss_b{bits}']:.6g})")
    assert abs(ours - theirs) <= 1e-3 * theirs


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_the_deployed_rule_keeps_the_reference_s_quality(name, bits):
    f = fixture(name)
    group = int(f["group"])
    got = restated(name, bits, True)
    assert got["nonfinite"] == 0
    ours = ref.proxy_loss(f["W"], got["W_hat"], f["H"])
    theirs = ref.proxy_loss(f["W"], f[f"Q_b{bits}"], f["H"])
    rtn = ref.proxy_loss(f["W"], rtn_weights(f["W"], bits, group), f["H"])
    print(f"{name} b{bits}: deployed / reference {ours / theirs:.4f}, deployed / round-to-nearest {ours / rtn:.4f}, "
          f"round-to-nearest / reference {rtn / theirs:.3f}")
    assert ours <= 1.05 * theirs
    assert ours < 0.5 * rtn
    # the weights the error feedback saw are the weights Format A dequantizes to: (q - z) * s16 in fp16
    q = got["q"].reshape(f["W"].shape).half()
    z = got["zero"].repeat_interleave(group, 1).reshape(f["W"].shape)
    s = got["scale"].repeat_interleave(group, 1).reshape(f["W"].shape)
    assert torch.equal(((q - z) * s).float(), got["W_hat"])


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_zero_is_a_code_and_the_scale_is_in_range(name, bits):
    got = restated(name, bits, True)
    z = got["zero"].float()
    assert got["zero"].dtype == torch.float16 and got["scale"].dtype == torch.float16
    assert torch.equal(z, z.round()) and float(z.min()) >= 0 and float(z.max()) <= 2 ** bits - 1
    assert float(got["scale"].float().min()) >= 2.0 ** -24
    ops.check_scale_range(torch.cat([got["scale"], got["zero"]], 1).reshape(-1), bits, ops.MODE_HQQ, name)
    assert int(got["q"].min()) >= 0 and int(got["q"].max()) <= 2 ** bits - 1
    if name == "gptqsolve_edge":
        f = fixture(name)
        per_row = f["W"].shape[1] // int(f["group"])
        assert float(got["scale"][0 * per_row]) == float(torch.tensor(2.0 / (2 ** bits - 1)).half())       # all-zero group: -1 / +1
        assert float(got["zero"][1 * per_row]) == 0.0                                                       # all-positive group: xmin = 0
        assert float(got["scale"][2 * per_row]) == 2.0 ** -24                                               # the floor
        assert torch.equal(got["W_hat"][2, :128], f["W"][2, :128].float())
        assert bool((got["W_hat"][:, f["dead"]] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ (d) refusals
EINVAL, ESHAPE = -1, -2
one = ctypes.c_void_p(256)
NAMES = "W U N K bits group W_q scale zero row_loss info workspace workspace_bytes stream"
GOOD = dict(W=one, U=one, N=64, K=512, bits=4, group=128, W_q=one, scale=one, zero=one, row_loss=one, info=one, workspace=one,
            workspace_bytes=ref.workspace_bytes(64, 512, 128), stream=None)
REFUSED = [(f"{n} null", {n: None}, EINVAL) for n in ("W", "U", "W_q", "scale", "zero", "row_loss", "info", "workspace")] + [
    ("W misaligned", dict(W=ctypes.c_void_p(264)), EINVAL), ("U misaligned", dict(U=ctypes.c_void_p(260)), EINVAL),
    ("workspace misaligned", dict(workspace=ctypes.c_void_p(264)), EINVAL),
    ("bits 5", dict(bits=5), EINVAL), ("bits 1", dict(bits=1), EINVAL),
    ("group 256 (two blocks)", dict(group=256), ESHAPE), ("group 96", dict(group=96, K=384), ESHAPE), ("group 16", dict(group=16), ESHAPE),
    ("group 0", dict(group=0), ESHAPE), ("N % 16", dict(N=72), ESHAPE), ("N 0", dict(N=0), ESHAPE),
    ("K % 128", dict(K=448, group=64), ESHAPE), ("K 0", dict(K=0), ESHAPE),
    ("workspace one byte short", dict(workspace_bytes=ref.workspace_bytes(64, 512, 128) - 1), EINVAL),
    ("workspace 0", dict(workspace_bytes=0), EINVAL),
]
ORDER = [("null before bits", dict(U=None, bits=5), EINVAL, b"null"), ("bits before group", dict(bits=5, group=256), EINVAL, b"bits"),
         ("group 256 names its rule", dict(group=256), ESHAPE, b"two 128-column blocks"), ("group before N", dict(group=96, N=72), ESHAPE, b"groups of"),
         ("N before K", dict(N=72, K=448), ESHAPE, b"N "), ("shape before workspace", dict(K=448, workspace_bytes=0), ESHAPE, b"K"),
         ("workspace names its size", dict(workspace_bytes=16), EINVAL, b"workspace too small")]


def test_gptq_entry_refusals():
    lib = _lib.load()
    fn = lib.amq_gptq_quantize_f16
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


# ------------------------------------------------------------------------------------------------------------------ (e) workspace
@pytest.mark.parametrize("N,K,group", [(16, 128, 128), (64, 512, 32), (64, 384, 64), (272, 384, 128), (4096, 4096, 128), (11008, 4096, 128),
                                       (4096, 11008, 64), (32000, 4096, 32)])
def test_workspace_bytes_is_the_documented_formula(N, K, group):
    want = 5 * N * K + N
    assert _lib.load().amq_gptq_quantize_workspace_bytes(N, K, group) == want == ref.workspace_bytes(N, K, group)


def test_workspace_bytes_of_a_refused_shape_is_zero():
    lib = _lib.load()
    for N, K, group in [(64, 512, 256), (64, 384, 96), (72, 512, 128), (64, 448, 64), (0, 512, 128)]:
        assert lib.amq_gptq_quantize_workspace_bytes(N, K, group) == 0 == ref.workspace_bytes(N, K, group)


# ------------------------------------------------------------------------------------------------------------------ (f) the factorisation
@pytest.mark.parametrize("name", FILES)
def test_gptq_hinv_reproduces_the_fixture(name):
    f = fixture(name)
    acc = ops.GPTQHessian(f["X"].shape[1], "cpu")
    for lo in range(0, f["X"].shape[0], 64):
        acc.add_batch(f["X"][lo:lo + 64].unsqueeze(0))
    assert acc.nsamples == -(-f["X"].shape[0] // 64)
    assert torch.allclose(acc.H.double(), f["H"], rtol=1e-5, atol=1e-5 * float(f["H"].diagonal().mean()))
    before = acc.H.clone()
    U, dead, where = ops.gptq_hinv(acc.H, 0.01, return_where=True)
    assert where == "host" and torch.equal(acc.H, before), "H must not be modified"
    assert torch.equal(dead, f["dead"])
    assert U.dtype == torch.float32 and bool((U.tril(-1) == 0).all())
    assert torch.allclose(U.diagonal(), f["U"].diagonal(), rtol=1e-5, atol=0)
    assert torch.allclose(U, f["U"], rtol=1e-4, atol=1e-5 * float(f["U"].diagonal().mean()))


def test_gptq_hinv_names_the_layer_of_a_failed_factorisation():
    H = -torch.eye(128)
    with pytest.raises(ValueError, match="down_proj"):
        ops.gptq_hinv(H, 0.01, name="down_proj")
