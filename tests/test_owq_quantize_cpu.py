"""CPU-only: OWQ's arithmetic (tests/owq_ref.py, written from the specification in include/amq_hip.h / DESIGN.md 3.12) against what the reference's
own GPTQ_OWQ + Quantizer(mse=True) produced on the CPU (tests/golden/owqsolve_*.npz, gen_golden_owq.py), and the host side of the C entry points.

(a) ``owq_ref.select`` reproduces every fixture's ``out_ids`` and ``ids`` exactly (the generator made the choice clear by more than 1 %).
(b) ``owq_ref.solve(deploy=False)``: the proxy loss tr(dW H dW^T) over all K columns, the outliers' change included, is no worse than 1.05 x the
    reference's Q's (the bound of tests/test_gpu_gptq_quantize.py).  The observed ratio is printed.
(c) ``deploy=True`` (the kernel's rule): the same bound, and < 0.5 x round-to-nearest's; the padding codes of a ragged last group dequantize to 0.
(d) the n_out rule reproduces what the generator recorded from the reference's formula for the 7B shapes at 2.25 / 3.25 / 4.25 bits.
(e) the ABI: symbols, workspace queries, one refused call per validation rule and their order (made-up pointers: an accepted call would launch).
"""
import ctypes
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

from amq_amd import _lib, ops

import gptq_solver_ref as gref
import owq_ref as ref
from test_gptq_quantize_cpu import rtn_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "owqsolve_*.npz")))
CASES = [(name, bits) for name in FILES for bits in (2, 3, 4)]
IDS = [f"{n[len('owqsolve_'):]}_b{b}" for n, b in CASES]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """dict of torch tensors: W fp16, X, n_out, H32 (ops.GPTQHessian over X on the CPU: the reference's accumulation), H (fp64, for the proxy
    loss), and per bits ids_b*, out_ids_b*, frob_b*, sens_b*, Q_b*, scale_b*, zero_b*"""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = {k: torch.from_numpy(d[k]) for k in d.files if d[k].ndim}
    out.update({k: d[k].item() for k in d.files if not d[k].ndim})
    acc = ops.GPTQHessian(out["X"].shape[1], "cpu")
    for lo in range(0, out["X"].shape[0], 64):
        acc.add_batch(out["X"][lo:lo + 64].unsqueeze(0))
    out["H32"] = acc.H
    assert torch.allclose(torch.diag(acc.H), out["H_diag"], rtol=1e-5, atol=0), "the rebuilt Hessian is not the reference's"
    out["H"] = gref.hessian(out["X"])
    return out


@functools.lru_cache(maxsize=None)
def permuted(name, bits):
    """(W_p fp16 with its dead columns zeroed, U_p, ids, dead in the permuted order, W0: W in the original order with the dead columns zeroed)"""
    f = fixture(name)
    ids = f[f"ids_b{bits}"]
    U, dead = ops.gptq_hinv(f["H32"][ids][:, ids], 0.01)
    Wp = f["W"][:, ids].clone()
    Wp[:, dead] = 0
    W0 = f["W"].clone()
    W0[:, ids[dead]] = 0
    return Wp, U, ids, dead, W0


@functools.lru_cache(maxsize=None)
def restated(name, bits, deploy):
    """the restatement of one case (its own search, the score in fp64), computed once and shared"""
    Wp, U, _, _, _ = permuted(name, bits)
    return ref.solve(Wp, U, int(fixture(name)["n_out"]), bits, deploy=deploy)


def losses(name, bits, dense_p):
    """(ours, the reference's, round-to-nearest's) proxy loss over all K columns"""
    f = fixture(name)
    _, _, ids, _, W0 = permuted(name, bits)
    ours = gref.proxy_loss(W0, ref.unpermute(dense_p, ids), f["H"])
    theirs = gref.proxy_loss(W0, f[f"Q_b{bits}"], f["H"])
    rtn = gref.proxy_loss(W0, rtn_weights(W0, bits, 128), f["H"])
    return ours, theirs, rtn


def test_the_fixture_list_is_complete():
    assert FILES == ["owqsolve_64x256_o0", "owqsolve_64x256_o128", "owqsolve_64x256_o4", "owqsolve_64x384_o130", "owqsolve_edge"]
    for name in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 500 * 1024
        f = fixture(name)
        assert list(f["bits"]) == [2, 3, 4]
        for bits in (2, 3, 4):
            n_out = int(f["n_out"])
            assert f[f"out_ids_b{bits}"].numel() == n_out and sorted(f[f"ids_b{bits}"].tolist()) == list(range(f["W"].shape[1]))
            if n_out:
                s = f[f"sens_b{bits}"].sort(descending=True)[0]
                assert float(s[n_out - 1]) > 1.01 * float(s[n_out])
    e = fixture("owqsolve_edge")
    assert int((e["H_diag"] == 0).sum()) == 1 and bool((e["X"][:, 37] == 0).all())
    assert bool((e["W"][0, :128] == 0).all()) and bool((e["W"][1, :128] > 0).all())
    assert float(e["W"][2, :128].max()) == 2.0 ** -24 and float(e["W"][2, :128].min()) == 0.0


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_select_reproduces_the_reference_s_columns(name, bits):
    f = fixture(name)
    ids, out_ids, frob, _ = ref.select(f["W"], f["H32"], int(f["n_out"]), bits)
    assert torch.equal(out_ids, f[f"out_ids_b{bits}"]) and out_ids.dtype == torch.int32
    assert torch.equal(ids, f[f"ids_b{bits}"])
    # the deployed rule moves the columns' round-off a little, never the order of magnitude
    assert float((frob / f[f"frob_b{bits}"]).max()) < 1.5 and float((frob / f[f"frob_b{bits}"]).min()) > 0.67


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_the_algorithm_is_the_reference_s(name, bits):
    got = restated(name, bits, False)
    assert got["nonfinite"] == 0
    ours, theirs, _ = losses(name, bits, got["dense_p"])
    print(f"{name} b{bits}: proxy loss {ours:.6g} (reference {theirs:.6g}, ratio {ours / theirs:.6f})")
    assert ours <= 1.05 * theirs


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_the_deployed_rule_keeps_the_reference_s_quality(name, bits):
    f = fixture(name)
    got = restated(name, bits, True)
    assert got["nonfinite"] == 0
    ours, theirs, rtn = losses(name, bits, got["dense_p"])
    print(f"{name} b{bits}: deployed / reference {ours / theirs:.4f}, deployed / round-to-nearest {ours / rtn:.4f}")
    assert ours <= 1.05 * theirs
    assert ours < 0.5 * rtn
    # the weights the error feedback saw are the weights Format A dequantizes to, and the padding dequantizes to exactly 0
    N, K = f["W"].shape
    nq, Kp = K - int(f["n_out"]), ref.packed_columns(K, int(f["n_out"]))
    q = got["q"].reshape(N, Kp).half()
    z = got["zero"].repeat_interleave(128, 1).reshape(N, Kp)
    s = got["scale"].repeat_interleave(128, 1).reshape(N, Kp)
    w = ((q - z) * s).float()
    assert torch.equal(w[:, :nq], got["W_hat"])
    assert bool((w[:, nq:] == 0).all()) and bool((q[:, nq:] == z[:, nq:]).all())
    zf = got["zero"].float()
    assert torch.equal(zf, zf.round()) and float(zf.min()) >= 0 and float(zf.max()) <= 2 ** bits - 1
    assert float(got["scale"].float().min()) >= 2.0 ** -24
    assert got["W_out"].dtype == torch.float16 and tuple(got["W_out"].shape) == (N, int(f["n_out"]))
    if name == "owqsolve_edge":
        assert float(got["scale"][0 * (Kp // 128)]) == 2.0 ** -24 and bool((got["W_hat"][0, :128] == 0).all())      # the all-zero group
        assert float(got["scale"][2 * (Kp // 128)]) == 2.0 ** -24                                                   # the floor
        assert bool((got["W_hat"][:, 37] == 0).all())                                                               # the dead column


def test_the_n_out_rule_is_the_reference_s():
    from amq_amd.patching import owq_n_out
    rule = json.load(open(os.path.join(GOLDEN, "owq_n_out.json")))
    assert sorted(rule) == ["2.25", "3.25", "4.25"]
    for avg, per in rule.items():
        assert len(per) == 7
        for name, (K, want) in per.items():
            assert owq_n_out(K, float(avg), name) == want == ref.n_out_rule(K, float(avg), name), (avg, name)
            assert want % 2 == 0


# ------------------------------------------------------------------------------------------------------------------ (e) the ABI
EINVAL, ESHAPE = -1, -2
one = ctypes.c_void_p(256)


def _refused(fn, names, good, table):
    lib = _lib.load()
    wrong = []
    for label, change, code, word in table:
        assert not set(change) - set(good), label
        args = dict(good, **change)
        rc = fn(*(args[n] for n in names.split()))
        assert rc != 0, f"{label}: ACCEPTED a call the table holds as refused"
        if rc != code or (word is not None and word not in lib.amq_last_error()):
            wrong.append((label, code, rc, lib.amq_last_error().decode()))
    assert not wrong, f"(rule, expected, got, message) {wrong}"


def test_owq_quantize_entry_refusals_and_their_order():
    names = "W_p U_p N K n_out bits group num W_q scale zero W_out choice row_loss info workspace workspace_bytes stream"
    good = dict(W_p=one, U_p=one, N=64, K=512, n_out=6, bits=4, group=128, num=40, W_q=one, scale=one, zero=one, W_out=one, choice=one,
                row_loss=one, info=one, workspace=one, workspace_bytes=ref.workspace_bytes(64, 512, 6), stream=None)
    table = [(f"{n} null", {n: None}, EINVAL, b"null") for n in ("W_p", "U_p", "W_q", "scale", "zero", "W_out", "choice", "row_loss", "info",
                                                                  "workspace")] + [
        ("W_p misaligned", dict(W_p=ctypes.c_void_p(264)), EINVAL, b"aligned"), ("U_p misaligned", dict(U_p=ctypes.c_void_p(260)), EINVAL, None),
        ("workspace misaligned", dict(workspace=ctypes.c_void_p(264)), EINVAL, None),
        ("bits 5", dict(bits=5), EINVAL, b"bits"), ("bits 1", dict(bits=1), EINVAL, b"bits"),
        ("group 32", dict(group=32), ESHAPE, b"groups of 128 only"), ("group 64", dict(group=64), ESHAPE, b"groups of 128 only"),
        ("group 256", dict(group=256), ESHAPE, b"groups of 128 only"), ("N % 16", dict(N=72), ESHAPE, b"N "), ("N 0", dict(N=0), ESHAPE, None),
        ("K % 128", dict(K=448), ESHAPE, b"K"), ("num 0", dict(num=0), ESHAPE, b"num"), ("num 101", dict(num=101), ESHAPE, b"num"),
        ("n_out odd", dict(n_out=5), ESHAPE, b"n_out"), ("n_out K", dict(n_out=512), ESHAPE, b"n_out"), ("n_out < 0", dict(n_out=-2), ESHAPE, b"n_out"),
        ("workspace one byte short", dict(workspace_bytes=ref.workspace_bytes(64, 512, 6) - 1), EINVAL, b"workspace too small"),
        # the order: pointers, bits, shape, workspace
        ("null before bits", dict(U_p=None, bits=5), EINVAL, b"null"), ("bits before group", dict(bits=5, group=64), EINVAL, b"bits"),
        ("group before N", dict(group=64, N=72), ESHAPE, b"groups of"), ("N before K", dict(N=72, K=448), ESHAPE, b"N "),
        ("K before num", dict(K=448, num=0), ESHAPE, b"K"), ("num before n_out", dict(num=0, n_out=5), ESHAPE, b"num"),
        ("shape before workspace", dict(n_out=5, workspace_bytes=0), ESHAPE, b"n_out")]
    _refused(_lib.load().amq_owq_quantize_f16, names, good, table)
    # n_out = 0 needs no W_out: only the workspace stops this call
    args = dict(good, n_out=0, W_out=None, workspace_bytes=0)
    assert _lib.load().amq_owq_quantize_f16(*(args[n] for n in names.split())) == EINVAL
    assert b"workspace too small" in _lib.load().amq_last_error()


def test_owq_range_and_layer_entry_refusals():
    lib = _lib.load()
    names = "W N K col0 L bits num scale zero choice score wq_err info stream"
    good = dict(W=one, N=64, K=512, col0=0, L=512, bits=3, num=40, scale=one, zero=one, choice=one, score=one, wq_err=None, info=one, stream=None)
    table = [(f"{n} null", {n: None}, EINVAL, b"null") for n in ("W", "scale", "zero", "choice", "score", "info")] + [
        ("choice misaligned", dict(choice=ctypes.c_void_p(258)), EINVAL, b"aligned"), ("bits 5", dict(bits=5), EINVAL, b"bits"),
        ("N % 16", dict(N=8), ESHAPE, b"N "), ("K % 128", dict(K=500, L=500), ESHAPE, b"K"), ("num 0", dict(num=0), ESHAPE, b"num"),
        ("segment past the row", dict(col0=128, L=512), ESHAPE, b"segment"), ("L 0", dict(L=0), ESHAPE, b"segment"),
        ("col0 < 0", dict(col0=-1), ESHAPE, b"segment"), ("L beyond LDS", dict(K=32768, L=32768), ESHAPE, b"LDS"),
        ("wq_err on a part of the row", dict(wq_err=one, L=384), ESHAPE, b"whole-row"),
        ("null before bits", dict(score=None, bits=5), EINVAL, b"null"), ("bits before shape", dict(bits=5, N=8), EINVAL, b"bits")]
    _refused(lib.amq_owq_range_f16, names, good, table)
    names = "x M K perm Kp xg stream"
    good = dict(x=one, M=4, K=512, perm=one, Kp=384, xg=one, stream=None)
    _refused(lib.amq_owq_gather_f16, names, good, [("x null", dict(x=None), EINVAL, b"null"), ("perm null", dict(perm=None), EINVAL, b"null"),
                                                   ("xg null", dict(xg=None), EINVAL, b"null"), ("M 0", dict(M=0), ESHAPE, b"M"),
                                                   ("Kp % 128", dict(Kp=380), ESHAPE, b"Kp"), ("null before M", dict(x=None, M=0), EINVAL, b"null")])
    names = "x M K out_ids n_out W_out y N stream"
    good = dict(x=one, M=4, K=512, out_ids=one, n_out=6, W_out=one, y=one, N=64, stream=None)
    _refused(lib.amq_owq_outlier_add_f16, names, good, [(f"{n} null", {n: None}, EINVAL, b"null") for n in ("x", "out_ids", "W_out", "y")] + [
        ("M 0", dict(M=0), ESHAPE, b"M"), ("M beyond the grid", dict(M=65536), ESHAPE, b"M"), ("n_out 0", dict(n_out=0), ESHAPE, b"n_out"),
        ("n_out K", dict(n_out=512), ESHAPE, b"n_out")])


@pytest.mark.parametrize("N,K,n_out", [(16, 128, 0), (16, 128, 2), (64, 256, 128), (80, 384, 130), (4096, 4096, 54), (4096, 11008, 54)])
def test_workspace_bytes_is_the_documented_formula(N, K, n_out):
    Kp = -(-(K - n_out) // 128) * 128
    assert _lib.load().amq_owq_quantize_workspace_bytes(N, K, n_out, 128) == 5 * N * Kp + N == ref.workspace_bytes(N, K, n_out)
    assert ops.owq_packed_columns(K, n_out) == Kp == ref.packed_columns(K, n_out)


def test_workspace_bytes_of_a_refused_shape_is_zero():
    lib = _lib.load()
    for N, K, n_out, group in [(64, 512, 6, 64), (64, 512, 6, 256), (64, 512, 6, 32), (72, 512, 6, 128), (64, 448, 6, 128), (64, 512, 5, 128),
                               (64, 512, 512, 128), (0, 512, 0, 128)]:
        assert lib.amq_owq_quantize_workspace_bytes(N, K, n_out, group) == 0 == ref.workspace_bytes(N, K, n_out, group)


def test_python_refuses_other_groups_with_a_sentence():
    for group in (32, 64, 256):
        with pytest.raises(ValueError, match="groups of 128 only"):
            ops.owq_quantize_buffers(64, 512, 6, 3, group, torch.device("cpu"))
