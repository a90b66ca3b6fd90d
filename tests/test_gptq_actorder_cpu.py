"""CPU-only: the arithmetic of the GPTQ solve with an activation order and static groups, and its C entry point's host side.

(a) tests/gptq_static_ref.py with ``deploy=False`` (fp32 scale, the reference's fake-quant weight) against what the reference's own
    ``fasterquant(actorder=True, static_groups=True)`` produced on the CPU (tests/golden/gptqact_*.npz, gen_golden_gptq_actorder.py): the proxy
    loss tr(dW H dW^T), H formed from X in fp64, within 1e-3 relative of the reference's (test_gptq_quantize_cpu.py's bound).
(b) ``deploy=True`` (the kernels' rule): loss <= 1.05 x the reference's, and strictly below the deployment-rule PLAIN restatement's
    (gptq_solver_ref.solve over the unpermuted factor) on the same fixture.  The observed ratios are printed.
(c) every (row, original group) holds codes in 0 .. 2^bits - 1 under one integer zero, and W_hat == fp16((q - z) * s16) exactly.
(d) ops.gptq_act_order: stable, dead entries rank as 1, equals the fixtures' perm.
(e) the ABI: symbols, signatures, workspace query, one refused call per validation rule (made-up pointers: an accepted call would launch).
"""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch

from amq_amd import _lib, ops

import gptq_solver_ref as plain
import gptq_static_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "gptqact_*.npz")))
CASES = [(name, bits) for name in FILES for bits in (2, 3, 4)]
IDS = [f"{n[len('gptqact_'):]}_b{b}" for n, b in CASES]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """dict of torch tensors: W fp16 with its dead columns zeroed (what the caller of the solve hands it), W_orig, X, perm, U_p, dead, group,
    Q_b*, loss_b*, Qplain_b*, H (fp64, from X)"""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = {k: torch.from_numpy(d[k]) for k in d.files if d[k].ndim}
    out.update({k: d[k].item() for k in d.files if not d[k].ndim})
    out["W_orig"] = out["W"]
    out["W"] = out["W"].clone()
    out["W"][:, out["dead"]] = 0
    out["H"] = plain.hessian(out["X"])
    return out


@functools.lru_cache(maxsize=None)
def restated(name, bits, deploy):
    """the restatement of one case, computed once and shared (tests/test_gpu_gptq_actorder.py compares the device with it)"""
    f = fixture(name)
    return ref.solve(f["W"], f["U_p"], f["perm"], bits, int(f["group"]), deploy=deploy)


@functools.lru_cache(maxsize=None)
def restated_plain(name, bits):
    """the deployment-rule PLAIN solve on the same data: the factor of the unpermuted Hessian, from the reference's three linalg calls on the
    fp32 Hessian ops.GPTQHessian accumulates"""
    f = fixture(name)
    acc = ops.GPTQHessian(f["X"].shape[1], "cpu")
    for lo in range(0, f["X"].shape[0], 64):
        acc.add_batch(f["X"][lo:lo + 64].unsqueeze(0))
    U, dead = plain.hinv_upper(acc.H)
    assert torch.equal(dead, f["dead"])
    return plain.solve(f["W"], U, bits, int(f["group"]), deploy=True)


def test_the_fixture_list_is_complete():
    assert FILES == ["gptqact_64x256_g128", "gptqact_64x256_g32", "gptqact_64x256_g64", "gptqact_64x384_g128", "gptqact_edge"]
    for name in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 500 * 1024
        f = fixture(name)
        K = f["W"].shape[1]
        assert list(f["bits"]) == [2, 3, 4]
        assert f["perm"].dtype == torch.int64 and torch.equal(torch.sort(f["perm"])[0], torch.arange(K))
        assert not torch.equal(f["perm"], torch.arange(K)), "an identity order shows nothing"
        d = torch.diag(f["H"]).clone()
        d[f["dead"]] = 1
        s = d[f["perm"]]
        assert float(((s[:-1] - s[1:]) / s[:-1]).min()) >= 1e-3, "the order must be unambiguous"
    e = fixture("gptqact_edge")
    assert int(e["dead"].sum()) == 1 and bool((e["X"][:, e["dead"]] == 0).all())
    assert bool((e["W_orig"][0, :128] == 0).all()) and bool((e["W_orig"][1, :128] > 0).all())
    assert float(e["W_orig"][2, :128].max()) == 2.0 ** -24 and float(e["W_orig"][2, :128].min()) == 0.0


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_the_algorithm_is_the_reference_s(name, bits):
    f = fixture(name)
    got = restated(name, bits, False)
    assert got["nonfinite"] == 0
    ours = plain.proxy_loss(f["W"], got["W_hat"], f["H"])
    theirs = plain.proxy_loss(f["W"], f[f"Q_b{bits}"], f["H"])
    print(f"{name} b{bits}: proxy loss {ours:.6g} (reference {theirs:.6g}, ratio {ours / theirs:.6f}); "
          f"solver loss {got['loss']:.6g} (reference printed {f[f'loss_b{bits}']:.6g})")
    assert abs(ours - theirs) <= 1e-3 * theirs


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_the_deployed_rule_keeps_the_reference_s_quality_and_beats_the_plain_solve(name, bits):
    f = fixture(name)
    got = restated(name, bits, True)
    assert got["nonfinite"] == 0
    ours = plain.proxy_loss(f["W"], got["W_hat"], f["H"])
    theirs = plain.proxy_loss(f["W"], f[f"Q_b{bits}"], f["H"])
    flat = plain.proxy_loss(f["W"], restated_plain(name, bits)["W_hat"], f["H"])
    ref_flat = plain.proxy_loss(f["W"], f[f"Qplain_b{bits}"], f["H"])
    print(f"{name} b{bits}: deployed / reference {ours / theirs:.4f}, deployed / deployed plain {ours / flat:.4f}, "
          f"reference / reference plain {theirs / ref_flat:.4f}")
    assert ours <= 1.05 * theirs
    assert ours < flat
    if name != "gptqact_edge":
        assert theirs < 0.8 * ref_flat, "the generator asserts this: the inputs can show the effect"


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_every_original_group_is_a_format_a_group(name, bits):
    f = fixture(name)
    group = int(f["group"])
    got = restated(name, bits, True)
    N, K = f["W"].shape
    z = got["zero"].float()
    assert got["zero"].dtype == torch.float16 and got["scale"].dtype == torch.float16
    assert tuple(got["q"].shape) == (N * K // group, group) and tuple(z.shape) == (N * K // group, 1)
    assert torch.equal(z, z.round()) and float(z.min()) >= 0 and float(z.max()) <= 2 ** bits - 1
    assert float(got["scale"].float().min()) >= 2.0 ** -24
    ops.check_scale_range(torch.cat([got["scale"], got["zero"]], 1).reshape(-1), bits, ops.MODE_HQQ, name)
    assert int(got["q"].min()) >= 0 and int(got["q"].max()) <= 2 ** bits - 1
    # the weights the error feedback saw are the weights Format A dequantizes to: (q - z) * s16 in fp16, per ORIGINAL group
    w = ((got["q"].half() - got["zero"]) * got["scale"]).float().reshape(N, K)
    assert torch.equal(w, got["W_hat"])
    # the parameters are the original groups': what the plain rule derives from W itself
    S, Z = ref.static_params(f["W"], bits, group, True)
    assert torch.equal(got["scale"].float().reshape(N, -1), S) and torch.equal(z.reshape(N, -1), Z)
    # the reference's own result keeps to 2^bits values per original group too
    Q = f[f"Q_b{bits}"].reshape(-1, group)
    assert max(len(torch.unique(row)) for row in Q) <= 2 ** bits
    if name == "gptqact_edge":
        per_row = K // group
        assert float(got["scale"][0 * per_row]) == float(torch.tensor(2.0 / (2 ** bits - 1)).half())       # all-zero group: -1 / +1
        assert float(got["zero"][1 * per_row]) == 0.0                                                       # all-positive group: xmin = 0
        assert float(got["scale"][2 * per_row]) == 2.0 ** -24                                               # the floor
        assert bool((got["W_hat"][:, f["dead"]] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ (d) the order
@pytest.mark.parametrize("name", FILES)
def test_gptq_act_order_is_the_fixture_s_perm(name):
    f = fixture(name)
    acc = ops.GPTQHessian(f["X"].shape[1], "cpu")
    for lo in range(0, f["X"].shape[0], 64):
        acc.add_batch(f["X"][lo:lo + 64].unsqueeze(0))
    before = acc.H.clone()
    perm = ops.gptq_act_order(acc.H)
    assert torch.equal(acc.H, before), "H must not be modified"
    assert perm.dtype == torch.int64 and perm.device == acc.H.device
    assert torch.equal(perm, f["perm"]) and torch.equal(perm, ref.act_order(acc.H))
    U, dead = ops.gptq_hinv(acc.H[perm][:, perm], 0.01)
    assert torch.allclose(U.diagonal(), f["U_p"].diagonal(), rtol=1e-5, atol=0)
    assert torch.allclose(U, f["U_p"], rtol=1e-4, atol=1e-5 * float(f["U_p"].diagonal().mean()))


def test_gptq_act_order_is_stable_and_ranks_dead_entries_as_one():
    d = torch.tensor([2.0, 0.5, 2.0, 0.0, 1.0, 3.0, 0.0, 0.5])       # dead: 3, 6 (rank as 1, with 4); ties: (0, 2), (3, 4, 6), (1, 7)
    H = torch.diag(d) + 0.01 * (1 - torch.eye(8))
    assert ops.gptq_act_order(H).tolist() == [5, 0, 2, 3, 4, 6, 1, 7]
    assert ops.gptq_act_order(torch.eye(16)).tolist() == list(range(16))
    assert float(H[3, 3]) == 0.0


# ------------------------------------------------------------------------------------------------------------------ (e) the ABI
EINVAL, ESHAPE = -1, -2
one = ctypes.c_void_p(256)
NAMES = "W U_p perm N K bits group W_q scale zero row_loss info workspace workspace_bytes stream"
GOOD = dict(W=one, U_p=one, perm=one, N=64, K=512, bits=4, group=128, W_q=one, scale=one, zero=one, row_loss=one, info=one, workspace=one,
            workspace_bytes=ref.workspace_bytes(64, 512, 128), stream=None)
REFUSED = [(f"{n} null", {n: None}, EINVAL) for n in ("W", "U_p", "perm", "W_q", "scale", "zero", "row_loss", "info", "workspace")] + [
    ("W misaligned", dict(W=ctypes.c_void_p(264)), EINVAL), ("U_p misaligned", dict(U_p=ctypes.c_void_p(260)), EINVAL),
    ("perm misaligned", dict(perm=ctypes.c_void_p(260)), EINVAL), ("workspace misaligned", dict(workspace=ctypes.c_void_p(264)), EINVAL),
    ("bits 5", dict(bits=5), EINVAL), ("bits 1", dict(bits=1), EINVAL),
    ("group 256 (two blocks)", dict(group=256), ESHAPE), ("group 96", dict(group=96, K=384), ESHAPE), ("group 16", dict(group=16), ESHAPE),
    ("group 0", dict(group=0), ESHAPE), ("N % 16", dict(N=72), ESHAPE), ("N 0", dict(N=0), ESHAPE),
    ("K % 128", dict(K=448, group=64), ESHAPE), ("K 0", dict(K=0), ESHAPE),
    ("workspace one byte short", dict(workspace_bytes=ref.workspace_bytes(64, 512, 128) - 1), EINVAL),
    ("workspace 0", dict(workspace_bytes=0), EINVAL),
]
ORDER = [("null before bits", dict(perm=None, bits=5), EINVAL, b"null"), ("bits before group", dict(bits=5, group=256), EINVAL, b"bits"),
         ("group 256 names its rule", dict(group=256), ESHAPE, b"two 128-column blocks"), ("group before N", dict(group=96, N=72), ESHAPE, b"groups of"),
         ("N before K", dict(N=72, K=448), ESHAPE, b"N "), ("shape before workspace", dict(K=448, workspace_bytes=0), ESHAPE, b"K"),
         ("workspace names its size", dict(workspace_bytes=16), EINVAL, b"workspace too small")]


def test_the_symbols_and_their_signatures():
    lib = _lib.load()
    plain_sig = _lib.SIGNATURES["amq_gptq_quantize_f16"]
    sig = _lib.SIGNATURES["amq_gptq_quantize_static_f16"]
    assert sig[0] is plain_sig[0] and sig[1] == plain_sig[1][:2] + [ctypes.c_void_p] + plain_sig[1][2:]      # the plain entry + perm after U
    assert _lib.SIGNATURES["amq_gptq_quantize_static_workspace_bytes"] == _lib.SIGNATURES["amq_gptq_quantize_workspace_bytes"]
    assert lib.amq_gptq_quantize_static_f16.argtypes == sig[1] and lib.amq_gptq_quantize_static_workspace_bytes.restype is ctypes.c_size_t
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "amq_hip.h")).read()
    assert "amq_gptq_quantize_static_f16(" in header and "amq_gptq_quantize_static_workspace_bytes(" in header


def test_static_entry_refusals():
    lib = _lib.load()
    fn = lib.amq_gptq_quantize_static_f16
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


@pytest.mark.parametrize("N,K,group", [(16, 128, 128), (64, 512, 32), (64, 384, 64), (272, 384, 128), (4096, 4096, 128), (11008, 4096, 128),
                                       (4096, 11008, 64), (32000, 4096, 32)])
def test_workspace_bytes_is_the_documented_formula(N, K, group):
    lib = _lib.load()
    want = 5 * N * K + N
    assert lib.amq_gptq_quantize_static_workspace_bytes(N, K, group) == want == ref.workspace_bytes(N, K, group)
    assert want == lib.amq_gptq_quantize_workspace_bytes(N, K, group)


def test_workspace_bytes_of_a_refused_shape_is_zero():
    lib = _lib.load()
    for N, K, group in [(64, 512, 256), (64, 384, 96), (72, 512, 128), (64, 448, 64), (0, 512, 128)]:
        assert lib.amq_gptq_quantize_static_workspace_bytes(N, K, group) == 0 == ref.workspace_bytes(N, K, group)


def test_perm_without_static_groups_is_refused_with_its_reason():
    W, U = torch.zeros(16, 128, dtype=torch.float16), torch.eye(128)
    with pytest.raises(NotImplementedError, match="Format A"):
        ops.gptq_quantize(W, U, 4, 128, perm=torch.arange(128))
    from amq_amd.patching import quantize_model_gptq
    with pytest.raises(NotImplementedError, match="Format A"):
        quantize_model_gptq(torch.nn.Linear(2, 2), 4, [], act_order=True)
