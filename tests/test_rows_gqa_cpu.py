"""CPU-only: the grouped rows attention (amq_attn_decode_rows_gqa_f16 and its _qkn twin) refuses what include/amq_hip.h says it refuses, one call per
rule and before any HIP call (every pointer is fake: an accepted call would launch), and QuantLlama.rows_attention_grouped decides what its class
constant says."""
import ctypes
import math

import pytest

from amq_amd import _lib

EINVAL, ESHAPE = -1, -2
NAMES = ("amq_attn_decode_rows_gqa_f16", "amq_attn_decode_rows_gqa_qkn_f16")
ARGS = "q k v kcache vcache out step_states rows n_heads n_kv_heads head_dim max_seq n_splits workspace workspace_bytes tickets stream".split()
ONE = ctypes.c_void_p(256)


def _good():
    wsb = _lib.load().amq_attn_decode_split_workspace_bytes(4, 32, 8)
    assert wsb == 4 * 32 * 8 * 132 * 4
    good = dict.fromkeys(ARGS[:7], ONE)
    good.update(rows=4, n_heads=32, n_kv_heads=8, head_dim=128, max_seq=2048, n_splits=8, workspace=ONE, workspace_bytes=wsb, tickets=ONE, stream=None)
    return good


# (what changes, return code, a word of the message) in the validator's order
REFUSED = [(dict([(n, None)]), EINVAL, b"null") for n in ARGS[:7]] + [
    (dict(workspace=None), EINVAL, b"null"),
    (dict(tickets=None), EINVAL, b"null"),
    (dict(head_dim=64), ESHAPE, b"head_dim"),
    (dict(rows=1), ESHAPE, b"rows"), (dict(rows=9), ESHAPE, b"rows"), (dict(rows=0), ESHAPE, b"rows"),
    (dict(n_heads=0), ESHAPE, b"head configuration"), (dict(n_kv_heads=5), ESHAPE, b"head configuration"), (dict(n_heads=256, n_kv_heads=16), ESHAPE, b"head configuration"),
    (dict(n_kv_heads=32), ESHAPE, b"2..16"),                    # multi-head: the per-head kernels' model
    (dict(n_heads=34, n_kv_heads=1), ESHAPE, b"2..16"),        # 34 query heads per kv head
    (dict(max_seq=0), ESHAPE, b"max_seq"),
    (dict(max_seq=(1 << 24) + 1), ESHAPE, b"2^24"),
    (dict(n_splits=0), EINVAL, b"n_splits"), (dict(n_splits=-1), EINVAL, b"n_splits"), (dict(n_splits=1025), EINVAL, b"n_splits"),
    (dict(workspace_bytes=4 * 32 * 8 * 132 * 4 - 1), EINVAL, b"workspace too small"),
    (dict(rows=8), EINVAL, b"workspace too small"),             # the workspace of 4 rows under 8
]


def test_symbols_bound_and_version_unchanged():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES[NAMES[0]] == _lib.SIGNATURES["amq_attn_decode_rows_f16"]
    assert _lib.SIGNATURES[NAMES[1]] == _lib.SIGNATURES["amq_attn_decode_rows_qkn_f16"]
    assert lib.amq_version() == 521


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("change,code,word", REFUSED, ids=[",".join(f"{k}={getattr(v, 'value', v)}" for k, v in c.items()) for c, _, _ in REFUSED])
def test_refused(name, change, code, word):
    lib = _lib.load()
    norm = _lib.QkNorm(16, 16, 1e-6)
    lead = (ctypes.byref(norm),) if name.endswith("_qkn_f16") else ()
    call = dict(_good(), **change)
    assert getattr(lib, name)(*lead, *(call[a] for a in ARGS)) == code
    assert word in lib.amq_last_error(), lib.amq_last_error()


def test_checks_run_in_the_validator_order():
    lib = _lib.load()
    f = lib.amq_attn_decode_rows_gqa_f16
    call = lambda **ch: f(*(dict(_good(), **ch)[a] for a in ARGS))
    assert call(q=None, head_dim=64) == EINVAL                                   # pointers first
    assert call(head_dim=64, rows=9) == ESHAPE and b"head_dim" in lib.amq_last_error()
    assert call(rows=9, n_kv_heads=32) == ESHAPE and b"rows" in lib.amq_last_error()
    assert call(n_kv_heads=32, n_splits=0) == ESHAPE and b"2..16" in lib.amq_last_error()     # the group in front of n_splits
    assert call(n_splits=0, workspace_bytes=0) == EINVAL and b"n_splits" in lib.amq_last_error()
    # a long cache in one chunk is this kernel's to take (the per-head forms refuse it for their score array): only the workspace is missing here
    assert call(max_seq=1 << 20, n_splits=1, workspace_bytes=0) == EINVAL and b"workspace too small" in lib.amq_last_error()


def test_the_twin_norm_rules():
    lib = _lib.load()
    f = lib.amq_attn_decode_rows_gqa_qkn_f16
    good = _good()
    rest = [good[a] for a in ARGS]
    for norm, word in ((_lib.QkNorm(None, 16, 1e-6), b"go together"), (_lib.QkNorm(16, None, 1e-6), b"go together"), (_lib.QkNorm(16, 16, -1.0), b"eps"),
                       (_lib.QkNorm(16, 16, math.nan), b"eps")):
        assert f(ctypes.byref(norm), *rest) == EINVAL and word in lib.amq_last_error()
        # the norm is looked at first: the same answer in front of a shape error
        assert f(ctypes.byref(norm), *(dict(good, head_dim=64)[a] for a in ARGS)) == EINVAL and word in lib.amq_last_error()
    # a NULL norm: the twin is its base
    for change, code, word in REFUSED:
        assert f(None, *(dict(good, **change)[a] for a in ARGS)) == code and word in lib.amq_last_error()


def test_ops_refuses_a_group_outside_2_16():
    torch = pytest.importorskip("torch")
    from amq_amd import ops
    t = torch.zeros(1, dtype=torch.float16)
    for nh, nkv in ((32, 32), (34, 1), (32, 5), (4, 0)):
        with pytest.raises(ValueError, match="2..16 query heads"):
            ops.attn_decode_rows(t, t, t, t, t, t, None, None, nh, nkv, grouped=True)
    assert ops.attn_rows_gqa_blocks(2, 4, 2) == 1 and ops.attn_rows_gqa_blocks(8, 32, 8) == 2 and ops.attn_rows_gqa_blocks(8, 28, 4) == 4
    assert ops.attn_rows_gqa_blocks(8, 16, 1) == 8 and ops.attn_rows_gqa_blocks(5, 6, 3) == 1 and ops.attn_rows_gqa_blocks(3, 28, 4) == 2


@pytest.mark.parametrize("nh,nkv,grouped_model", [(32, 32, False), (32, 8, True), (28, 4, True), (34, 2, False)])
def test_rows_attention_grouped(nh, nkv, grouped_model, monkeypatch):
    from amq_amd.llama import QuantLlama
    f = QuantLlama.rows_attention_grouped
    frm = QuantLlama.ROWS_GQA_FROM
    assert frm is None or frm >= 2048                           # (not below 2048 in this change: shorter caches keep their arithmetic)
    for max_seq in (1024, 2048, 8192):
        assert f(nh, nkv, max_seq) is (grouped_model and frm is not None and max_seq >= frm)
    monkeypatch.setattr(QuantLlama, "ROWS_GQA_FROM", 2048)
    assert [f(nh, nkv, s) for s in (1024, 2048, 8192)] == [False, grouped_model, grouped_model]
    monkeypatch.setattr(QuantLlama, "ROWS_GQA_FROM", 4096)
    assert [f(nh, nkv, s) for s in (1024, 2048, 8192)] == [False, False, grouped_model]
    monkeypatch.setattr(QuantLlama, "ROWS_GQA_FROM", None)
    assert [f(nh, nkv, s) for s in (1024, 2048, 8192)] == [False, False, False]
