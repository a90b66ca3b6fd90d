"""CPU-only: what the nineteen decode-step entry points of the C ABI refuse, and with which return code -- the ten decode-attention functions
(amq_attn_decode{,_cur,_split,_seq,_rows}{,_qkn}_f16), the seven token tails and the two set_token functions.

One call per rule, breaking that rule alone in an otherwise acceptable call.  The table holds refused calls only: the pointers are made up, an
accepted call would launch.  The refusals tests/test_ragged_cpu.py, test_lookup_cpu.py, test_sampling_cpu.py and test_qknorm_cpu.py already hold
are not restated here.  DESIGN.md ("Decode-step entry points: what is checked") states the rules; the LDS boundaries follow from the
160 KiB limit: 6 * 128 + 4 * keys + 17 KiB (+ 2 * 7 * 128 * 2 + 16 bytes in the rows form) must fit."""
import ctypes

import pytest

from amq_amd import _lib

EINVAL, ESHAPE = -1, -2
one = ctypes.c_void_p(16)
f32 = ctypes.c_float

# ---------------------------------------------------------------------------------------------------------------- decode attention
# name -> (argument names in the order of include/amq_hip.h, an acceptable call); the _qkn twins take the same behind an amq_qk_norm*
_HEADS = dict(n_heads=8, n_kv_heads=2, head_dim=128)
_QKV = dict(q=one, k=one, v=one, kcache=one, vcache=one, out=one)
ATTN = {
    "amq_attn_decode_f16": ("q k v kcache vcache out pos_dev pos batch n_heads n_kv_heads head_dim max_seq rope_theta rope_table stream",
                            dict(_QKV, pos_dev=None, pos=5, batch=3, **_HEADS, max_seq=64, rope_theta=f32(10000.0), rope_table=None, stream=None)),
    "amq_attn_decode_cur_f16": ("q k v kcache vcache out step_state batch n_heads n_kv_heads head_dim max_seq stream",
                                dict(_QKV, step_state=one, batch=3, **_HEADS, max_seq=64, stream=None)),
    "amq_attn_decode_split_f16": ("q k v kcache vcache out step_state pos_dev pos batch n_heads n_kv_heads head_dim max_seq rope_theta rope_table "
                                  "n_splits workspace workspace_bytes tickets stream",
                                  dict(_QKV, step_state=None, pos_dev=None, pos=5, batch=3, **_HEADS, max_seq=2048, rope_theta=f32(10000.0),
                                       rope_table=None, n_splits=2, workspace=one, workspace_bytes=3 * 8 * 2 * 528, tickets=one, stream=None)),
    "amq_attn_decode_seq_f16": ("q k v kcache vcache out step_states batch n_heads n_kv_heads head_dim max_seq n_splits workspace workspace_bytes "
                                "tickets stream",
                                dict(_QKV, step_states=one, batch=3, **_HEADS, max_seq=2048, n_splits=2, workspace=one,
                                     workspace_bytes=3 * 8 * 2 * 528, tickets=one, stream=None)),
    "amq_attn_decode_rows_f16": ("q k v kcache vcache out step_states rows n_heads n_kv_heads head_dim max_seq n_splits workspace workspace_bytes "
                                 "tickets stream",
                                 dict(_QKV, step_states=one, rows=3, **_HEADS, max_seq=2048, n_splits=2, workspace=one,
                                      workspace_bytes=3 * 8 * 2 * 528, tickets=one, stream=None)),
}
_NO_SPLIT = dict(n_splits=0, workspace=None, workspace_bytes=0, tickets=None)
_HEAD_RULES = [("n_heads 256", dict(n_heads=256, n_kv_heads=2), ESHAPE), ("n_heads 0", dict(n_heads=0), ESHAPE),
               ("n_kv_heads 0", dict(n_kv_heads=0), ESHAPE), ("n_heads % n_kv_heads", dict(n_heads=8, n_kv_heads=3), ESHAPE),
               ("head_dim 64", dict(head_dim=64), ESHAPE), ("max_seq 0", dict(max_seq=0), ESHAPE)]
_OPTIONAL_SPLIT_RULES = [("n_splits -1", dict(n_splits=-1), EINVAL), ("n_splits 1025", dict(n_splits=1025), EINVAL),
                         ("splits without workspace", dict(workspace=None), EINVAL), ("splits without tickets", dict(tickets=None), EINVAL),
                         ("workspace one byte short", dict(workspace_bytes=3 * 8 * 2 * 528 - 1), EINVAL),
                         ("chunks of 36448 keys", dict(max_seq=72833), ESHAPE)]


def _nulls(*names):
    return [(f"{n} null", {n: None}, EINVAL) for n in names]


ATTN_REFUSED = {
    "amq_attn_decode_f16": _nulls(*_QKV) + [("batch 0", dict(batch=0), ESHAPE)] + _HEAD_RULES + [
        ("host pos = max_seq", dict(pos=64), ESHAPE), ("host pos -1", dict(pos=-1), ESHAPE),
        ("max_seq 36417", dict(max_seq=36417), ESHAPE)],
    "amq_attn_decode_cur_f16": _nulls(*_QKV, "step_state") + [("batch 0", dict(batch=0), ESHAPE)] + _HEAD_RULES + [
        ("max_seq 36417", dict(max_seq=36417), ESHAPE)],
    "amq_attn_decode_split_f16": _nulls(*_QKV, "workspace", "tickets") + [
        ("batch 0", dict(batch=0), ESHAPE), ("batch 65536", dict(batch=65536, workspace_bytes=65536 * 8 * 2 * 528), ESHAPE)] + _HEAD_RULES + [
        ("host pos = max_seq", dict(pos=2048), ESHAPE), ("host pos -1", dict(pos=-1), ESHAPE),
        ("n_splits -1", dict(n_splits=-1), EINVAL), ("n_splits 0", dict(n_splits=0), EINVAL), ("n_splits 1025", dict(n_splits=1025), EINVAL),
        ("workspace one byte short", dict(workspace_bytes=3 * 8 * 2 * 528 - 1), EINVAL),
        ("chunks of 36448 keys", dict(max_seq=72833), ESHAPE),
        ("chunks of 36448 keys, one block", dict(max_seq=72833, step_state=one), ESHAPE)],
    "amq_attn_decode_seq_f16": _nulls(*_QKV) + [
        ("batch 0", dict(batch=0), ESHAPE), ("batch 65536", dict(batch=65536, workspace_bytes=65536 * 8 * 2 * 528), ESHAPE),
        ("n_heads 256", dict(n_heads=256, n_kv_heads=2), ESHAPE), ("n_heads 0", dict(n_heads=0), ESHAPE),
        ("n_kv_heads 0", dict(n_kv_heads=0), ESHAPE), ("max_seq 0", dict(max_seq=0), ESHAPE),
        ("n_splits -1", dict(n_splits=-1), EINVAL), ("n_splits 1025", dict(n_splits=1025), EINVAL),
        ("splits without tickets", dict(tickets=None), EINVAL),
        ("one split without workspace", dict(n_splits=1, workspace=None), EINVAL),
        ("max_seq 36417", dict(_NO_SPLIT, max_seq=36417), ESHAPE), ("chunks of 36448 keys", dict(max_seq=72833), ESHAPE)],
    "amq_attn_decode_rows_f16": _nulls("k", "v", "kcache", "vcache", "out") + [
        ("n_heads 256", dict(n_heads=256, n_kv_heads=2), ESHAPE), ("n_heads 0", dict(n_heads=0), ESHAPE),
        ("n_kv_heads 0", dict(n_kv_heads=0), ESHAPE), ("n_splits 1025", dict(n_splits=1025), EINVAL),
        ("splits without tickets", dict(tickets=None), EINVAL),
        ("max_seq 35517", dict(_NO_SPLIT, max_seq=35517), ESHAPE), ("chunks of 35520 keys", dict(max_seq=70977), ESHAPE)],
}
# the twins: everything their base refuses (the refusals other files hold for the BASE are theirs only: here the twin's are stated), and the norm
_TWIN_ONLY = {
    "amq_attn_decode_seq_f16": _nulls("step_states") + [
        ("head_dim 64", dict(head_dim=64), ESHAPE), ("n_heads % n_kv_heads", dict(n_heads=8, n_kv_heads=3), ESHAPE),
        ("splits without workspace", dict(workspace=None), EINVAL), ("workspace one byte short", dict(workspace_bytes=3 * 8 * 2 * 528 - 1), EINVAL)],
    "amq_attn_decode_rows_f16": _nulls("q", "step_states") + [
        ("rows 1", dict(rows=1), ESHAPE), ("rows 9", dict(rows=9), ESHAPE), ("head_dim 64", dict(head_dim=64), ESHAPE),
        ("n_heads % n_kv_heads", dict(n_heads=8, n_kv_heads=3), ESHAPE), ("max_seq 0", dict(max_seq=0), ESHAPE),
        ("n_splits -1", dict(n_splits=-1), EINVAL), ("splits without workspace", dict(workspace=None), EINVAL),
        ("workspace one byte short", dict(workspace_bytes=3 * 8 * 2 * 528 - 1), EINVAL)],
}
NORM_REFUSED = [("q_gamma null", (None, 16, 1e-6)), ("k_gamma null", (16, None, 1e-6)), ("eps negative", (16, 16, -1e-6)), ("eps nan", (16, 16, float("nan")))]

# ---------------------------------------------------------------------------------------------------------------- token tails and set_token
_TAIL = dict(logits=one, vocab=1024, embed=one, hidden=256, token=one, pos=one, x=one, rope_table=one, rope_cur=one, rope_rows=64)
_TAIL_SEQ = dict(logits=one, vocab=1024, embed=one, hidden=256, token=one, step_states=one, x=one, rope_table=one, rope_rows=64)
TAIL = {
    "amq_decode_tail_f16": ("logits vocab embed hidden token pos x rope_table rope_cur rope_rows stream", dict(_TAIL, stream=None)),
    "amq_decode_tail_batch_f16": ("logits vocab embed hidden token pos x rope_table rope_cur rope_rows batch stream", dict(_TAIL, batch=3, stream=None)),
    "amq_decode_tail_suppress_f16": ("logits vocab embed hidden token pos x rope_table rope_cur rope_rows batch suppress_ids stream",
                                     dict(_TAIL, batch=3, suppress_ids=one, stream=None)),
    "amq_decode_tail_sample_f16": ("logits vocab embed hidden token pos x rope_table rope_cur rope_rows batch suppress_ids state stream",
                                   dict(_TAIL, batch=3, suppress_ids=None, state=one, stream=None)),
    "amq_set_token_f16": ("token_in n_in embed vocab hidden token pos x rope_table rope_cur rope_rows batch stream",
                          dict(_TAIL, token_in=one, n_in=3, batch=3, stream=None)),
    "amq_decode_tail_seq_f16": ("logits vocab embed hidden token step_states x rope_table rope_rows batch suppress_ids stream",
                                dict(_TAIL_SEQ, batch=3, suppress_ids=None, stream=None)),
    "amq_decode_tail_sample_seq_f16": ("logits vocab embed hidden token step_states x rope_table rope_rows batch suppress_ids state stream",
                                       dict(_TAIL_SEQ, batch=3, suppress_ids=None, state=one, stream=None)),
    "amq_set_token_seq_f16": ("token_in n_in embed vocab hidden token step_states x rope_table rope_rows batch stream",
                              dict(_TAIL_SEQ, token_in=one, n_in=3, batch=3, stream=None)),
    "amq_decode_tail_lookup_f16": ("logits vocab embed hidden token step_states x rope_table rope_rows rows suppress_ids lookup_state history "
                                   "history_cap stream",
                                   dict(_TAIL_SEQ, rows=3, suppress_ids=None, lookup_state=one, history=one, history_cap=64, stream=None)),
}
_PAIRING = [("rope_table without rope_cur", dict(rope_cur=None), EINVAL), ("rope_cur without rope_table", dict(rope_table=None), EINVAL),
            ("rope_rows 0", dict(rope_rows=0), EINVAL)]
_SIZES = [("vocab 0", dict(vocab=0), ESHAPE), ("hidden 12", dict(hidden=12), ESHAPE), ("hidden 0", dict(hidden=0), ESHAPE)]
_BATCH = [("batch 0", dict(batch=0), ESHAPE), ("batch 65536", dict(batch=65536), ESHAPE)]
TAIL_REFUSED = {
    "amq_decode_tail_f16": _nulls("logits", "embed", "token", "pos", "x") + _PAIRING + _SIZES,
    "amq_decode_tail_batch_f16": _nulls("logits", "embed", "token", "pos", "x") + _PAIRING + _SIZES + _BATCH + [
        ("vocab % 8 with 2 rows", dict(vocab=1001, batch=2), ESHAPE)],
    "amq_decode_tail_suppress_f16": _nulls("logits", "embed", "token", "pos", "x", "suppress_ids") + _PAIRING + _SIZES + _BATCH + [
        ("vocab % 8 with 2 rows", dict(vocab=1001, batch=2), ESHAPE)],
    # (the sampled tail answers vocab 0 and batch 0 with AMQ_EINVAL: tests/test_sampling_cpu.py; its per-sequence form with AMQ_ESHAPE, below)
    "amq_decode_tail_sample_f16": _nulls("logits", "embed", "token", "pos", "x") + _PAIRING + [
        ("hidden 12", dict(hidden=12), ESHAPE), ("hidden 0", dict(hidden=0), ESHAPE)],
    "amq_set_token_f16": _nulls("token_in", "embed", "token", "pos", "x") + _PAIRING + _SIZES + _BATCH + [
        ("n_in neither 1 nor batch", dict(n_in=2), ESHAPE), ("n_in 0", dict(n_in=0), ESHAPE)],
    "amq_decode_tail_seq_f16": _nulls("logits", "embed", "token", "x") + [("rope_rows 0", dict(rope_rows=0), EINVAL)] + _SIZES + _BATCH,
    "amq_decode_tail_sample_seq_f16": _nulls("logits", "embed", "token", "step_states", "x", "rope_table") + [
        ("rope_rows 0", dict(rope_rows=0), EINVAL)] + _SIZES + [("batch 0", dict(batch=0), ESHAPE)],
    "amq_set_token_seq_f16": _nulls("embed", "token", "step_states", "x", "rope_table") + [("rope_rows 0", dict(rope_rows=0), EINVAL)] + _SIZES + _BATCH + [
        ("n_in 0", dict(n_in=0), ESHAPE)],
    "amq_decode_tail_lookup_f16": _nulls("embed", "token", "step_states", "x", "rope_table") + [
        ("vocab 0", dict(vocab=0), ESHAPE), ("hidden 0", dict(hidden=0), ESHAPE),
        ("history_cap above 2^24", dict(history_cap=(1 << 24) + 1), ESHAPE)],
}


def _run(name, names, good, refused, lead=()):
    fn = getattr(_lib.load(), name)
    wrong = []
    for label, change, code in refused:
        unknown = set(change) - set(good)
        assert not unknown, (name, label, unknown)
        args = dict(good, **change)
        rc = fn(*lead, *(args[n] for n in names.split()))
        assert rc != 0, f"{name} / {label}: ACCEPTED a call the table holds as refused"
        if rc != code:
            wrong.append((label, code, rc, _lib.load().amq_last_error().decode()))
    assert not wrong, f"{name}: (rule, expected, got, message) {wrong}"


def test_the_table_covers_the_nineteen_entry_points():
    names = list(ATTN) + [n[:-len("_f16")] + "_qkn_f16" for n in ATTN] + list(TAIL)
    assert len(names) == len(set(names)) == 19
    assert set(ATTN) == set(ATTN_REFUSED) and set(TAIL) == set(TAIL_REFUSED)
    for n in names:
        assert n in _lib.SIGNATURES


@pytest.mark.parametrize("name", list(ATTN))
def test_decode_attention_refusals(name):
    names, good = ATTN[name]
    _run(name, names, good, ATTN_REFUSED[name])


@pytest.mark.parametrize("name", list(ATTN))
def test_decode_attention_qkn_refusals(name):
    names, good = ATTN[name]
    twin = name[:-len("_f16")] + "_qkn_f16"
    norm = _lib.QkNorm(16, 16, 1e-6)
    _run(twin, names, good, ATTN_REFUSED[name] + _TWIN_ONLY.get(name, []), lead=(ctypes.byref(norm),))
    # ... and under a NULL norm (the twin is then its base)
    _run(twin, names, good, ATTN_REFUSED[name] + _TWIN_ONLY.get(name, []), lead=(None,))
    fn = getattr(_lib.load(), twin)
    for label, fields in NORM_REFUSED:
        bad = _lib.QkNorm(*fields)
        assert fn(ctypes.byref(bad), *(good[n] for n in names.split())) == EINVAL, (twin, label)
        # the norm is looked at first: the same answer in front of a shape error
        assert fn(ctypes.byref(bad), *(dict(good, head_dim=64)[n] for n in names.split())) == EINVAL, (twin, label)


@pytest.mark.parametrize("name", list(TAIL))
def test_token_tail_refusals(name):
    names, good = TAIL[name]
    _run(name, names, good, TAIL_REFUSED[name])
