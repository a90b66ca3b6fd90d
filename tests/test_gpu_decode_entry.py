"""GPU: which C entry point every decode-step ops call reaches, and with which arguments -- the dispatch of ops.attn_decode, attn_decode_rows,
decode_tail, decode_tail_sample, set_token and decode_tail_lookup ("Decode-step entry points").

``_lib.load`` is replaced by a pass-through proxy that records, per C call of the nineteen decode-step entry points, the name and every argument:
integers and floats by value, pointers as ``None`` / ``"ptr"`` or -- where they are the address of a tensor of the call -- that tensor's name; the
amq_qk_norm of a ``_qkn`` call as ("qkn", q_gamma, k_gamma, eps).  The calls run for real: after each, the stream synchronises and the outputs are
finite.  EXPECTED holds what this recorder gives for the ops.py of the commit before the entry points shared one validator and one dispatcher
per family; the records of a call with q/k norms are those of the call without, under the ``_qkn`` name and behind the norm (so on that commit
too)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NH, NKV, HID, VOCAB, R = 2, 1, 256, 1024, 3
EPS = ctypes.c_float(1e-6).value
ENTRY = tuple("amq_attn_decode%s%s_f16" % (form, qkn) for form in ("", "_cur", "_split", "_seq", "_rows") for qkn in ("", "_qkn")) + (
    "amq_decode_tail_f16", "amq_decode_tail_batch_f16", "amq_decode_tail_suppress_f16", "amq_decode_tail_sample_f16", "amq_decode_tail_seq_f16",
    "amq_decode_tail_sample_seq_f16", "amq_decode_tail_lookup_f16", "amq_set_token_f16", "amq_set_token_seq_f16")


class _Recorder:
    """stands for the loaded library: every attribute is the library's; the decode-step entry points also leave a record"""

    def __init__(self, lib, tensors):
        self._lib, self._names, self.calls = lib, {t.data_ptr(): n for n, t in tensors.items()}, []

    def _show(self, a):
        if a is None or isinstance(a, int):
            return a
        if isinstance(a, ctypes.c_float):
            return a.value
        if isinstance(a, ctypes.c_void_p):
            return None if a.value is None else self._names.get(a.value, "ptr")
        norm = a._obj                                   # ctypes.byref(QkNorm)
        return ("qkn", self._names.get(norm.q_gamma, "ptr"), self._names.get(norm.k_gamma, "ptr"), norm.eps)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ENTRY:
            return fn

        def call(*args):
            self.calls.append((name,) + tuple(self._show(a) for a in args))
            return fn(*args)
        return call


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _attn_tensors(B, rows, max_seq, seed):
    """q / k / v / out of ``rows`` rows, finite caches of B sequences, the cos/sin table, q/k norm weights -- seeded on the CPU"""
    g = _gen(seed)
    mk = lambda *shape: torch.randn(*shape, generator=g).half().to(DEV)
    t = dict(q=mk(rows, NH * 128), k=mk(rows, NKV * 128), v=mk(rows, NKV * 128), kcache=mk(B, NKV, max_seq, 128), vcache=mk(B, NKV, max_seq, 128))
    t["out"] = torch.zeros(rows, NH * 128, dtype=torch.float16, device=DEV)
    t["q_norm"], t["k_norm"] = (1.0 + 0.1 * mk(128)).contiguous(), (1.0 + 0.1 * mk(128)).contiguous()
    return t


def _state(ops, table, positions=None, pos=None):
    """a step state at ``pos`` (one block) or at ``positions`` (one block each) with the cos/sin rows of ``table`` [rows, 128]"""
    if positions is None:
        cur, p, err = ops.new_step_state(torch.device(DEV))
        p.fill_(pos)
        cur.copy_(table[pos])
    else:
        cur, p, err = ops.new_step_state(torch.device(DEV), batch=len(positions))
        p.copy_(torch.tensor(positions, dtype=torch.int32))
        cur.copy_(table[torch.tensor(positions, device=DEV)])
    return cur, p, err


def _attn_case(form, B, max_seq, n_splits=0):
    """-> (call(ops, norms), tensors by name, outputs) of one ops.attn_decode / attn_decode_rows call"""
    from amq_amd import ops
    rows = R if form == "rows" else B
    t = _attn_tensors(1 if form == "rows" else B, rows, max_seq, 100 * max_seq + 10 * B + len(form))
    table = ops.rope_table(max_seq, 10000.0, torch.device(DEV))
    p0 = max_seq - 60
    kw = dict(n_splits=n_splits)
    if form == "seq":
        t["cur"], t["pos"], err = _state(ops, table.view(max_seq, 128), positions=[p0, 2, max_seq // 2][:B])
    elif form == "rows":
        t["cur"], t["pos"], err = _state(ops, table.view(max_seq, 128), positions=[p0 + j for j in range(R)])
    elif form == "cur":
        t["cur"], t["pos"], err = _state(ops, table.view(max_seq, 128), pos=p0)
    elif form == "pos_dev":
        t["pos"], t["table"], err = torch.full((1,), p0, dtype=torch.int32, device=DEV), table, None
    else:
        assert form == "host"
        err = None
    pos = t["pos"] if "pos" in t else p0

    def call(norms):
        nk = dict(q_norm=t["q_norm"], k_norm=t["k_norm"], norm_eps=1e-6) if norms else {}
        if form == "rows":
            ops.attn_decode_rows(t["q"], t["k"], t["v"], t["kcache"], t["vcache"], t["out"], t["cur"], pos, NH, NKV, **kw, **nk)
        else:
            ops.attn_decode(t["q"], t["k"], t["v"], t["kcache"], t["vcache"], t["out"], pos, NH, NKV, rope_theta=10000.0, table=t.get("table"),
                            cur=t.get("cur"), **kw, **nk)
        torch.cuda.synchronize()
        assert err is None or err.tolist() == [0] * err.numel()
    return call, t, [t["out"], t["kcache"], t["vcache"]]


def _tail_case(kind, B, seq, suppress=False, bare=False):
    """-> the same for one call of the tail family over B rows (``kind``: tail / sample / set_token / lookup)"""
    from amq_amd import ops
    g = _gen(7 * B + len(kind) + 2 * seq + suppress)
    t = dict(logits=torch.randn(B, VOCAB, generator=g).half().to(DEV), embed=torch.randn(VOCAB, HID, generator=g).half().to(DEV),
             token=torch.zeros(B, dtype=torch.int64, device=DEV), x=torch.zeros(B, HID, dtype=torch.float16, device=DEV))
    table = ops.rope_table(64, 10000.0, torch.device(DEV))
    if kind == "lookup":
        t["cur"], t["pos"], err = _state(ops, table.view(64, 128), positions=[9 + j for j in range(B)])
        t["state"], t["history"] = ops.new_lookup_state(torch.device(DEV), B - 1, 2, 64)
        t["history"][:10].copy_(torch.arange(10, dtype=torch.int32))
        t["state"][ops.LOOKUP_COUNT] = 10
    elif seq:
        t["cur"], t["pos"], err = _state(ops, table.view(64, 128), positions=[5, 2, 40][:B])
    elif bare:
        t["pos"], err = torch.full((1,), 5, dtype=torch.int32, device=DEV), None
    else:
        t["cur"], t["pos"], err = _state(ops, table.view(64, 128), pos=5)
    if not bare:
        t["table"] = table
    if suppress:
        t["suppress"] = torch.tensor([3, 7] + [-1] * 6, dtype=torch.int32, device=DEV)
    if kind == "sample":
        t["state"] = ops.new_sampling_state(torch.device(DEV))
        ops.set_sampling_state(t["state"], top_k=4, seed=3)
    if kind == "set_token":
        t["token_in"] = torch.tensor([11, 1023, 0][:B], dtype=torch.int64, device=DEV)

    def call(norms):
        assert not norms
        if kind == "tail":
            ops.decode_tail(t["logits"], t["embed"], t["token"], t["pos"], t["x"], table=t.get("table"), cur=t.get("cur"), suppress=t.get("suppress"))
        elif kind == "sample":
            ops.decode_tail_sample(t["logits"], t["embed"], t["token"], t["pos"], t["x"], t["state"], table=t.get("table"), cur=t.get("cur"),
                                   suppress=t.get("suppress"))
        elif kind == "set_token":
            ops.set_token(t["token_in"], t["embed"], t["token"], t["pos"], t["x"], table=t.get("table"), cur=t.get("cur"))
        else:
            ops.decode_tail_lookup(t["logits"], t["embed"], t["token"], t["pos"], t["x"], t["state"], t["history"], t["table"], t["cur"],
                                   suppress=t.get("suppress"))
        torch.cuda.synchronize()
        assert err is None or err.tolist() == [0] * err.numel()
        assert bool(((t["token"] >= 0) & (t["token"] < VOCAB)).all())
    return call, t, [t["x"]] + ([t["cur"]] if "cur" in t else [])


CASES = {      # name -> (builder, its arguments, takes q/k norms)
    "attn seq B1 64": (_attn_case, ("seq", 1, 64), True),
    "attn seq B3 64": (_attn_case, ("seq", 3, 64), True),
    "attn seq B3 768 policy": (_attn_case, ("seq", 3, 768), True),
    "attn seq B1 768 four splits": (_attn_case, ("seq", 1, 768, 4), True),
    "attn split block B1 768 policy": (_attn_case, ("cur", 1, 768), True),
    "attn split pos_dev B3 768 policy": (_attn_case, ("pos_dev", 3, 768), True),
    "attn split host B1 768 two splits": (_attn_case, ("host", 1, 768, 2), True),
    "attn cur B1 64": (_attn_case, ("cur", 1, 64), True),
    "attn cur B3 64": (_attn_case, ("cur", 3, 64), True),
    "attn host B3 64": (_attn_case, ("host", 3, 64), True),
    "attn pos_dev B1 64": (_attn_case, ("pos_dev", 1, 64), True),
    "attn cur B1 768 one split": (_attn_case, ("cur", 1, 768, 1), True),
    "rows 64": (_attn_case, ("rows", 1, 64), True),
    "rows 768 policy": (_attn_case, ("rows", 1, 768), True),
    "tail seq B3": (_tail_case, ("tail", 3, True), False),
    "tail seq B1 suppress": (_tail_case, ("tail", 1, True, True), False),
    "tail suppress B3": (_tail_case, ("tail", 3, False, True), False),
    "tail suppress B1": (_tail_case, ("tail", 1, False, True), False),
    "tail B1": (_tail_case, ("tail", 1, False), False),
    "tail B1 no table": (_tail_case, ("tail", 1, False, False, True), False),
    "tail B3": (_tail_case, ("tail", 3, False), False),
    "sample seq B3": (_tail_case, ("sample", 3, True), False),
    "sample B1": (_tail_case, ("sample", 1, False), False),
    "sample B3 suppress no table": (_tail_case, ("sample", 3, False, True, True), False),
    "set_token seq B3": (_tail_case, ("set_token", 3, True), False),
    "set_token B3": (_tail_case, ("set_token", 3, False), False),
    "set_token B1 no table": (_tail_case, ("set_token", 1, False, False, True), False),
    "lookup R3": (_tail_case, ("lookup", R, True), False),
}


def record(name, norms, monkeypatch):
    """run case ``name`` once under the recorder -> its records"""
    from amq_amd import _lib
    builder, args, _ = CASES[name]
    call, tensors, outputs = builder(*args)
    rec = _Recorder(_lib.load(), tensors)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    call(norms)
    monkeypatch.undo()
    for o in outputs:
        assert bool(torch.isfinite(o.float()).all()), name
    return rec.calls


def with_norm(calls):
    """the records of the same calls given q/k norms: the `_qkn` twin, the same arguments behind the norm"""
    return [(c[0][:-len("_f16")] + "_qkn_f16", ("qkn", "q_norm", "k_norm", EPS)) + c[1:] for c in calls]


def _attn(form, *args):
    return [("amq_attn_decode%s_f16" % form, "q", "k", "v", "kcache", "vcache", "out") + args + (None,)]      # (the stream: the null stream)


def _tail(name, *args):
    return [("amq_decode_tail%s_f16" % name, "logits", VOCAB, "embed", HID, "token") + args + (None,)]


def _set_token(seq, n_in, *args):
    return [("amq_set_token%s_f16" % seq, "token_in", n_in, "embed", VOCAB, HID, "token") + args + (None,)]


_WS = 132 * 4       # workspace bytes per (row, head, split)
EXPECTED = {
    "attn seq B1 64": _attn("_seq", "cur", 1, NH, NKV, 128, 64, 0, None, 0, None),
    "attn seq B3 64": _attn("_seq", "cur", 3, NH, NKV, 128, 64, 0, None, 0, None),
    # (two query heads per kv head: the policy of the grouped-query kernel, 128-key chunks -> 6)
    "attn seq B3 768 policy": _attn("_seq", "cur", 3, NH, NKV, 128, 768, 6, "ptr", 3 * NH * 6 * _WS, "ptr"),
    "attn seq B1 768 four splits": _attn("_seq", "cur", 1, NH, NKV, 128, 768, 4, "ptr", 1 * NH * 4 * _WS, "ptr"),
    "attn split block B1 768 policy": _attn("_split", "cur", "pos", 0, 1, NH, NKV, 128, 768, 10000.0, None, 6, "ptr", 1 * NH * 6 * _WS, "ptr"),
    "attn split pos_dev B3 768 policy": _attn("_split", None, "pos", 0, 3, NH, NKV, 128, 768, 10000.0, "table", 6, "ptr", 3 * NH * 6 * _WS, "ptr"),
    "attn split host B1 768 two splits": _attn("_split", None, None, 708, 1, NH, NKV, 128, 768, 10000.0, None, 2, "ptr", 1 * NH * 2 * _WS, "ptr"),
    "attn cur B1 64": _attn("_cur", "cur", 1, NH, NKV, 128, 64),
    "attn cur B3 64": _attn("_cur", "cur", 3, NH, NKV, 128, 64),
    "attn host B3 64": _attn("", None, 4, 3, NH, NKV, 128, 64, 10000.0, None),
    "attn pos_dev B1 64": _attn("", "pos", 0, 1, NH, NKV, 128, 64, 10000.0, "table"),
    "attn cur B1 768 one split": _attn("_cur", "cur", 1, NH, NKV, 128, 768),
    "rows 64": _attn("_rows", "cur", R, NH, NKV, 128, 64, 0, None, 0, None),
    # (the per-head policy, without n_kv_heads: 768 / 272 keys -> 3)
    "rows 768 policy": _attn("_rows", "cur", R, NH, NKV, 128, 768, 3, "ptr", R * NH * 3 * _WS, "ptr"),
    "tail seq B3": _tail("_seq", "cur", "x", "table", 64, 3, None),
    "tail seq B1 suppress": _tail("_seq", "cur", "x", "table", 64, 1, "suppress"),
    "tail suppress B3": _tail("_suppress", "pos", "x", "table", "cur", 64, 3, "suppress"),
    "tail suppress B1": _tail("_suppress", "pos", "x", "table", "cur", 64, 1, "suppress"),
    "tail B1": _tail("", "pos", "x", "table", "cur", 64),
    "tail B1 no table": _tail("", "pos", "x", None, None, 0),
    "tail B3": _tail("_batch", "pos", "x", "table", "cur", 64, 3),
    "sample seq B3": _tail("_sample_seq", "cur", "x", "table", 64, 3, None, "state"),
    "sample B1": _tail("_sample", "pos", "x", "table", "cur", 64, 1, None, "state"),
    "sample B3 suppress no table": _tail("_sample", "pos", "x", None, None, 0, 3, "suppress", "state"),
    "set_token seq B3": _set_token("_seq", 3, "cur", "x", "table", 64, 3),
    "set_token B3": _set_token("", 3, "pos", "x", "table", "cur", 64, 3),
    "set_token B1 no table": _set_token("", 1, "pos", "x", None, None, 0, 1),
    "lookup R3": _tail("_lookup", "cur", "x", "table", 64, R, None, "state", "history", 64),
}


@pytest.mark.parametrize("name,norms", [(n, False) for n in CASES] + [(n, True) for n in CASES if CASES[n][2]])
def test_entry_point_and_arguments_of_each_dispatch_row(name, norms, monkeypatch):
    calls = record(name, norms, monkeypatch)
    print(name, norms, calls)
    assert calls == (with_norm(EXPECTED[name]) if norms else EXPECTED[name])
