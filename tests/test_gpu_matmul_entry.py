"""GPU: which C entry point every fp16 matmul ops call reaches, and with which arguments -- the dispatch of ops.gemv, gemv_grouped,
gemv_grouped_sums, gemm, gemm_res_norm_xfrag, gemm_f16w, gemm_xfrag, gemm_xfrag_grouped and linear ("Matmul entry points: what is
checked").

``_lib.load`` is replaced by a pass-through proxy (the pattern of tests/test_gpu_decode_entry.py) that records, per C call of the matmul entry
points, the name and every argument: integers and floats by value, pointers as ``None`` / ``"ptr"`` or -- where they are the address of a tensor
of the call -- that tensor's name; an amq_segment array as one ("seg", qweight, meta, bias, residual, y, N, bits, mode, y_stride) per segment,
the amq_gemv_opts as ("opts", math, waves, depth, rpt, dot, act_mask).  The calls run for real: after each, the stream synchronises and the
outputs are finite.  EXPECTED holds what this recorder gives for the ops.py of the commit before the entry points shared their validators.

Shapes are the smallest each path accepts: N = K = 256 where nothing forces more; K = 2048 and two rows for the partial-sum form; 40 and 300
rows for the GEMM; (65, 16, 512) -- by the host query the smallest (M, N, K) with split-K partials -- and its N = 128 twin where the rows are
handed on in fragment order."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, K = 256, 256
SK = (65, 16, 512)          # split-K: see test_the_split_k_shape_is_the_smallest
EPS = ctypes.c_float(1e-6).value
ENTRY = ("amq_gemv_f16", "amq_gemv_grouped_f16", "amq_gemv_grouped_sums_f16", "amq_gemm_f16", "amq_gemm_splitk_f16", "amq_gemm_route_f16",
         "amq_gemm_res_f16", "amq_gemm_res_norm_xfrag_f16", "amq_gemm_gated_f16", "amq_gemm_f16w_f16", "amq_gemm_xfrag_f16",
         "amq_gemm_xfrag_grouped_f16", "amq_gemm_xfrag_grouped_form_f16", "amq_linear_f16", "amq_silu_mul_f16")


class _Recorder:
    """stands for the loaded library: every attribute is the library's; the matmul entry points also leave a record"""

    def __init__(self, lib, tensors):
        self._lib, self._names, self.calls = lib, {t.data_ptr(): n for n, t in tensors.items()}, []

    def _ptr(self, v):
        return None if v is None else self._names.get(v, "ptr")

    def _show(self, a):
        if a is None or isinstance(a, (int, float)):
            return a
        if isinstance(a, ctypes.c_float):
            return a.value
        if isinstance(a, ctypes.c_void_p):
            return self._ptr(a.value)
        if isinstance(a, ctypes.Array):                 # amq_segment[]
            return tuple(("seg", self._ptr(s.qweight_native), self._ptr(s.meta_native), self._ptr(s.bias), self._ptr(s.residual), self._ptr(s.y),
                          s.N, s.bits, s.mode, s.y_stride) for s in a)
        o = a._obj                                      # ctypes.byref(GemvOpts)
        return ("opts", o.math, o.waves, o.depth, o.rpt, o.dot, o.act_mask)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ENTRY:
            return fn

        def call(*args):
            self.calls.append((name,) + tuple(self._show(a) for a in args))
            return fn(*args)
        return call


def _half(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).half().to(DEV)


def _layer(t, tag, n, k, bits, group=128):
    """a packed layer of random HQQ weights under the names qn<tag> / mn<tag>"""
    from amq_amd import ops
    from amq_amd.hqq_format import random_hqq
    h = random_hqq(n, k, bits, seed=10 * bits + n % 7, group=group).to(DEV)
    t["qn" + tag], t["mn" + tag] = ops.repack_from_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, n, k, group=group)
    return t["qn" + tag], t["mn" + tag]


def _zeros(m, n):
    return torch.zeros(m, n, dtype=torch.float16, device=DEV)


def _gemv_case(m, group=128, bias=False, out=False, opts=None):
    from amq_amd import ops
    t = dict(x=_half(1, m, K))
    qn, mn = _layer(t, "", N, K, 3, group)
    if bias:
        t["bias"] = _half(2, N)
    if out:
        t["y"] = _zeros(m, N)
    res = []

    def call():
        res.append(ops.gemv(t["x"], qn, mn, 3, ops.MODE_HQQ, N, K, bias=t.get("bias"), out=t.get("y"), opts=None if opts is None else ops.GemvOpts(**opts)))
    return call, t, res


def _grouped_case(m, pro="none", nseg=2, act=False, x_activated=False, residual=False, bias=False, group=128, opts=None):
    from amq_amd import ops
    t = dict(x=_half(3, m, K))
    segments = []
    for i in range(nseg):
        qn, mn = _layer(t, str(i), N, K, 2 + i % 3, group)
        t["y%d" % i] = _zeros(m, N)
        s = dict(qn=qn, mn=mn, bits=2 + i % 3, mode=ops.MODE_HQQ, N=N, y=t["y%d" % i])
        if bias and i == 0:
            s["bias"] = t["bias0"] = _half(4, N)
        if residual and i == nseg - 1:
            s["residual"] = t["res%d" % i] = _half(5, m, N)
        if act and i == 0:
            s["act"] = True
        segments.append(s)
    kw = {}
    if pro == "rmsnorm":
        t["gamma"] = 1.0 + 0.1 * _half(6, K)
        kw = dict(prologue=ops.PRO_RMSNORM, gamma=t["gamma"], eps=1e-6)
    elif pro == "silu_mul":
        t["x2"] = _half(7, m, K)
        kw = dict(prologue=ops.PRO_SILU_MUL, x2=t["x2"], x_activated=x_activated)

    def call():
        ops.gemv_grouped(t["x"], segments, K, opts=None if opts is None else ops.GemvOpts(**opts), **kw)
    return call, t, [s["y"] for s in segments]


def _sums_case(nseg, sums_in=False, sums_out=False):
    from amq_amd import ops
    m, k = 2, 2048
    t = dict(x=_half(8, m, k))
    segments = []
    for i in range(nseg):
        qn, mn = _layer(t, str(i), N, k, 3 + i % 2)
        t["y%d" % i] = _zeros(m, N)
        segments.append(dict(qn=qn, mn=mn, bits=3 + i % 2, mode=ops.MODE_HQQ, N=N, y=t["y%d" % i]))
    kw = {}
    if sums_in:
        t["gamma"] = 1.0 + 0.1 * _half(9, k)
        t["sums_in"] = (t["x"].float() ** 2).view(m, k // 16, 16).sum(-1).contiguous()
        kw = dict(gamma=t["gamma"], eps=1e-6, sums_in=t["sums_in"])
    if sums_out:
        t["sums_out"] = torch.zeros(m, N // 16, dtype=torch.float32, device=DEV)
        kw["sums_out"] = t["sums_out"]

    def call():
        ops.gemv_grouped_sums(t["x"], segments, k, **kw)
    return call, t, [s["y"] for s in segments] + ([t["sums_out"]] if sums_out else [])


def _gemm_case(shape, route="GEMM_AUTO", residual=False, gate=None, bias=False, group=128, out=True):
    """gate: None, "own" (a tensor of its own), "y" (the output aliases it)"""
    from amq_amd import ops
    m, n, k = shape
    t = dict(x=_half(11, m, k))
    qn, mn = _layer(t, "", n, k, 3, group)
    if bias:
        t["bias"] = _half(12, n)
    if residual:
        t["residual"] = _half(13, m, n)
    if gate:
        t["gate"] = _half(14, m, n)
    if out and gate != "y":
        t["y"] = _zeros(m, n)
    res = []

    def call():
        res.append(ops.gemm(t["x"], qn, mn, 3, ops.MODE_HQQ, n, k, bias=t.get("bias"), out=t["gate"] if gate == "y" else t.get("y"),
                            residual=t.get("residual"), route=getattr(ops, route), gate=t.get("gate")))
    return call, t, res


def _res_norm_case(shape, residual=True, group=128):
    from amq_amd import ops
    m, n, k = shape
    t = dict(x=_half(15, m, k), gamma=1.0 + 0.1 * _half(16, n), y=_zeros(m, n))
    qn, mn = _layer(t, "", n, k, 4, group)
    if residual:
        t["residual"] = _half(17, m, n)
    t["xf"] = torch.zeros(((m + 63) // 64) * 64 * n, dtype=torch.float16, device=DEV)
    res = []

    def call():
        res.extend(ops.gemm_res_norm_xfrag(t["x"], qn, mn, 4, ops.MODE_HQQ, n, k, t["gamma"], 1e-6, residual=t.get("residual"), out=t["y"], xf_out=t["xf"]))
    return call, t, res


def _f16w_case(m, residual=False, gate=False, bias=False):
    from amq_amd import ops
    t = dict(x=_half(18, m, K), w=0.05 * _half(19, N, K), y=_zeros(m, N))
    for name, on, shape in (("bias", bias, (N,)), ("residual", residual, (m, N)), ("gate", gate, (m, N))):
        if on:
            t[name] = _half(20 + len(name), *shape)

    def call():
        ops.gemm_f16w(t["x"], t["w"], bias=t.get("bias"), out=t["y"], residual=t.get("residual"), gate=t.get("gate"))
    return call, t, [t["y"]]


def _xfrag_case(m, residual=False, gate=False, bias=False):
    from amq_amd import ops
    t = dict(xf=ops.xfrag(_half(21, m, K), m, K), y=_zeros(m, N))
    qn, mn = _layer(t, "", N, K, 2)
    for name, on, shape in (("bias", bias, (N,)), ("residual", residual, (m, N)), ("gate", gate, (m, N))):
        if on:
            t[name] = _half(30 + len(name), *shape)

    def call():
        ops.gemm_xfrag(t["xf"], m, qn, mn, 2, ops.MODE_HQQ, N, K, bias=t.get("bias"), out=t["y"], residual=t.get("residual"), gate=t.get("gate"))
    return call, t, [t["y"]]


def _xfrag_grouped_case(m, nseg, form=0, blocks_per_wg=0, residual=False):
    from amq_amd import ops
    t = dict(xf=ops.xfrag(_half(22, m, K), m, K))
    segments = []
    for i in range(nseg):
        qn, mn = _layer(t, str(i), N, K, 2 + i % 3)
        t["y%d" % i] = _zeros(m, N)
        s = dict(qn=qn, mn=mn, bits=2 + i % 3, mode=ops.MODE_HQQ, N=N, y=t["y%d" % i])
        if residual and i == 0:
            s["residual"] = t["res0"] = _half(23, m, N)
            s["bias"] = t["bias0"] = _half(24, N)
        segments.append(s)

    def call():
        ops.gemm_xfrag_grouped(t["xf"], m, segments, K, form=form, blocks_per_wg=blocks_per_wg)
    return call, t, [s["y"] for s in segments]


def _linear_case(m, group=128, bias=False):
    from amq_amd import ops
    t = dict(x=_half(25, m, K))
    qn, mn = _layer(t, "", N, K, 4, group)
    if bias:
        t["bias"] = _half(26, N)
    res = []

    def call():
        res.append(ops.linear(t["x"], qn, mn, 4, ops.MODE_HQQ, N, K, bias=t.get("bias")))
    return call, t, res


CASES = {      # name -> (builder, its arguments, its keyword arguments)
    "gemv one row": (_gemv_case, (1,), {}),
    "gemv 3 rows bias out": (_gemv_case, (3,), dict(bias=True, out=True)),
    "gemv groups of 64": (_gemv_case, (2,), dict(group=64)),
    "gemv opts": (_gemv_case, (1,), dict(opts=dict(waves=8), bias=True)),
    "grouped none": (_grouped_case, (1,), {}),
    "grouped rmsnorm 3 segments": (_grouped_case, (1,), dict(pro="rmsnorm", nseg=3)),
    "grouped silu_mul residual": (_grouped_case, (3,), dict(pro="silu_mul", nseg=1, residual=True)),
    "grouped act": (_grouped_case, (1,), dict(pro="rmsnorm", act=True, bias=True)),
    "grouped act with opts": (_grouped_case, (1,), dict(act=True, opts=dict(math=3, waves=8))),
    "grouped x_activated": (_grouped_case, (1,), dict(pro="silu_mul", nseg=1, x_activated=True)),
    "grouped groups of 32 opts": (_grouped_case, (2,), dict(group=32, opts=dict(depth=2))),
    "sums none": (_sums_case, (2,), {}),
    "sums in": (_sums_case, (2,), dict(sums_in=True)),
    "sums out": (_sums_case, (1,), dict(sums_out=True)),
    "gemm 40 rows": (_gemm_case, ((40, N, K),), dict(out=False)),
    "gemm 300 rows bias": (_gemm_case, ((300, N, K),), dict(bias=True)),
    "gemm 40 rows residual": (_gemm_case, ((40, N, K),), dict(residual=True)),
    "gemm split-K residual": (_gemm_case, (SK,), dict(residual=True)),
    "gemm 300 rows tiled route": (_gemm_case, ((300, N, K), "GEMM_TILED"), {}),
    "gemm 300 rows DEQ route": (_gemm_case, ((300, N, K), "GEMM_DEQ"), {}),
    "gemm 40 rows groups of 64": (_gemm_case, ((40, N, K),), dict(group=64)),
    "gemm 300 rows groups of 32": (_gemm_case, ((300, N, K),), dict(group=32)),
    "gemm 40 rows gated": (_gemm_case, ((40, N, K),), dict(gate="own", bias=True)),
    "gemm 300 rows gated": (_gemm_case, ((300, N, K),), dict(gate="own")),
    "gemm split-K gated": (_gemm_case, (SK,), dict(gate="own")),
    "gemm 40 rows gate is y, fused": (_gemm_case, ((40, N, K),), dict(gate="y")),
    "gemm 300 rows gate is y, not fused": (_gemm_case, ((300, N, K),), dict(gate="y")),
    "gemm split-K gate is y, not fused": (_gemm_case, (SK,), dict(gate="y", bias=True)),
    "gemm 300 rows DEQ route gate is y, fused": (_gemm_case, ((300, N, K), "GEMM_DEQ"), dict(gate="y")),
    "res_norm 40 rows": (_res_norm_case, ((40, N, K),), {}),
    "res_norm split-K": (_res_norm_case, ((SK[0], 128, SK[2]),), {}),
    "res_norm 300 rows groups of 64 no residual": (_res_norm_case, ((300, N, K),), dict(residual=False, group=64)),
    "f16w plain": (_f16w_case, (40,), {}),
    "f16w residual bias": (_f16w_case, (300,), dict(residual=True, bias=True)),
    "f16w gate": (_f16w_case, (40,), dict(gate=True)),
    "xfrag plain": (_xfrag_case, (40,), {}),
    "xfrag gate residual bias": (_xfrag_case, (70,), dict(gate=True, residual=True, bias=True)),
    "xfrag grouped": (_xfrag_grouped_case, (40, 3), {}),
    "xfrag grouped stream form": (_xfrag_grouped_case, (40, 2), dict(form=2, blocks_per_wg=2, residual=True)),
    "linear one row": (_linear_case, (1,), {}),
    "linear 8 rows bias": (_linear_case, (8,), dict(bias=True)),
    "linear 9 rows": (_linear_case, (9,), {}),
    "linear 3 rows groups of 64": (_linear_case, (3,), dict(group=64)),
    "linear 40 rows groups of 32": (_linear_case, (40,), dict(group=32, bias=True)),
}


def record(name, monkeypatch):
    """run case ``name`` once under the recorder -> its records"""
    from amq_amd import _lib, ops
    builder, args, kw = CASES[name]
    call, tensors, outputs = builder(*args, **kw)
    rec = _Recorder(_lib.load(), tensors)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(ops, "_SPLITK_WS", ops._ScratchPool(torch.float32))      # (grow-only: its size would depend on the tests before this one)
    call()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert outputs
    for o in outputs:
        assert bool(torch.isfinite(o.float()).all()), name
    return rec.calls


def _seg(i, bits, bias=None, residual=None):
    return ("seg", "qn%d" % i, "mn%d" % i, bias, residual, "y%d" % i, N, bits, 0, 0)


EXPECTED = {
    "f16w gate": [
        ("amq_gemm_f16w_f16", "x", "w", None, None, "gate", "y", 40, 256, 256, 0, 0, None)],
    "f16w plain": [
        ("amq_gemm_f16w_f16", "x", "w", None, None, None, "y", 40, 256, 256, 0, 0, None)],
    "f16w residual bias": [
        ("amq_gemm_f16w_f16", "x", "w", "bias", "residual", None, "y", 300, 256, 256, 0, 0, None)],
    "gemm 300 rows DEQ route": [
        ("amq_gemm_route_f16", 6, 3, 0, "x", "qn", "mn", None, None, "y", 300, 256, 256, 128, 0, 0, "ptr", 131072, None)],
    "gemm 300 rows DEQ route gate is y, fused": [
        ("amq_gemm_gated_f16", 6, 3, 0, "x", "qn", "mn", None, "gate", "gate", 300, 256, 256, 128, 0, "ptr", 131072, None)],
    "gemm 300 rows bias": [
        ("amq_gemm_route_f16", 0, 3, 0, "x", "qn", "mn", "bias", None, "y", 300, 256, 256, 128, 0, 0, None, 0, None)],
    "gemm 300 rows gate is y, not fused": [
        ("amq_gemm_route_f16", 0, 3, 0, "x", "qn", "mn", None, None, "ptr", 300, 256, 256, 128, 0, 0, None, 0, None),
        ("amq_silu_mul_f16", "gate", "ptr", "gate", 76800, None)],
    "gemm 300 rows gated": [
        ("amq_gemm_gated_f16", 0, 3, 0, "x", "qn", "mn", None, "gate", "y", 300, 256, 256, 128, 0, None, 0, None)],
    "gemm 300 rows groups of 32": [
        ("amq_gemm_route_f16", 0, 3, 0, "x", "qn", "mn", None, None, "y", 300, 256, 256, 32, 0, 0, None, 0, None)],
    "gemm 300 rows tiled route": [
        ("amq_gemm_route_f16", 1, 3, 0, "x", "qn", "mn", None, None, "y", 300, 256, 256, 128, 0, 0, None, 0, None)],
    "gemm 40 rows": [
        ("amq_gemm_route_f16", 0, 3, 0, "x", "qn", "mn", None, None, "ptr", 40, 256, 256, 128, 0, 0, None, 0, None)],
    "gemm 40 rows gate is y, fused": [
        ("amq_gemm_gated_f16", 0, 3, 0, "x", "qn", "mn", None, "gate", "gate", 40, 256, 256, 128, 0, None, 0, None)],
    "gemm 40 rows gated": [
        ("amq_gemm_gated_f16", 0, 3, 0, "x", "qn", "mn", "bias", "gate", "y", 40, 256, 256, 128, 0, None, 0, None)],
    "gemm 40 rows groups of 64": [
        ("amq_gemm_route_f16", 0, 3, 0, "x", "qn", "mn", None, None, "y", 40, 256, 256, 64, 0, 0, None, 0, None)],
    "gemm 40 rows residual": [
        ("amq_gemm_route_f16", 0, 3, 0, "x", "qn", "mn", None, "residual", "y", 40, 256, 256, 128, 0, 0, None, 0, None)],
    "gemm split-K gate is y, not fused": [
        ("amq_gemm_route_f16", 0, 3, 0, "x", "qn", "mn", "bias", None, "ptr", 65, 16, 512, 128, 0, 0, "ptr", 8320, None),
        ("amq_silu_mul_f16", "gate", "ptr", "gate", 1040, None)],
    "gemm split-K gated": [
        ("amq_gemm_gated_f16", 0, 3, 0, "x", "qn", "mn", None, "gate", "y", 65, 16, 512, 128, 0, "ptr", 8320, None)],
    "gemm split-K residual": [
        ("amq_gemm_route_f16", 0, 3, 0, "x", "qn", "mn", None, "residual", "y", 65, 16, 512, 128, 0, 0, "ptr", 8320, None)],
    "gemv 3 rows bias out": [
        ("amq_gemv_f16", 3, 0, "x", "qn", "mn", "bias", "y", 3, 256, 256, 128, 0, 0, None)],
    "gemv groups of 64": [
        ("amq_gemv_f16", 3, 0, "x", "qn", "mn", None, "ptr", 2, 256, 256, 64, 0, 0, None)],
    "gemv one row": [
        ("amq_gemv_f16", 3, 0, "x", "qn", "mn", None, "ptr", 1, 256, 256, 128, 0, 0, None)],
    "gemv opts": [
        ("amq_gemv_grouped_f16", (("seg", "qn", "mn", "bias", None, "ptr", 256, 3, 0, 0),), 1, "x", None, None, 0.0, 0, 1, 256, 128, 0, ("opts", 0, 8, 0, 0, 0, 0), None)],
    "grouped act": [
        ("amq_gemv_grouped_f16", (_seg(0, 2, "bias0"), _seg(1, 3)), 2, "x", None, "gamma", EPS, 1, 1, 256, 128, 0, ("opts", 0, 0, 0, 0, 0, 1), None)],
    "grouped act with opts": [
        ("amq_gemv_grouped_f16", (_seg(0, 2), _seg(1, 3)), 2, "x", None, None, 0.0, 0, 1, 256, 128, 0, ("opts", 3, 8, 0, 0, 0, 1), None)],
    "grouped groups of 32 opts": [
        ("amq_gemv_grouped_f16", (_seg(0, 2), _seg(1, 3)), 2, "x", None, None, 0.0, 0, 2, 256, 32, 0, ("opts", 0, 0, 2, 0, 0, 0), None)],
    "grouped none": [
        ("amq_gemv_grouped_f16", (_seg(0, 2), _seg(1, 3)), 2, "x", None, None, 0.0, 0, 1, 256, 128, 0, None, None)],
    "grouped rmsnorm 3 segments": [
        ("amq_gemv_grouped_f16", (_seg(0, 2), _seg(1, 3), _seg(2, 4)), 3, "x", None, "gamma", EPS, 1, 1, 256, 128, 0, None, None)],
    "grouped silu_mul residual": [
        ("amq_gemv_grouped_f16", (_seg(0, 2, None, "res0"),), 1, "x", "x2", None, 0.0, 2, 3, 256, 128, 0, None, None)],
    "grouped x_activated": [
        ("amq_gemv_grouped_f16", (_seg(0, 2),), 1, "x", "x2", None, 0.0, 4, 1, 256, 128, 0, None, None)],
    "linear 3 rows groups of 64": [
        ("amq_gemv_f16", 4, 0, "x", "qn", "mn", None, "ptr", 3, 256, 256, 64, 0, 0, None)],
    "linear 40 rows groups of 32": [
        ("amq_gemm_route_f16", 0, 4, 0, "x", "qn", "mn", "bias", None, "ptr", 40, 256, 256, 32, 0, 0, None, 0, None)],
    "linear 8 rows bias": [
        ("amq_linear_f16", 4, 0, "x", "qn", "mn", "bias", "ptr", 8, 256, 256, 128, None)],
    "linear 9 rows": [
        ("amq_gemm_route_f16", 0, 4, 0, "x", "qn", "mn", None, None, "ptr", 9, 256, 256, 128, 0, 0, None, 0, None)],
    "linear one row": [
        ("amq_linear_f16", 4, 0, "x", "qn", "mn", None, "ptr", 1, 256, 256, 128, None)],
    "res_norm 300 rows groups of 64 no residual": [
        ("amq_gemm_res_norm_xfrag_f16", 4, 0, "x", "qn", "mn", None, None, "y", 300, 256, 256, 64, 0, None, 0, "gamma", 1e-06, "xf", None)],
    "res_norm 40 rows": [
        ("amq_gemm_res_norm_xfrag_f16", 4, 0, "x", "qn", "mn", None, "residual", "y", 40, 256, 256, 128, 0, None, 0, "gamma", 1e-06, "xf", None)],
    "res_norm split-K": [
        ("amq_gemm_res_norm_xfrag_f16", 4, 0, "x", "qn", "mn", None, "residual", "y", 65, 128, 512, 128, 0, "ptr", 66560, "gamma", 1e-06, "xf", None)],
    "sums in": [
        ("amq_gemv_grouped_sums_f16", (_seg(0, 3), _seg(1, 4)), 2, "x", "gamma", EPS, "sums_in", None, 2, 2048, 128, None)],
    "sums none": [
        ("amq_gemv_grouped_sums_f16", (_seg(0, 3), _seg(1, 4)), 2, "x", None, 0.0, None, None, 2, 2048, 128, None)],
    "sums out": [
        ("amq_gemv_grouped_sums_f16", (_seg(0, 3),), 1, "x", None, 0.0, None, "sums_out", 2, 2048, 128, None)],
    "xfrag gate residual bias": [
        ("amq_gemm_xfrag_f16", 2, 0, "xf", "qn", "mn", "bias", "gate", "residual", "y", 70, 256, 256, 128, 0, None)],
    "xfrag grouped": [
        ("amq_gemm_xfrag_grouped_form_f16", (_seg(0, 2), _seg(1, 3), _seg(2, 4)), 3, "xf", 40, 256, 128, 0, 0, None)],
    "xfrag grouped stream form": [
        ("amq_gemm_xfrag_grouped_form_f16", (_seg(0, 2, "bias0", "res0"), _seg(1, 3)), 2, "xf", 40, 256, 128, 2, 2, None)],
    "xfrag plain": [
        ("amq_gemm_xfrag_f16", 2, 0, "xf", "qn", "mn", None, None, None, "y", 40, 256, 256, 128, 0, None)],
}


def test_the_split_k_shape_is_the_smallest():
    """no smaller M, N (a multiple of 16) or K (a multiple of 128) has split-K partials, by the host query"""
    from amq_amd import _lib
    lib = _lib.load()
    m, n, k = SK
    assert lib.amq_gemm_route_workspace_bytes(_lib.GEMM_AUTO, m, n, k) == 2 * m * n * 4
    for mm, nn, kk in ((m - 1, n, k), (m, n, k - 128)):
        assert lib.amq_gemm_route_workspace_bytes(_lib.GEMM_AUTO, mm, nn, kk) == 0
    assert lib.amq_gemm_route_workspace_bytes(_lib.GEMM_AUTO, m, 128, k) == 2 * m * 128 * 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_point_and_arguments_of_each_dispatch_branch(name, monkeypatch):
    calls = record(name, monkeypatch)
    print(repr(name), ":", calls)
    assert calls == EXPECTED[name]
