"""CPU-only: what the fp16 matmul C entry points check ("Matmul entry points: what is checked") -- one refused call per rule and per
entry point of the two families (weight-streaming GEMV / grouped few-row calls, packed GEMM), with the return code and a distinctive piece of
the message, and the host queries over a small grid against values recorded from the commit before the entry points shared their validators
(tests/golden/matmul_entry_queries.json).

Dummy non-null pointers as in tests/test_strided_cpu.py; every call breaks exactly ONE rule, so no call of this file reaches a launch and none
depends on the order of the checks."""
import ctypes
import itertools
import json
import os

import pytest

from amq_amd import _lib

EINVAL, ESHAPE = -1, -2
ONE, TWO = ctypes.c_void_p(256), ctypes.c_void_p(512)
N, K = 256, 256
BIG_N, BIG_K = 4096, 4096        # 80 rows of it run split-K (amq_gemm_splitk_workspace_bytes != 0)
FP = ctypes.cast(256, ctypes.c_void_p)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matmul_entry_queries.json")
ROUTES = (_lib.GEMM_AUTO, _lib.GEMM_TILED, _lib.GEMM_SKINNY, _lib.GEMM_RING, _lib.GEMM_RING128, _lib.GEMM_WS, _lib.GEMM_DEQ)


def seg(n=N, bits=3, mode=0, qn=256, mn=256, y=256, residual=None, bias=None, ys=0):
    return _lib.Segment(qn, mn, bias, residual, y, n, bits, mode, ys)


def segs(*ss):
    ss = ss or (seg(), seg(bits=4))
    return (_lib.Segment * len(ss))(*ss)


def opts(**kw):
    return ctypes.byref(_lib.GemvOpts(**kw))


def grouped(lib, ss=None, nseg=None, x=ONE, x2=None, gamma=None, pro=_lib.PRO_NONE, M=1, k=K, group=128, o=None):
    ss = segs() if ss is None else ss
    return lib.amq_gemv_grouped_f16(ss, len(ss) if nseg is None else nseg, x, x2, gamma, 1e-6, pro, M, k, group, 0, o, None)


def sums(lib, ss=None, nseg=None, x=ONE, gamma=None, sums_in=None, sums_out=None, M=2, k=2048, group=128):
    ss = segs() if ss is None else ss
    return lib.amq_gemv_grouped_sums_f16(ss, len(ss) if nseg is None else nseg, x, gamma, 1e-6, sums_in, sums_out, M, k, group, None)


def xf_grouped(lib, ss=None, nseg=None, xf=ONE, M=40, k=K, group=128, form=_lib.FEWROW_AUTO, bpw=0):
    ss = segs() if ss is None else ss
    return lib.amq_gemm_xfrag_grouped_form_f16(ss, len(ss) if nseg is None else nseg, xf, M, k, group, form, bpw, None)


def gemv1(lib, bits=3, mode=0, x=ONE, qn=ONE, mn=ONE, y=ONE, M=1, n=N, k=K, group=128):
    return lib.amq_gemv_f16(bits, mode, x, qn, mn, None, y, M, n, k, group, 0, 0, None)


# ---- the segments of the three grouped calls: shape / mode / null pointers per segment --------------------------------------------
SEGMENT_RULES = {       # name -> (second segment, group, code, piece of the message)
    "bits": (seg(bits=5), 128, EINVAL, b"bits must be 2, 3 or 4 (got 5)"),
    "N": (seg(n=250), 128, ESHAPE, b"need N % 16 == 0 and K % 128 == 0 (got N=250 K="),
    "mode": (seg(mode=3), 128, EINVAL, b"unknown dequant mode 3"),
    "null qweight": (seg(qn=None), 128, EINVAL, b"segment 1: null pointer"),
    "null meta": (seg(mn=None), 128, EINVAL, b"segment 1: null pointer"),
    "null y": (seg(y=None), 128, EINVAL, b"segment 1: null pointer"),
    "group 96": (seg(), 96, ESHAPE, b"group size must be 32, 64 or a multiple of 128 (got 96)"),
}
GROUPED_CALLS = {"amq_gemv_grouped_f16": (grouped, {}), "amq_gemv_grouped_sums_f16": (sums, {}), "amq_gemm_xfrag_grouped_f16": (xf_grouped, {})}


@pytest.mark.parametrize("fn", sorted(GROUPED_CALLS))
@pytest.mark.parametrize("rule", sorted(SEGMENT_RULES))
def test_per_segment_rules_of_the_grouped_calls(fn, rule):
    lib = _lib.load()
    call, kw = GROUPED_CALLS[fn]
    second, group, code, piece = SEGMENT_RULES[rule]
    rc = call(lib, ss=segs(seg(), second), group=group, **kw)
    assert (rc, piece in lib.amq_last_error()) == (code, True), (rc, lib.amq_last_error())


def test_a_group_that_does_not_divide_K():
    lib = _lib.load()
    for call, k in ((grouped, 256), (sums, 2176), (xf_grouped, 256)):       # 2176 = 17 * 128
        rc = call(lib, k=k, group=384)
        assert rc == ESHAPE and b"group size 384 does not divide K=%d" % k in lib.amq_last_error(), lib.amq_last_error()


def test_the_calls_of_groups_of_128_name_themselves_on_finer_groups():
    lib = _lib.load()
    for group in (64, 32):
        rc = xf_grouped(lib, group=group)
        assert rc == ESHAPE and b"amq_gemm_xfrag_grouped_f16 serves groups of 128 (and multiples); groups of %d" % group in lib.amq_last_error()
        rc = lib.amq_gemm_xfrag_f16(3, 0, ONE, ONE, ONE, None, None, None, ONE, 40, N, K, group, 0, None)
        assert rc == ESHAPE and b"amq_gemm_xfrag_f16 serves groups of 128 (and multiples); groups of %d" % group in lib.amq_last_error()
        rc = sums(lib, group=group)
        assert rc == ESHAPE and b"groups of 128 (and multiples) only (got %d)" % group in lib.amq_last_error()


# ---- amq_gemv_grouped_f16 / amq_gemv_f16 -----------------------------------------------------------------------------------------------
def _lds_rows(lib, k):
    out = (ctypes.c_int * 6)()
    lib.amq_query(k, out, 6)
    return list(out)


GEMV_RULES = {      # name -> (call(lib), code, piece of the message)
    "nseg 0": (lambda lib: grouped(lib, nseg=0), EINVAL, b"nseg must be 1..4 (got 0)"),
    "nseg 5": (lambda lib: grouped(lib, nseg=5), EINVAL, b"nseg must be 1..4 (got 5)"),
    "null segs": (lambda lib: lib.amq_gemv_grouped_f16(None, 1, ONE, None, None, 0.0, 0, 1, K, 128, 0, None, None), EINVAL, b"nseg must be 1..4 (got 1)"),
    "null x": (lambda lib: grouped(lib, x=None), EINVAL, b"null x"),
    "prologue 3": (lambda lib: grouped(lib, pro=3, x2=ONE, gamma=ONE), EINVAL, b"unknown prologue 3"),
    "prologue 5": (lambda lib: grouped(lib, pro=5, x2=ONE, gamma=ONE), EINVAL, b"unknown prologue 5"),
    "prologue -1": (lambda lib: grouped(lib, pro=-1, x2=ONE, gamma=ONE), EINVAL, b"unknown prologue -1"),
    "no gamma": (lambda lib: grouped(lib, pro=_lib.PRO_RMSNORM, x2=ONE), EINVAL, b"RMSNorm prologue needs gamma"),
    "SiLU*mul no x2": (lambda lib: grouped(lib, pro=_lib.PRO_SILU_MUL, gamma=ONE), EINVAL, b"SiLU*mul prologue needs x2"),
    "mul no x2": (lambda lib: grouped(lib, pro=_lib.PRO_MUL, gamma=ONE), EINVAL, b"mul prologue needs x2"),
    "M 0": (lambda lib: grouped(lib, M=0), ESHAPE, b"M must be >= 1 (got 0)"),
    "M -3": (lambda lib: grouped(lib, M=-3), ESHAPE, b"M must be >= 1 (got -3)"),
    "math -1": (lambda lib: grouped(lib, o=opts(math=-1)), EINVAL, b"opts.math must be AMQ_MATH_DEFAULT"),
    "math 4": (lambda lib: grouped(lib, o=opts(math=4)), EINVAL, b"opts.math must be AMQ_MATH_DEFAULT"),
    "waves 3": (lambda lib: grouped(lib, o=opts(waves=3)), EINVAL, b"opts.waves must be 0, 4, 8 or 16"),
    "waves 32": (lambda lib: grouped(lib, o=opts(waves=32)), EINVAL, b"opts.waves must be 0, 4, 8 or 16"),
    "depth 3": (lambda lib: grouped(lib, o=opts(depth=3)), EINVAL, b"opts.depth must be 0, 2, 4 or AMQ_GEMV_DEPTH_GENERIC"),
    "depth -2": (lambda lib: grouped(lib, o=opts(depth=-2)), EINVAL, b"opts.depth must be 0, 2, 4 or AMQ_GEMV_DEPTH_GENERIC"),
    "rpt -1": (lambda lib: grouped(lib, o=opts(rpt=-1)), EINVAL, b"opts.rpt (row-tiles per workgroup) must be 0..64"),
    "rpt 65": (lambda lib: grouped(lib, o=opts(rpt=65)), EINVAL, b"opts.rpt (row-tiles per workgroup) must be 0..64"),
    "act_mask -1": (lambda lib: grouped(lib, o=opts(act_mask=-1)), EINVAL, b"opts.act_mask names segments 0..1 (got 0xffffffff)"),
    "act_mask beyond nseg": (lambda lib: grouped(lib, o=opts(act_mask=4)), EINVAL, b"opts.act_mask names segments 0..1 (got 0x4)"),
    "act_mask, groups of 64": (lambda lib: grouped(lib, group=64, o=opts(act_mask=1)), ESHAPE,
                               b"opts.act_mask / AMQ_PRO_MUL: groups of 128 (and multiples) only (got 64); use AMQ_PRO_SILU_MUL"),
    "PRO_MUL, groups of 32": (lambda lib: grouped(lib, group=32, pro=_lib.PRO_MUL, x2=ONE), ESHAPE,
                              b"opts.act_mask / AMQ_PRO_MUL: groups of 128 (and multiples) only (got 32); use AMQ_PRO_SILU_MUL"),
    "17 rows": (lambda lib: grouped(lib, M=17), ESHAPE, b"M=17 rows of K=256 do not fit LDS for the GEMV path; use amq_gemm_f16"),
    "act with residual": (lambda lib: grouped(lib, ss=segs(seg(), seg(residual=256)), o=opts(act_mask=2)), EINVAL,
                          b"segment 1: an activated output (opts.act_mask) takes no residual"),
    "dot, groups of 64": (lambda lib: grouped(lib, group=64, o=opts(dot=1)), EINVAL, b"groups of 64: the GEMV kernel's default form only"),
    "linear math, groups of 32": (lambda lib: grouped(lib, group=32, o=opts(math=_lib.MATH_LINEAR)), EINVAL, b"groups of 32: the GEMV kernel's default form only"),
    "depth 4, groups of 64": (lambda lib: grouped(lib, group=64, o=opts(depth=4)), EINVAL, b"groups of 64: the GEMV kernel's default form only"),
    "amq_gemv_f16 null x": (lambda lib: gemv1(lib, x=None), EINVAL, b"null x"),
    "amq_gemv_f16 M 0": (lambda lib: gemv1(lib, M=0), ESHAPE, b"M must be >= 1 (got 0)"),
    "amq_gemv_f16 17 rows": (lambda lib: gemv1(lib, M=17), ESHAPE, b"M=17 rows of K=256 do not fit LDS"),
    "amq_gemv_f16 bits": (lambda lib: gemv1(lib, bits=1), EINVAL, b"bits must be 2, 3 or 4 (got 1)"),
    "amq_gemv_f16 K": (lambda lib: gemv1(lib, k=200), ESHAPE, b"need N % 16 == 0 and K % 128 == 0 (got N=256 K=200)"),
    "amq_gemv_f16 mode": (lambda lib: gemv1(lib, mode=-1), EINVAL, b"unknown dequant mode -1"),
    "amq_gemv_f16 null y": (lambda lib: gemv1(lib, y=None), EINVAL, b"segment 0: null pointer"),
    "amq_gemv_f16 null qn": (lambda lib: gemv1(lib, qn=None), EINVAL, b"segment 0: null pointer"),
}


def _check(lib, table, name):
    call, code, piece = table[name]
    rc = call(lib)
    msg = lib.amq_last_error()
    assert rc == code and piece in msg, (name, rc, msg)


@pytest.mark.parametrize("name", sorted(GEMV_RULES))
def test_gemv_rules(name):
    _check(_lib.load(), GEMV_RULES, name)


def test_gemv_rows_that_do_not_fit_lds():
    """the row limit of a K is amq_query's: one row more is refused -- whatever the options (vals[0]), and with default options (vals[4])"""
    lib = _lib.load()
    k = 11008
    any_opts, plain = _lds_rows(lib, k)[0], _lds_rows(lib, k)[4]
    assert any_opts < plain < 16
    assert grouped(lib, M=plain + 1, k=k, pro=_lib.PRO_RMSNORM, gamma=ONE) == ESHAPE
    assert b"M=%d rows of K=11008 do not fit LDS for the GEMV path; use amq_gemm_f16" % (plain + 1) in lib.amq_last_error()
    assert grouped(lib, M=any_opts + 1, k=k, o=opts(waves=4)) == ESHAPE
    assert b"M=%d rows of K=11008 do not fit LDS" % (any_opts + 1) in lib.amq_last_error()


# ---- amq_gemv_grouped_sums_f16 ---------------------------------------------------------------------------------------------------------
SUMS_RULES = {
    "nseg 0": (lambda lib: sums(lib, nseg=0), EINVAL, b"nseg must be 1..4 (got 0)"),
    "nseg 5": (lambda lib: sums(lib, nseg=5), EINVAL, b"nseg must be 1..4 (got 5)"),
    "null x": (lambda lib: sums(lib, x=None), EINVAL, b"null x"),
    "sums_in without gamma": (lambda lib: sums(lib, sums_in=FP), EINVAL, b"sums_in (the partial sums of squares of x) and gamma go together"),
    "gamma without sums_in": (lambda lib: sums(lib, gamma=ONE), EINVAL, b"sums_in (the partial sums of squares of x) and gamma go together"),
    "one row": (lambda lib: sums(lib, M=1), ESHAPE, b"the partial-sum forms live in the 2 .. 8-row kernels (got M=1)"),
    "nine rows": (lambda lib: sums(lib, M=9), ESHAPE, b"the partial-sum forms live in the 2 .. 8-row kernels (got M=9)"),
    "K 1920": (lambda lib: sums(lib, k=1920), ESHAPE, b"K >= 2048 (the 2 .. 8-row kernels run 8 or 16 waves per workgroup; got K=1920)"),
    "sums_out of two": (lambda lib: sums(lib, sums_out=FP), EINVAL, b"sums_out describes ONE output: nseg must be 1"),
    "sums_out with sums_in": (lambda lib: sums(lib, ss=segs(seg()), sums_out=FP, sums_in=FP, gamma=ONE), EINVAL,
                              b"sums_out is written by launches without a prologue"),
    "sums_in K 8320": (lambda lib: sums(lib, sums_in=FP, gamma=ONE, k=8320), ESHAPE, b"sums_in: K <= 8192 (K / 16 <= 512 partials per row; got K=8320)"),
    "rows beyond LDS": (lambda lib: sums(lib, M=8, k=32768), ESHAPE, b"M=8 rows of K=32768 do not fit LDS for the GEMV path"),
}


@pytest.mark.parametrize("name", sorted(SUMS_RULES))
def test_partial_sum_gemv_rules(name):
    _check(_lib.load(), SUMS_RULES, name)


# ---- the fragment-ordered pair ---------------------------------------------------------------------------------------------------------
def xf1(lib, bits=3, mode=0, xf=ONE, qn=ONE, mn=ONE, y=ONE, M=40, n=N, k=K, group=128):
    return lib.amq_gemm_xfrag_f16(bits, mode, xf, qn, mn, None, None, None, y, M, n, k, group, 0, None)


MANY = 65535 * 64 + 1
XFRAG_RULES = {
    "form -1": (lambda lib: xf_grouped(lib, form=-1), EINVAL, b"unknown few-row form -1"),
    "form 3": (lambda lib: xf_grouped(lib, form=3), EINVAL, b"unknown few-row form 3"),
    "blocks without STREAM": (lambda lib: xf_grouped(lib, form=_lib.FEWROW_TILE, bpw=2), EINVAL, b"blocks_per_wg is 0, or 1 / 2 / 3 / 4 / 6 with AMQ_FEWROW_STREAM (got 2)"),
    "blocks 5": (lambda lib: xf_grouped(lib, form=_lib.FEWROW_STREAM, bpw=5), EINVAL, b"blocks_per_wg is 0, or 1 / 2 / 3 / 4 / 6 with AMQ_FEWROW_STREAM (got 5)"),
    "blocks 7": (lambda lib: xf_grouped(lib, form=_lib.FEWROW_STREAM, bpw=7), EINVAL, b"blocks_per_wg is 0, or 1 / 2 / 3 / 4 / 6 with AMQ_FEWROW_STREAM (got 7)"),
    "blocks -1": (lambda lib: xf_grouped(lib, form=_lib.FEWROW_STREAM, bpw=-1), EINVAL, b"blocks_per_wg is 0, or 1 / 2 / 3 / 4 / 6 with AMQ_FEWROW_STREAM (got -1)"),
    "nseg 0": (lambda lib: xf_grouped(lib, nseg=0), EINVAL, b"nseg must be 1..4 (got 0)"),
    "nseg 5": (lambda lib: xf_grouped(lib, nseg=5), EINVAL, b"nseg must be 1..4 (got 5)"),
    "null xf": (lambda lib: xf_grouped(lib, xf=None), EINVAL, b"null xf"),
    "M 0": (lambda lib: xf_grouped(lib, M=0), ESHAPE, b"M must be >= 1 (got 0)"),
    "M beyond a launch": (lambda lib: xf_grouped(lib, M=MANY), ESHAPE, b"M=%d exceeds one launch" % MANY),
    "auto form, M 0": (lambda lib: lib.amq_gemm_xfrag_grouped_f16(segs(), 2, ONE, 0, K, 128, None), ESHAPE, b"M must be >= 1 (got 0)"),
    "single bits": (lambda lib: xf1(lib, bits=5), EINVAL, b"bits must be 2, 3 or 4 (got 5)"),
    "single N": (lambda lib: xf1(lib, n=250), ESHAPE, b"need N % 16 == 0 and K % 128 == 0 (got N=250 K=256)"),
    "single mode": (lambda lib: xf1(lib, mode=3), EINVAL, b"unknown dequant mode 3"),
    "single null xf": (lambda lib: xf1(lib, xf=None), EINVAL, b"null pointer"),
    "single null y": (lambda lib: xf1(lib, y=None), EINVAL, b"null pointer"),
    "single M 0": (lambda lib: xf1(lib, M=0), ESHAPE, b"M must be >= 1 (got 0)"),
    "single M beyond a launch": (lambda lib: xf1(lib, M=MANY), ESHAPE, b"M=%d exceeds one launch" % MANY),
}


@pytest.mark.parametrize("name", sorted(XFRAG_RULES))
def test_fragment_ordered_gemm_rules(name):
    _check(_lib.load(), XFRAG_RULES, name)


# ---- the packed GEMM family ------------------------------------------------------------------------------------------------------------
def gemm(lib, bits=3, mode=0, x=ONE, qn=ONE, mn=ONE, y=ONE, M=40, n=N, k=K, group=128):
    return lib.amq_gemm_f16(bits, mode, x, qn, mn, None, y, M, n, k, group, 0, 0, None)


def splitk(lib, bits=3, mode=0, x=ONE, qn=ONE, mn=ONE, y=ONE, M=80, n=BIG_N, k=BIG_K, group=128, ws=ONE, ws_bytes=1 << 40):
    return lib.amq_gemm_splitk_f16(bits, mode, x, qn, mn, None, y, M, n, k, group, 0, 0, ws, ws_bytes, None)


def route(lib, r=_lib.GEMM_AUTO, bits=3, mode=0, x=ONE, qn=ONE, mn=ONE, residual=None, y=ONE, M=40, n=N, k=K, group=128, ws=None, ws_bytes=0):
    return lib.amq_gemm_route_f16(r, bits, mode, x, qn, mn, None, residual, y, M, n, k, group, 0, 0, ws, ws_bytes, None)


def res(lib, bits=3, mode=0, x=ONE, qn=ONE, mn=ONE, y=ONE, M=40, n=N, k=K, group=128, ws=None, ws_bytes=0):
    return lib.amq_gemm_res_f16(bits, mode, x, qn, mn, None, ONE, y, M, n, k, group, 0, 0, ws, ws_bytes, None)


def res_norm(lib, bits=3, mode=0, x=ONE, qn=ONE, mn=ONE, y=ONE, M=40, n=N, k=K, group=128, ws=None, ws_bytes=0, gamma=ONE, xf=ONE):
    return lib.amq_gemm_res_norm_xfrag_f16(bits, mode, x, qn, mn, None, ONE, y, M, n, k, group, 0, ws, ws_bytes, gamma, 1e-6, xf, None)


def gated(lib, r=_lib.GEMM_AUTO, bits=3, mode=0, x=ONE, qn=ONE, mn=ONE, gate=ONE, y=TWO, M=40, n=N, k=K, group=128, ws=None, ws_bytes=0):
    return lib.amq_gemm_gated_f16(r, bits, mode, x, qn, mn, None, gate, y, M, n, k, group, 0, ws, ws_bytes, None)


SHARED_GEMM_RULES = {       # the prefix every packed-GEMM entry point shares: name -> (keyword arguments, code, piece of the message)
    "bits": (dict(bits=5), EINVAL, b"bits must be 2, 3 or 4 (got 5)"),
    "group": (dict(group=96), ESHAPE, b"group size must be 32, 64 or a multiple of 128 (got 96)"),
    "N": (dict(n=250), ESHAPE, b"need N % 16 == 0 and K % 128 == 0 (got N=250 K="),
    "K": (dict(k=192), ESHAPE, b"need N % 16 == 0 and K % 128 == 0 (got N="),
    "group divides K": (dict(k=640, group=256), ESHAPE, b"group size 256 does not divide K=640"),
    "mode": (dict(mode=3), EINVAL, b"unknown dequant mode 3"),
    "null x": (dict(x=None), EINVAL, b"null pointer"),
    "null qn": (dict(qn=None), EINVAL, b"null pointer"),
    "null mn": (dict(mn=None), EINVAL, b"null pointer"),
    "null y": (dict(y=None), EINVAL, b"null pointer"),
    "M 0": (dict(M=0), ESHAPE, b"M must be >= 1 (got 0)"),
}
GEMM_CALLS = {"amq_gemm_f16": gemm, "amq_gemm_splitk_f16": splitk, "amq_gemm_route_f16": route, "amq_gemm_res_f16": res,
              "amq_gemm_res_norm_xfrag_f16": res_norm, "amq_gemm_gated_f16": gated}


@pytest.mark.parametrize("fn", sorted(GEMM_CALLS))
@pytest.mark.parametrize("rule", sorted(SHARED_GEMM_RULES))
def test_shared_rules_of_the_packed_gemm_entry_points(fn, rule):
    lib = _lib.load()
    kw, code, piece = SHARED_GEMM_RULES[rule]
    if fn == "amq_gemm_res_norm_xfrag_f16" and rule == "N":
        piece = b"N % 128 == 0 (got N=250)"           # (its own rule on N speaks first: the rows are handed on in fragment order)
    rc = GEMM_CALLS[fn](lib, **kw)
    msg = lib.amq_last_error()
    assert rc == code and piece in msg, (rc, msg)


DEQ_BYTES = N * K * 2
HUGE_M = 1 << 20            # rows of K = 8192 that span 16 GiB: the fp16-weight GEMM of the dequantize-once route addresses below 4 GiB
GEMM_RULES = {
    "route -1": (lambda lib: route(lib, r=-1), EINVAL, b"unknown GEMM route -1"),
    "route 7": (lambda lib: route(lib, r=7), EINVAL, b"unknown GEMM route 7"),
    "gated route -1": (lambda lib: gated(lib, r=-1), EINVAL, b"unknown GEMM route -1"),
    "gated route 7": (lambda lib: gated(lib, r=7), EINVAL, b"unknown GEMM route 7"),
    "gated null gate": (lambda lib: gated(lib, gate=None), EINVAL, b"null pointer"),
    "few-row route, 65 rows": (lambda lib: route(lib, r=_lib.GEMM_SKINNY, M=65), ESHAPE, b"the few-row kernel takes at most 64 rows (got 65)"),
    "few-row route, 257 rows of groups of 64": (lambda lib: route(lib, r=_lib.GEMM_SKINNY, M=257, group=64), ESHAPE, b"the few-row kernel takes at most 64 rows (got 257)"),
    "gated few-row route, 65 rows": (lambda lib: gated(lib, r=_lib.GEMM_SKINNY, M=65), ESHAPE, b"the few-row kernel takes at most 64 rows (got 65)"),
    "gated few-row route, 257 rows of groups of 32": (lambda lib: gated(lib, r=_lib.GEMM_SKINNY, M=257, group=32), ESHAPE, b"the few-row kernel takes at most 64 rows (got 257)"),
    "DEQ without a workspace": (lambda lib: route(lib, r=_lib.GEMM_DEQ), EINVAL, b"AMQ_GEMM_DEQ needs a workspace of N * K * 2 bytes for the fp16 weights"),
    "DEQ without a workspace, groups of 64": (lambda lib: route(lib, r=_lib.GEMM_DEQ, group=64), EINVAL, b"AMQ_GEMM_DEQ needs a workspace of N * K * 2 bytes"),
    "gated DEQ without a workspace": (lambda lib: gated(lib, r=_lib.GEMM_DEQ), EINVAL, b"AMQ_GEMM_DEQ needs a workspace of N * K * 2 bytes for the fp16 weights"),
    "gated DEQ without a workspace, groups of 32": (lambda lib: gated(lib, r=_lib.GEMM_DEQ, group=32), EINVAL, b"AMQ_GEMM_DEQ needs a workspace of N * K * 2 bytes"),
    "DEQ workspace too small": (lambda lib: route(lib, r=_lib.GEMM_DEQ, ws=ONE, ws_bytes=DEQ_BYTES - 1), EINVAL,
                                b"workspace too small: need %d bytes, got %d" % (DEQ_BYTES, DEQ_BYTES - 1)),
    "gated DEQ workspace too small": (lambda lib: gated(lib, r=_lib.GEMM_DEQ, group=64, ws=ONE, ws_bytes=16), EINVAL,
                                      b"workspace too small: need %d bytes, got 16" % DEQ_BYTES),
    "split-K workspace too small": (lambda lib: route(lib, M=80, n=BIG_N, k=BIG_K, ws=ONE, ws_bytes=64), EINVAL, b"workspace too small: need "),
    "res split-K workspace too small": (lambda lib: res(lib, M=80, n=BIG_N, k=BIG_K, ws=ONE, ws_bytes=64), EINVAL, b"workspace too small: need "),
    "res_norm split-K workspace too small": (lambda lib: res_norm(lib, M=80, n=BIG_N, k=BIG_K, ws=ONE, ws_bytes=64), EINVAL, b"workspace too small: need "),
    "gated split-K workspace too small": (lambda lib: gated(lib, M=80, n=BIG_N, k=BIG_K, ws=ONE, ws_bytes=64), EINVAL, b"workspace too small: need "),
    "splitk entry without a workspace": (lambda lib: splitk(lib, ws=None), EINVAL, b"split-K workspace too small: need "),
    "splitk entry workspace too small": (lambda lib: splitk(lib, ws_bytes=64), EINVAL, b"split-K workspace too small: need "),
    "DEQ beyond 4 GiB of x": (lambda lib: route(lib, r=_lib.GEMM_DEQ, M=HUGE_M, n=BIG_N, k=8192, ws=ONE, ws_bytes=BIG_N * 8192 * 2), ESHAPE,
                              b"AMQ_GEMM_DEQ: strides must be multiples of 8 (x) / 4 (y) halves and x, W must each span < 4 GiB"),
    "groups of 64 beyond 4 GiB of x": (lambda lib: route(lib, M=HUGE_M, n=BIG_N, k=8192, group=64, ws=ONE, ws_bytes=BIG_N * 8192 * 2), ESHAPE,
                                       b"AMQ_GEMM_DEQ: strides must be multiples of 8 (x) / 4 (y) halves and x, W must each span < 4 GiB"),
    "gated groups of 64 beyond 4 GiB of x": (lambda lib: gated(lib, M=HUGE_M, n=BIG_N, k=8192, group=64, ws=ONE, ws_bytes=BIG_N * 8192 * 2), ESHAPE,
                                             b"groups of 64 (dequantize-once route): x_stride must be a multiple of 8 halves, N of 4, x and W must each span < 4 GiB"),
    "gated DEQ groups of 32 beyond 4 GiB of x": (lambda lib: gated(lib, r=_lib.GEMM_DEQ, M=HUGE_M, n=BIG_N, k=8192, group=32, ws=ONE, ws_bytes=BIG_N * 8192 * 2), ESHAPE,
                                                 b"groups of 32 (dequantize-once route): x_stride must be a multiple of 8 halves"),
    "gate aliases y, tiled route": (lambda lib: gated(lib, r=_lib.GEMM_TILED, M=300, y=ONE), EINVAL,
                                    b"gate may alias y only where the kernel applies it in its epilogue (amq_gemm_gated_fused)"),
    "gate aliases y, split-K": (lambda lib: gated(lib, M=80, n=BIG_N, k=BIG_K, y=ONE, ws=ONE, ws_bytes=1 << 40), EINVAL, b"gate may alias y only where"),
    "gate aliases y, tiled kernel over groups of 64": (lambda lib: gated(lib, r=_lib.GEMM_TILED, M=40, group=64, y=ONE), EINVAL, b"gate may alias y only where"),
    "res_norm N 192": (lambda lib: res_norm(lib, n=192), ESHAPE, b"the normed rows are handed on in fragment order: N % 128 == 0 (got N=192)"),
    "res_norm null gamma": (lambda lib: res_norm(lib, gamma=None), EINVAL, b"null pointer"),
    "res_norm null xf": (lambda lib: res_norm(lib, xf=None), EINVAL, b"null pointer"),
    "f16w null w": (lambda lib: lib.amq_gemm_f16w_f16(ONE, None, None, None, None, ONE, 40, N, K, 0, 0, None), EINVAL, b"null pointer"),
    "f16w residual and gate": (lambda lib: lib.amq_gemm_f16w_f16(ONE, ONE, None, ONE, ONE, ONE, 40, N, K, 0, 0, None), EINVAL, b"residual and gate are exclusive"),
    "f16w M 0": (lambda lib: lib.amq_gemm_f16w_f16(ONE, ONE, None, None, None, ONE, 0, N, K, 0, 0, None), ESHAPE, b"need M >= 1, N % 16 == 0, K % 128 == 0"),
}
for _g in (64, 32):
    for _r, _n in ((_lib.GEMM_RING, "ring"), (_lib.GEMM_RING128, "ring128"), (_lib.GEMM_WS, "ws")):
        GEMM_RULES["%s route, groups of %d" % (_n, _g)] = (
            lambda lib, _r=_r, _g=_g: route(lib, r=_r, M=300, group=_g), EINVAL, b"groups of %d: the ring / wave-specialised kernels read one (scale, zero) per 128 columns" % _g)
        GEMM_RULES["gated %s route, groups of %d" % (_n, _g)] = (
            lambda lib, _r=_r, _g=_g: gated(lib, r=_r, M=300, group=_g), EINVAL, b"groups of %d: the ring / wave-specialised kernels read one (scale, zero) per 128 columns" % _g)
del _g, _r, _n


@pytest.mark.parametrize("name", sorted(GEMM_RULES))
def test_packed_gemm_rules(name):
    _check(_lib.load(), GEMM_RULES, name)


def test_split_k_sizes_in_the_refusals_are_the_query_s():
    lib = _lib.load()
    need = lib.amq_gemm_route_workspace_bytes(_lib.GEMM_AUTO, 80, BIG_N, BIG_K)
    assert need == lib.amq_gemm_splitk_workspace_bytes(80, BIG_N, BIG_K) and need % (80 * BIG_N * 4) == 0 and need > 80 * BIG_N * 4
    for call in (route, res, res_norm, gated):
        assert call(lib, M=80, n=BIG_N, k=BIG_K, ws=ONE, ws_bytes=need - 1) == EINVAL
        assert b"workspace too small: need %d bytes, got %d" % (need, need - 1) in lib.amq_last_error()
    assert splitk(lib, ws_bytes=need - 1) == EINVAL and b"split-K workspace too small: need %d bytes, got %d" % (need, need - 1) in lib.amq_last_error()


# ---- amq_gemv_route's own refusals ----------------------------------------------------------------------------------------------------
def test_gemv_route_refusals():
    lib = _lib.load()
    i3 = (ctypes.c_int * 5)(3, 3, 3, 3, 3)
    for nseg in (0, 5):
        assert lib.amq_gemv_route(0, 1, 4096, 128, nseg, i3, i3, None) == EINVAL
        assert b"nseg must be 1..4 (got %d), bits and modes non-null" % nseg in lib.amq_last_error()
    assert lib.amq_gemv_route(0, 1, 4096, 128, 1, None, i3, None) == EINVAL and b"bits and modes non-null" in lib.amq_last_error()
    for group in (96, 16, 0, 192):
        assert lib.amq_gemv_route(0, 1, 4096, group, 1, i3, i3, None) == ESHAPE
        assert b"must be 32, 64 or a multiple of 128 (got %d)" % group in lib.amq_last_error()


# ---- the host queries over a grid ------------------------------------------------------------------------------------------------------
QUERY_M = (1, 16, 64, 65, 256, 257, 6144)
QUERY_NK = ((4096, 4096), (13824, 5120))
QUERY_GROUPS = (32, 64, 128, 256)
ROUTE_K = (256, 1408, 2048, 4096, 11008, 16384, 28672)
ROUTE_OPTS = (None, dict(waves=8), dict(waves=16), dict(depth=_lib.GEMV_DEPTH_GENERIC), dict(math=_lib.MATH_GROUPSCALE), dict(dot=1), dict(rpt=2), dict(depth=2))
ROUTE_BITS = ((4,), (3,), (2, 4), (3, 3, 3), (4, 2, 3), (2, 3, 4, 4))


def host_queries(lib):
    """every value of the grid: per query and its arguments but M, the values over QUERY_M (the GEMV route: over ROUTE_BITS x ROUTE_OPTS, as digits)"""
    out = {}
    for r, (n, k), g in itertools.product(ROUTES, QUERY_NK, QUERY_GROUPS):
        out["workspace_bytes_g %d %d %d %d" % (r, n, k, g)] = [int(lib.amq_gemm_route_workspace_bytes_g(r, m, n, k, g)) for m in QUERY_M]
        for use_ws in (0, 1):
            out["gated_fused_g %d %d %d %d %d" % (r, n, k, use_ws, g)] = [int(lib.amq_gemm_gated_fused_g(r, m, n, k, use_ws, g)) for m in QUERY_M]
        if g == 128:
            out["workspace_bytes %d %d %d" % (r, n, k)] = [int(lib.amq_gemm_route_workspace_bytes(r, m, n, k)) for m in QUERY_M]
            out["gated_fused %d %d %d 1" % (r, n, k)] = [int(lib.amq_gemm_gated_fused(r, m, n, k, 1)) for m in QUERY_M]
    for n, k in QUERY_NK:
        out["splitk_workspace_bytes %d %d" % (n, k)] = [int(lib.amq_gemm_splitk_workspace_bytes(m, n, k)) for m in QUERY_M]
    for r in (-1, 7):                                          # outside the domain: 0
        out["workspace_bytes_g %d 4096 4096 128" % r] = [int(lib.amq_gemm_route_workspace_bytes_g(r, m, 4096, 4096, 128)) for m in QUERY_M]
        out["gated_fused_g %d 4096 4096 1 128" % r] = [int(lib.amq_gemm_gated_fused_g(r, m, 4096, 4096, 1, 128)) for m in QUERY_M]
    for r in ROUTES:                                           # no rows
        out["no rows %d" % r] = [int(lib.amq_gemm_route_workspace_bytes_g(r, 0, 4096, 4096, 128)), int(lib.amq_gemm_gated_fused_g(r, 0, 4096, 4096, 1, 128))]
    for pro, m, k, g, mode in itertools.product((0, 1, 2, 4), (1, 2), ROUTE_K, (64, 128, 256), (_lib.MODE_HQQ, _lib.MODE_FMA1)):
        digits = ""
        for bits, o in itertools.product(ROUTE_BITS, ROUTE_OPTS):
            n = len(bits)
            digits += str(lib.amq_gemv_route(pro, m, k, g, n, (ctypes.c_int * n)(*bits), (ctypes.c_int * n)(*([mode] * n)), None if o is None else opts(**o)))
        out["gemv_route %d %d %d %d %d" % (pro, m, k, g, mode)] = digits
    for k in (128, 256, 4096, 5120, 8192, 11008, 13824, 16384, 28672, 65536):
        out["query %d" % k] = _lds_rows(lib, k)
    v = (ctypes.c_int * 6)(*([-7] * 6))
    assert lib.amq_query(4096, v, 3) == 3 and list(v)[3:] == [-7] * 3 and list(v)[:3] == out["query 4096"][:3]
    return out


def test_host_queries_against_the_recorded_values():
    got = host_queries(_lib.load())
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if want[k] != v} == {}


if __name__ == "__main__":         # python tests/test_matmul_entry_cpu.py record: writes the fixture from the library as built
    import sys
    if sys.argv[1:] == ["record"]:
        with open(GOLDEN, "w") as f:
            json.dump(host_queries(_lib.load()), f, indent=0, sort_keys=True, separators=(",", ": "))
            f.write("\n")
