"""CPU-only: the row strides of the fp16 matmul entry points (include/amq_hip.h: x_stride, y_stride, amq_segment.y_stride) are validated on the
host, before any HIP call -- dummy non-null pointers, as in tests/test_abi_cpu.py; no call of this file reaches a launch.

The rule (amq_capi.hip check_strides, written into the header at amq_gemv_f16): a stride is 0 (dense) or at least the row it steps over, never
negative; x_stride % 8 == 0; y_stride % 8 == 0 (amq_gemm_f16w_f16: % 4); where the few-row GEMM kernel can serve the call (M <= 256) strided x
rows span fewer than 2^31 elements.

Every call passes y = NULL, which the entry points look at AFTER the strides: a call whose strides pass is shown to pass by ending as "null
pointer", and a stride the check wrongly let through would end the same way, never as a launch on dummy pointers.  amq_gemm_f16w_f16 looks at
its pointers first: there x spans 8 GiB, which is refused after the strides, with its own message."""
import ctypes

import pytest

from amq_amd import _lib

ESHAPE, EINVAL = -2, -1
N, K = 4096, 4096
ONE = ctypes.c_void_p(256)
ROUTES = (_lib.GEMM_AUTO, _lib.GEMM_TILED, _lib.GEMM_SKINNY, _lib.GEMM_RING, _lib.GEMM_RING128, _lib.GEMM_WS, _lib.GEMM_DEQ)


def _segs(ys, ns=(N, 1024, 1024)):
    return (_lib.Segment * len(ns))(*[_lib.Segment(256, 256, None, None, None, n, 2 + i, 0, s) for i, (n, s) in enumerate(zip(ns, ys))])


def _route(route, m):
    return lambda lib, xs, ys: lib.amq_gemm_route_f16(route, 3, 0, ONE, ONE, ONE, None, ONE, None, m, N, K, 128, xs, ys, ONE, N * K * 2 + 8 * m * N * 4, None)


# name -> (call(lib, x_stride, y_stride), takes x_stride, takes y_stride, y alignment, its M where the few-row GEMM kernel can be given the call)
ENTRIES = {
    "amq_gemv_f16": (lambda lib, xs, ys: lib.amq_gemv_f16(3, 0, ONE, ONE, ONE, None, None, 4, N, K, 128, xs, ys, None), True, True, 8, None),
    "amq_gemv_grouped_f16": (lambda lib, xs, ys: lib.amq_gemv_grouped_f16(_segs((ys, 0, 0)), 3, ONE, ONE, None, 0.0, _lib.PRO_SILU_MUL, 3, K, 128, xs, None, None),
                             True, True, 8, None),
    "amq_gemm_f16": (lambda lib, xs, ys: lib.amq_gemm_f16(3, 0, ONE, ONE, ONE, None, None, 40, N, K, 128, xs, ys, None), True, True, 8, 40),
    "amq_gemm_splitk_f16": (lambda lib, xs, ys: lib.amq_gemm_splitk_f16(3, 0, ONE, ONE, ONE, None, None, 80, N, K, 128, xs, ys, ONE, 8 * 80 * N * 4, None),
                            True, True, 8, 80),
    "amq_gemm_res_f16": (lambda lib, xs, ys: lib.amq_gemm_res_f16(3, 0, ONE, ONE, ONE, None, ONE, None, 40, N, K, 128, xs, ys, None, 0, None), True, True, 8, 40),
    "amq_gemm_gated_f16": (lambda lib, xs, ys: lib.amq_gemm_gated_f16(_lib.GEMM_AUTO, 3, 0, ONE, ONE, ONE, None, ONE, None, 40, N, K, 128, xs, None, 0, None),
                           True, False, 8, 40),
    "amq_gemm_f16w_f16": (lambda lib, xs, ys: lib.amq_gemm_f16w_f16(ONE, ONE, None, ONE, None, ONE, 1 << 20, N, K, xs, ys, None), True, True, 4, None),
    "amq_gemm_xfrag_f16": (lambda lib, xs, ys: lib.amq_gemm_xfrag_f16(3, 0, ONE, ONE, ONE, None, None, ONE, None, 40, N, K, 128, ys, None), False, True, 8, None),
    "amq_gemm_xfrag_grouped_f16": (lambda lib, xs, ys: lib.amq_gemm_xfrag_grouped_f16(_segs((ys, 0, 0)), 3, ONE, 40, K, 128, None), False, True, 8, None),
}
FEWROW_ROUTES = (_lib.GEMM_AUTO, _lib.GEMM_SKINNY)     # the routes that can end in the few-row kernel (amq_gemm.hip gemm_is_skinny; DEQ runs the fp16-weight GEMM or is refused)
for _r in ROUTES:
    _m = 40 if _r == _lib.GEMM_SKINNY else 300
    ENTRIES[f"amq_gemm_route_f16[route {_r}]"] = (_route(_r, _m), True, True, 8, _m if _m <= 256 else None)
    if _r != _lib.GEMM_SKINNY:                             # ... and each route at few rows
        ENTRIES[f"amq_gemm_route_f16[route {_r}, 40 rows]"] = (_route(_r, 40), True, True, 8, 40 if _r in FEWROW_ROUTES else None)
del _r, _m


def _refused(lib, rc, name_of_the_stride):
    msg = lib.amq_last_error()
    assert rc == ESHAPE, (rc, msg)
    assert msg, "a refusal leaves amq_last_error() non-empty"
    assert name_of_the_stride in msg, msg


def _past_the_strides(lib, name, rc):
    """the call got past the stride check: it failed for ANOTHER reason, before any launch"""
    msg = lib.amq_last_error()
    assert b"_stride=" not in msg, (name, msg)
    if name == "amq_gemm_f16w_f16":
        assert rc == ESHAPE and b"4 GiB" in msg, (rc, msg)
    else:
        assert rc == EINVAL and b"null pointer" in msg, (rc, msg)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_strides_shorter_than_the_row_or_negative_are_refused(name):
    lib = _lib.load()
    call, has_x, has_y, _, _ = ENTRIES[name]
    if has_x:
        for xs in (8, K - 8, K - 1, -8, -K, -(1 << 31)):
            _refused(lib, call(lib, xs, 0), b"x_stride=%d" % xs)
    if has_y:
        for ys in (8, N - 8, N - 1, -8, -N, -(1 << 31)):
            _refused(lib, call(lib, 0, ys), b"y_stride=%d" % ys)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_misaligned_strides_are_refused(name):
    """x rows are read in 16-byte pieces everywhere; y and the residual in 16-byte pieces by the split-K reduce (8-byte by the ring, wave-specialised
    and fp16-weight epilogues): x_stride % 8, y_stride % 8 for every packed-weight entry point, y_stride % 4 for amq_gemm_f16w_f16"""
    lib = _lib.load()
    call, has_x, has_y, y_align, _ = ENTRIES[name]
    if has_x:
        for d in (1, 2, 4, 12):
            _refused(lib, call(lib, K + d, 0), b"x_stride=%d" % (K + d))
            assert b"multiple of 8" in lib.amq_last_error()
    if has_y:
        for d in (1, 2, 3, 4, 6, 12):
            rc = call(lib, 0, N + d)
            if d % y_align:
                _refused(lib, rc, b"y_stride=%d" % (N + d))
                assert b"multiple of %d" % y_align in lib.amq_last_error()
            else:
                _past_the_strides(lib, name, rc)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_dense_and_row_length_strides_pass_validation(name):
    lib = _lib.load()
    call, has_x, has_y, _, _ = ENTRIES[name]
    for xs in ((0, K, K + 8, K + 64) if has_x else (0,)):
        for ys in ((0, N, N + 8, N + 24) if has_y else (0,)):
            _past_the_strides(lib, name, call(lib, xs, ys))


@pytest.mark.parametrize("name", sorted(n for n, e in ENTRIES.items() if e[1] and n != "amq_gemm_f16w_f16"))
def test_strided_x_of_the_few_row_kernel_spans_less_than_2_to_31(name):
    """amq_gemm.hip skinny_body forms row * x_stride + column as a 32-bit int: refused where that kernel can be given the call (M <= 256), accepted
    where only the size_t-addressed kernels serve it: more rows, or a forced tiled / ring / wave-specialised route (a ring call that cannot run as
    one goes to the tiled kernel; the dequantize-once route guards its own 4 GiB)"""
    lib = _lib.load()
    call, _, _, _, fewrow_m = ENTRIES[name]
    xs = 1 << 26                                           # 39 rows further on: 39 * 2^26 > 2^31
    if fewrow_m is not None:
        _refused(lib, call(lib, xs, 0), b"x_stride=%d" % xs)
        assert b"2^31" in lib.amq_last_error()
    else:
        _past_the_strides(lib, name, call(lib, xs, 0))


@pytest.mark.parametrize("fn", ["amq_gemv_grouped_f16", "amq_gemv_grouped_sums_f16", "amq_gemm_xfrag_grouped_f16"])
@pytest.mark.parametrize("bad", [8, 1024 - 8, 1024 + 4, -1024])
def test_grouped_calls_check_every_segment(fn, bad):
    lib = _lib.load()

    def call(ys):
        segs = _segs(ys, ns=(1024, 1024, 1024))
        if fn == "amq_gemv_grouped_f16":
            return lib.amq_gemv_grouped_f16(segs, 3, ONE, None, None, 0.0, _lib.PRO_NONE, 3, K, 128, 0, None, None)
        if fn == "amq_gemv_grouped_sums_f16":              # (the 2 .. 8-row partial-sum form takes the same segments: no prologue, no sums written)
            return lib.amq_gemv_grouped_sums_f16(segs, 3, ONE, None, 0.0, None, None, 3, K, 128, None)
        return lib.amq_gemm_xfrag_grouped_f16(segs, 3, ONE, 40, K, 128, None)
    for where in (0, 2):
        ys = [3072, 3072, 3072]                            # the fused q/k/v layout: every segment steps over the whole buffer row
        ys[where] = bad
        _refused(lib, call(ys), b"segment %d" % where)
        assert b"y_stride=%d" % bad in lib.amq_last_error()
    rc = call([3072, 3072, 3072])
    assert rc == EINVAL and b"segment 0: null pointer" in lib.amq_last_error()


def test_existing_refusals_keep_their_codes_and_texts():
    lib = _lib.load()
    # strided x where the rows would only fit LDS in two K phases (tests/test_gpu_kernels.py test_gemv_strided_x_through_the_c_abi)
    rc = lib.amq_gemv_f16(3, 0, ONE, ONE, ONE, None, ONE, 8, 512, 11008, 128, 11008 + 64, 512, None)
    assert rc == ESHAPE and b"(strided x) do not fit LDS" in lib.amq_last_error()
    # the dequantize-once route's own check still speaks for what only it cannot serve: an x of 4 GiB or more
    rc = lib.amq_gemm_route_f16(_lib.GEMM_DEQ, 3, 0, ONE, ONE, ONE, None, None, ONE, 1 << 20, N, 8192, 128, 0, 0, ONE, N * 8192 * 2, None)
    assert rc == ESHAPE and b"AMQ_GEMM_DEQ: strides must be multiples of 8 (x) / 4 (y) halves" in lib.amq_last_error()
    # ... and amq_gemm_f16w_f16's
    rc = lib.amq_gemm_f16w_f16(ONE, ONE, None, None, None, ONE, 512, N, K, K + 4, 0, None)
    assert rc == ESHAPE
    rc = lib.amq_gemm_f16w_f16(ONE, ONE, None, None, None, ONE, 1 << 20, N, 8192, 0, 0, None)
    assert rc == ESHAPE and b"x and W < 4 GiB" in lib.amq_last_error()
