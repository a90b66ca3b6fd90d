"""GPU: the ADDRESSING side of every fp16 matmul entry point -- rows of x taken out of a wider buffer, rows of y (and of the residual) written
into one (include/amq_hip.h: x_stride, y_stride, amq_segment.y_stride), which the Python layer never passes: plain ctypes calls.

Every launch runs on guarded buffers (Guarded below): x and x2 rows carry NaN behind their K columns (a kernel that reads past a row, or finds
row m at m * K, multiplies a NaN in); y lies in an allocation pre-filled with one sentinel bit pattern -- a NaN payload no arithmetic produces --
with a band of 256 elements before row 0 and after the last row; a residual carries NaN in its gaps; workspaces are exactly as large as the
*_workspace_bytes query says, followed by a sentinel band.  Per launch: return code 0; no sentinel left in the live columns; every element outside
them holds its pre-filled bits (compared as uint16); the live columns equal, bit for bit, those of the SAME entry point and route called with
contiguous copies and stride 0; and the strided result stands on its own against x.double() @ W.double().T, W = ops.dequantize (bit-exact:
tests/test_gpu_metadomain.py), within test_gemv_random's bound |y - y64| - 2^-10 |y64| <= 2.5e-4 rms(y64), one more 2^-10 term per further fp16
rounding (bias, residual, gate product) as test_gemm_splitk_matches_single_pass counts them.  Each case runs through the product library and
through the conservative-waits twin (_both: the same bits).

Why bits against the dense call everywhere: at the spans tested the host picks a kernel from (M, N, K, route, options), not from a stride that
passed validation (amq_gemm.hip launch_gemm_nogate; gemm_ring_ok and gemm_f16w_ok ask y_stride % 4 and x_stride % 8, which amq_capi.hip
check_strides guarantees, and that x spans less than 4 GiB, ((M - 1) * x_stride + K) * 2 bytes, amq_gemm_ring.hip:414 / amq_gemm_f16.hip:431 -- a
stride large enough to cross it sends a forced ring / wave-specialised call to the tiled kernel, and every case here stays below 1 MiB;
amq_gemv.hip launch_gemv looks at x_stride only for the two-K-phase form, which no case here reaches), so the same kernel serves both calls; the
per-test docstrings name the selecting line.  The one place where a stride changes the path INSIDE a kernel is the GEMV's x staging
(amq_gemv_body.cuh:984-988): see test_gemv_f16.

Only strides the code serves are launched: multiples of 8 elements (what is refused is tests/test_strided_cpu.py's business, without a launch)."""
import ctypes
import functools

import pytest
import torch

from test_gpu_metadomain import _both, _dev

pytestmark = pytest.mark.gpu

SENT = 0x7E37                   # the sentinel: a quiet NaN with a payload (fp16 arithmetic produces 0x7e00 / 0xfe00)
NAN = 0x7E00
BAND = 256                      # elements before row 0 and after the last row
HQQ, FMA = 0, 1


class Guarded:
    """rows x stride fp16 elements of which the first ``live`` columns of every row are data, inside one allocation with a BAND before and after.
    ``gap`` fills columns live .. stride-1, ``band`` the bands and -- unless ``data`` is given -- the live columns."""

    def __init__(self, rows, live, stride, gap, band, data=None):
        stride = stride or live
        assert stride >= live
        self.rows, self.live, self.stride = rows, live, stride
        self.buf = torch.full((BAND + rows * stride + BAND,), band, dtype=torch.int16, device=_dev())
        self.body = self.buf[BAND:BAND + rows * stride].view(rows, stride)
        self.body[:, live:] = gap
        if data is not None:
            assert tuple(data.shape) == (rows, live) and data.dtype == torch.float16
            self.body[:, :live] = data.to(_dev()).view(torch.int16)
        self.before = self.buf.clone()

    def ptr(self, col=0):
        return ctypes.c_void_p(self.body.data_ptr() + 2 * col)

    def out(self, col=0, n=None):
        n = self.live - col if n is None else n
        return self.body[:, col:col + n].contiguous().view(torch.float16)

    def check(self, what):
        """no sentinel in the live columns; everything else as it was"""
        live = self.body[:, :self.live]
        left = int((live == SENT).sum())
        assert left == 0, f"{what}: {left} of {live.numel()} live outputs still hold the sentinel (never written)"
        now = self.buf.clone()
        now[BAND:BAND + self.rows * self.stride].view(self.rows, self.stride)[:, :self.live] = self.before[BAND:BAND + self.rows * self.stride].view(
            self.rows, self.stride)[:, :self.live]
        bad = torch.nonzero(now != self.before).flatten()
        if bad.numel():
            i = int(bad[0]) - BAND
            pytest.fail(f"{what}: {bad.numel()} elements outside the live columns were written; first at row {i // self.stride}, column {i % self.stride} "
                        f"(live columns 0..{self.live - 1}, stride {self.stride}; negative / beyond the last row: a guard band): "
                        f"0x{int(now[bad[0]]) & 0xffff:04x}, was 0x{int(self.before[bad[0]]) & 0xffff:04x}")


def _xbuf(x, xs):
    """x [M, K] inside [M, xs] with NaN behind every row (xs = 0: dense)"""
    return Guarded(x.shape[0], x.shape[1], xs, NAN, NAN, data=x)


def _ybuf(m, n, ys, inplace=None):
    """y [M, N] inside [M, ys], sentinel everywhere; ``inplace``: the residual's values in the live columns, NaN in the gaps, sentinel in the bands"""
    return Guarded(m, n, ys, SENT if inplace is None else NAN, SENT, data=inplace)


class Workspace:
    """exactly ``nbytes`` bytes, then a sentinel band"""

    def __init__(self, nbytes):
        assert nbytes % 2 == 0
        self.nbytes = nbytes
        self.buf = torch.full((nbytes // 2 + BAND,), SENT, dtype=torch.int16, device=_dev())

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr()) if self.nbytes else None

    def check(self, what):
        assert bool((self.buf[self.nbytes // 2:] == SENT).all()), f"{what}: written behind the {self.nbytes} bytes of its workspace"


def _bits_equal(a, b, what):
    a, b = a.view(torch.int16), b.view(torch.int16)
    if not torch.equal(a, b):
        bad = torch.nonzero(a != b)
        m, n = (int(v) for v in bad[0])
        pytest.fail(f"{what}: {bad.shape[0]} of {a.numel()} outputs differ from the dense call; first at row {m}, column {n}: "
                    f"0x{int(a[m, n]) & 0xffff:04x} vs dense 0x{int(b[m, n]) & 0xffff:04x}")


def _judge(y, y64, adds, what, factor=None):
    """|y - ref| <= 2^-10 |y64| + 2.5e-4 rms(y64) (tests/test_gpu_kernels.py:413) + 2^-10 |partial sum| per further fp16 rounding: ``adds`` are the
    terms added one rounding at a time (bias, residual); ``factor`` (the activated gate, fp16) multiplies the rounded product, one more rounding.
    That last rounding has no rms floor beside it, and a gate near 0 takes the product into fp16's subnormal range, where the rounding step is
    absolute: its error is at most max(2^-11 |v|, 2^-25), so the term for it is 2^-10 |v| + 2^-25 (measured before this was written down: gate
    1.1e-4, product -9.19 * 2^-24, the kernel's -9 * 2^-24 is the correctly rounded value)."""
    rms = y64.pow(2).mean().sqrt()
    acc, tol = y64, 2.0 ** -10 * y64.abs() + 2.5e-4 * rms
    for a in adds:
        acc = acc + a.double()
        tol = tol + 2.0 ** -10 * acc.abs()
    if factor is not None:
        f = factor.double()
        acc, tol = acc * f, tol * f.abs()
        tol = tol + 2.0 ** -10 * acc.abs() + 2.0 ** -25
    err =(y.double() - acc).abs()
    assert torch.isfinite(y.float()).all(), f"{what}: non-finite outputs (a NaN of a gap was read)"
    worst = float((err / tol.clamp_min(1e-30)).max())
    print(f"{what}: worst |y - y64| / bound = {worst:.3f}")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} of {err.numel()} outputs beyond the fp64 bound, worst {worst:.3f} of it"


@functools.lru_cache(maxsize=None)
def _layer(bits, n, k, group=128, mode=HQQ, bias=False, seed=0):
    """random HQQ layer -> native buffers, the fp64 image of the weights the kernels multiply by, bias; computed once, never modified"""
    from amq_amd import ops
    from amq_amd.hqq_format import random_hqq
    h = random_hqq(n, k, bits, seed=1000 * bits + n + k + seed, bias=bias, group=group).to(_dev())
    qn, mn = ops.repack_from_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, n, k, group=group)
    if mode == FMA:                                        # the reference kernels' arithmetic: c = -fp16(zero * scale) (HIPQuantLinear.to_kernel_arithmetic)
        assert group == 128
        mt = mn.clone().view(-1, 2)
        mt[:, 1] = -(mt[:, 1] * mt[:, 0])
        mn = mt.reshape(-1)
    w = ops.dequantize(qn, mn, bits, mode, n, k)
    return dict(qn=qn, mn=mn, w16=w, w64=w.double(), bias=h.bias, bits=bits, mode=mode, n=n, group=group)


def _randn(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.float16).to(_dev())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    from amq_amd import _lib
    return _lib.current_stream()


# --------------------------------------------------------------------------------------------------- one output: strided against dense
def _single(call, L, m, k, xs, ys, what, *, res=None, gate=None, ws_bytes=0, x_of=None, seed=0):
    """call(lib, x, y, res, gate, xs, ys, ws, ws_bytes) -> rc, once on guarded strided buffers and once on dense ones (stride 0).
    res: None, "own" (a strided buffer of its own) or "inplace" (aliased to y); gate: None, "dense" ([M, N] contiguous: amq_gemm_gated_f16) or
    "strided" (y's stride); x_of(x [M, K] dense fp16) -> what the entry point takes as x (fragment order), default: x itself, strided."""
    from amq_amd import _lib, ops
    n = L["n"]
    x = _randn((m, k), 11 + seed + m + k)
    r = _randn((m, n), 12 + seed + m + n) if res else None
    g = _randn((m, n), 13 + seed + m + n) if gate else None

    def fn():
        lib = _lib.load()
        outs = []
        for sx, sy in ((xs, ys), (0, 0)):
            X = _xbuf(x, sx) if x_of is None else None
            xin = None if x_of is None else x_of(x)        # (held until the launch has run)
            xp = X.ptr() if x_of is None else _p(xin)
            Y = _ybuf(m, n, sy, inplace=r if res == "inplace" else None)
            R = Guarded(m, n, sy, NAN, NAN, data=r) if res == "own" else None
            G = Guarded(m, n, sy if gate == "strided" else 0, NAN, NAN, data=g) if gate else None
            W = Workspace(ws_bytes)
            rc = call(lib, xp, Y.ptr(), Y.ptr() if res == "inplace" else R.ptr() if R else None, G.ptr() if G else None, sx, sy, W.ptr(), ws_bytes)
            assert rc == 0, (what, rc, lib.amq_last_error())
            torch.cuda.synchronize()
            tag = f"{what} [{'strided' if (sx, sy) != (0, 0) else 'dense'} xs={sx} ys={sy}]"
            Y.check(tag)
            W.check(tag)
            for side in (X, R, G):
                if side is not None:
                    assert torch.equal(side.buf, side.before), f"{tag}: an input buffer was written"
            outs.append(Y.out())
        _bits_equal(outs[0], outs[1], what)
        return outs[0]
    y = torch.from_numpy(_both(fn)).to(_dev())
    y64 = x.double() @ L["w64"].t()
    adds = ([L["bias"]] if L["bias"] is not None else []) + ([r] if res else [])
    _judge(y, y64, adds, what, factor=ops.silu_mul(g, torch.ones_like(g)) if gate else None)


# --------------------------------------------------------------------------------------------------- amq_gemv_f16
GEMV_N = 144
GEMV_CASES = [(m, k, pair) for k in (512, 4096) for m in (1, 2, 5, 8, 16) if k == 512 or m <= 8 for pair in range(3)]


def _gemv_strides(k, pair):
    return [(k + 8, 0), (0, GEMV_N + 8), (k + 64, GEMV_N + 24)][pair]


def _gemv(L, m, k, xs, ys, what):
    from amq_amd import ops
    assert m <= ops.gemv_max_rows(k), "the GEMV kernel must serve the case"

    def call(lib, x, y, res, gate, sx, sy, ws, wsb):
        return lib.amq_gemv_f16(L["bits"], L["mode"], x, _p(L["qn"]), _p(L["mn"]), _p(L["bias"]), y, m, L["n"], k, L["group"], sx, sy, _stream())
    _single(call, L, m, k, xs, ys, what)


@pytest.mark.parametrize("m,k,pair", GEMV_CASES)
def test_gemv_f16(m, k, pair):
    """3 bit, x / y / both strided, bias on the pair that strides both.  Bits against the dense call: amq_gemv.hip launch_gemv picks the kernel
    (waves, RS = 64 / 128 / 256 row kernels, rows per workgroup) from M, K and the options alone -- K = 512 runs 4 waves and the generic staging for every
    M (amq_gemv.hip:133 `nw != 4`), K = 4096 the row kernels for 2 .. 8 rows.  Inside the row kernels a dense launch stages x by LDS-DMA (xmode 2,
    amq_gemv_body.cuh:984) and a strided one through stage_x (xmode 0, :988); with no prologue both put the SAME fp16 values at the same LDS
    addresses -- a copy, no arithmetic -- and everything behind the staging barrier (the MFMA loop, the cross-wave sum in red[], the epilogue) is the
    one code path of that kernel instance: the fp32 summation order cannot differ, so bits are asserted.  M = 1 reads row 0 only (xmode 1): the
    stride is never used."""
    xs, ys = _gemv_strides(k, pair)
    _gemv(_layer(3, GEMV_N, k, bias=pair == 2), m, k, xs, ys, f"gemv M={m} K={k} xs={xs} ys={ys}")


@pytest.mark.parametrize("bits,mode,group", [(2, HQQ, 128), (4, HQQ, 128), (3, FMA, 128), (3, HQQ, 64)])
def test_gemv_f16_other_widths_arithmetic_and_groups(bits, mode, group):
    """the representative case (5 rows of K = 4096, x and y strided) at 2 and 4 bit, in the reference kernels' arithmetic, and over groups of 64
    (RS = 256 kernels with the generic staging: amq_gemv.hip:128 `plain` needs groups of 128)"""
    k = 4096
    _gemv(_layer(bits, GEMV_N, k, group=group, mode=mode), 5, k, k + 64, GEMV_N + 24, f"gemv {bits} bit mode {mode} group {group}")


# --------------------------------------------------------------------------------------------------- amq_gemv_grouped_f16
SEG_N = (64, 32, 48)
SEG_BITS = (3, 2, 4)


def _grouped(prologue, m, k, xs, gap, what, *, group=128, res_seg=None, res_inplace=False, nseg=3, bits=SEG_BITS, mode=HQQ, keyed=None):
    """three segments of different bit-widths into ONE [M, N0 + N1 + N2 (+ gap)] buffer, segment i at its column offset with y_stride = the buffer's
    width (the fused q/k/v layout); the dense call writes three contiguous [M, N_i] outputs with stride 0.  ``res_seg``: that segment adds a residual
    read at its y_stride -- from a buffer of its own, or (``res_inplace``) aliased to y: the residual's values lie in the segment's columns of the
    fused buffer (NaN in the gaps, the sentinel in the bands and in the other segments' columns), in the dense call in a contiguous y"""
    from amq_amd import _lib, ops
    Ls = [_layer(bits[i], SEG_N[i], k, group=group, mode=mode, seed=i) for i in range(nseg)]
    offs = [sum(SEG_N[:i]) for i in range(nseg)]
    total = sum(SEG_N[:nseg])
    assert m <= ops.gemv_max_rows(k)
    route = ops.gemv_route(prologue, m, k, list(bits[:nseg]), modes=[mode] * nseg, group=group)
    if keyed is not None:
        assert (route == _lib.GEMV_ROUTE_KEYED) == keyed, f"{what}: amq_gemv_route says {route}"
    x = _randn((m, k), 21 + m + k)
    x2 = _randn((m, k), 22 + m + k) if prologue == _lib.PRO_SILU_MUL else None
    gamma = _randn((k,), 23 + k, 0.5) + 1.0 if prologue == _lib.PRO_RMSNORM else None
    r = _randn((m, SEG_N[res_seg]), 24 + m) if res_seg is not None else None
    eps = 1e-5

    def fn():
        lib = _lib.load()
        outs = []
        for strided in (True, False):
            sx = xs if strided else 0
            X, X2 = _xbuf(x, sx), (_xbuf(x2, sx) if x2 is not None else None)
            if strided:
                Y = Guarded(m, total, total + gap, NAN if res_inplace else SENT, SENT)
                if res_inplace:
                    Y.body[:, offs[res_seg]:offs[res_seg] + SEG_N[res_seg]] = r.view(torch.int16)
                    Y.before = Y.buf.clone()
                ys = [Y] * nseg
                ptrs = [Y.ptr(o) for o in offs]
                stride = total + gap
            else:
                ys = [_ybuf(m, SEG_N[i], 0, inplace=r if (res_inplace and i == res_seg) else None) for i in range(nseg)]
                ptrs = [b.ptr() for b in ys]
                stride = 0
            # the residual of one segment: strided like the fused buffer (its rows `stride` apart, NaN between them), or dense; in place: y itself
            R = Guarded(m, SEG_N[res_seg], stride, NAN, NAN, data=r) if (r is not None and not res_inplace) else None
            rptr = None if r is None else ptrs[res_seg].value if res_inplace else R.ptr().value
            segs = (_lib.Segment * nseg)(*[_lib.Segment(Ls[i]["qn"].data_ptr(), Ls[i]["mn"].data_ptr(), None, rptr if i == res_seg else None,
                                                        ptrs[i].value, SEG_N[i], bits[i], mode, stride) for i in range(nseg)])
            rc = lib.amq_gemv_grouped_f16(segs, nseg, X.ptr(), X2.ptr() if X2 else None, _p(gamma), eps, prologue, m, k, group, sx, None, _stream())
            assert rc == 0, (what, rc, lib.amq_last_error())
            torch.cuda.synchronize()
            tag = f"{what} [{'fused buffer' if strided else 'dense'}]"
            for b in set(ys):
                b.check(tag)
            for side in (X, X2, R):
                if side is not None:
                    assert torch.equal(side.buf, side.before), f"{tag}: an input buffer was written"
            outs.append(Y.out() if strided else torch.cat([b.out() for b in ys], dim=1))
        _bits_equal(outs[0], outs[1], what)
        return outs[0]
    y = torch.from_numpy(_both(fn)).to(_dev())
    if prologue == _lib.PRO_SILU_MUL:
        xe = ops.silu_mul(x, x2)                           # the prologue's expression, bit for bit (tests/test_gpu_actdomain.py)
    elif prologue == _lib.PRO_RMSNORM:                     # LlamaRMSNorm: gamma * fp16(x * rsqrt(mean(x^2) + eps))
        xf = x.float()
        xe = gamma * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(torch.float16)
    else:
        xe = x
    for i in range(nseg):
        y64 = xe.double() @ Ls[i]["w64"].t()
        _judge(y[:, offs[i]:offs[i] + SEG_N[i]], y64, [r] if i == res_seg else [], f"{what}, segment {i}")


def test_gemv_grouped_rmsnorm_one_row_keyed():
    """M = 1, K = 4096, RMSNorm prologue, three bit-widths: the keyed kernels (asserted through amq_gemv_route), which run the segments in ascending
    bit-width -- every output must still land in its own segment's columns of the fused buffer.  One row: x_stride is passed and never used; bits
    against the dense call (the same launch but for the y addresses)."""
    from amq_amd import _lib
    _grouped(_lib.PRO_RMSNORM, 1, 4096, 4096 + 8, 8, "grouped RMSNorm M=1", keyed=True)


@pytest.mark.parametrize("group,gap", [(128, 0), (64, 8)])
def test_gemv_grouped_plain_four_rows(group, gap):
    """M = 4, no prologue, K = 2048, groups of 128 (RS = 64 row kernel: dense rows by LDS-DMA, strided rows through stage_x -- a copy either way, same
    bits, see test_gemv_f16) and of 64 (generic staging for both); gap 0: y_stride is exactly N0 + N1 + N2, a row's last segment borders the next row"""
    from amq_amd import _lib
    _grouped(_lib.PRO_NONE, 4, 2048, 2048 + 64, gap, f"grouped plain M=4 group {group}", group=group, keyed=False)


@pytest.mark.parametrize("m", [1, 3])
def test_gemv_grouped_silu_mul_reads_x2_at_x_stride(m):
    """AMQ_PRO_SILU_MUL with x AND x2 strided by x_stride (amq_gemv_body.cuh:190, :233, :508: x2 + row * a.x_stride), NaN behind every row of both.
    M = 3 at K = 2048: the dense call transfers the gate rows by LDS-DMA and multiplies in place (x_finish_dma), the strided call runs stage_x; both
    apply gate_mul element by element -- no sum is involved -- so the staged fp16 values and hence all bits are equal."""
    from amq_amd import _lib
    _grouped(_lib.PRO_SILU_MUL, m, 2048, 2048 + 8, 8, f"grouped SiLU*mul M={m}", keyed=False)


@pytest.mark.parametrize("inplace", [False, True], ids=["own", "inplace"])
@pytest.mark.parametrize("m", [1, 6])
def test_gemv_grouped_residual_at_y_stride(m, inplace):
    """a residual read with its segment's y_stride (amq_gemv_body.cuh:695).  M = 1: one segment, the keyed o_proj form (asserted); M = 6: the middle
    one of three segments, RS = 128 row kernel at K = 2048.  ``inplace``: the residual IS y (h += o_proj(...), what a decode step runs): the
    epilogue's prefetch of the residual a row-tile ahead (:695) and its later plain or SC1 store (:738-740) act on the same strided address, each
    element read and written by the one thread that owns it.  Bits against the dense call: launch_gemv picks the kernel from M, K, the segments and
    the options (amq_gemv.hip:104-139), staging as in test_gemv_f16."""
    from amq_amd import _lib
    if m == 1:
        _grouped(_lib.PRO_NONE, 1, 2048, 2048 + 8, 8, f"o_proj form M=1 inplace={inplace}", res_seg=0, res_inplace=inplace, nseg=1, keyed=True)
    else:
        _grouped(_lib.PRO_NONE, 6, 2048, 2048 + 8, 8, f"grouped residual M=6 inplace={inplace}", res_seg=1, res_inplace=inplace, keyed=False)


def test_gemv_grouped_reference_kernel_arithmetic():
    """M = 4, K = 2048, three segments in the reference kernels' arithmetic (AMQ_MODE_FMA), x and the fused y strided.  Not keyed (asserted: the keyed
    kernels take MODE_HQQ only, amq_gemv.hip:73); RS = 64 row kernel (amq_gemv.hip:133-135), whose dense / strided staging only copies: bits against
    the dense call, as in test_gemv_f16."""
    from amq_amd import _lib
    _grouped(_lib.PRO_NONE, 4, 2048, 2048 + 8, 8, "grouped MODE_FMA M=4", mode=FMA, keyed=False)


# --------------------------------------------------------------------------------------------------- amq_gemm_route_f16 (and _splitk_f16)
ROUTE_SHAPES = {"tiled": (130, 144, 512), "skinny": (17, 48, 384), "splitk": (80, 256, 1024), "ring128": (129, 2048, 256), "ws": (129, 2048, 256),
                "deq": (129, 2048, 256), "ring": (300, 1040, 1152)}
VARIANTS = ("x", "y", "bias_res", "inplace")


def _route_id(family):
    from amq_amd import _lib
    return dict(tiled=_lib.GEMM_TILED, skinny=_lib.GEMM_SKINNY, splitk=_lib.GEMM_AUTO, ring128=_lib.GEMM_RING128, ws=_lib.GEMM_WS, deq=_lib.GEMM_DEQ,
                ring=_lib.GEMM_RING)[family]


def _route_workspace(family, m, n, k, group):
    """the workspace each family's case passes, checked against the project's own predicates for the kernel it means to reach"""
    from amq_amd import _lib
    lib, route = _lib.load(), _route_id(family)
    need = lib.amq_gemm_route_workspace_bytes_g(route, m, n, k, group)
    if family == "splitk":
        assert need > 0 and need == lib.amq_gemm_splitk_workspace_bytes(m, n, k), "the case must split K"
        return need
    if family == "deq":
        assert need == n * k * 2 and lib.amq_gemm_gated_fused_g(route, m, n, k, 1, group) == 1
        return need
    if family in ("ring", "ring128", "ws"):                # (gemm_gate_fused: the ring / wave-specialised kernel takes the launch, gemm_ring_ok included)
        assert need == 0 and lib.amq_gemm_gated_fused(route, m, n, k, 0) == 1
    if family == "skinny":
        assert need == 0 and lib.amq_gemm_gated_fused_g(route, m, n, k, 0, group) == 1
    if family == "tiled":                                  # no workspace passed: ONE pass through gemm_kernel, its own epilogue (amq_gemm.hip:169)
        assert lib.amq_gemm_gated_fused_g(route, m, n, k, 0, group) == 0
    return 0


def _route(family, variant, bits=3, mode=HQQ, group=128, direct_splitk=False):
    m, n, k = ROUTE_SHAPES[family]
    L = _layer(bits, n, k, group=group, mode=mode, bias=variant == "bias_res")
    wsb = _route_workspace(family, m, n, k, group)
    xs, ys = {"x": (k + 8, 0), "y": (0, n + 8), "bias_res": (k + 64, n + 24), "inplace": (k + 8, n + 8)}[variant]
    res = {"bias_res": "own", "inplace": "inplace"}.get(variant)
    route = _route_id(family)

    def call(lib, x, y, r, gate, sx, sy, ws, b):
        if direct_splitk:
            return lib.amq_gemm_splitk_f16(bits, mode, x, _p(L["qn"]), _p(L["mn"]), _p(L["bias"]), y, m, n, k, group, sx, sy, ws, b, _stream())
        return lib.amq_gemm_route_f16(route, bits, mode, x, _p(L["qn"]), _p(L["mn"]), _p(L["bias"]), r, y, m, n, k, group, sx, sy, ws, b, _stream())
    _single(call, L, m, k, xs, ys, f"gemm {family}{' (amq_gemm_splitk_f16)' if direct_splitk else ''} {variant} {bits} bit mode {mode} group {group}",
            res=res, ws_bytes=wsb)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("family", list(ROUTE_SHAPES))
def test_gemm_route_f16(family, variant):
    """every route at 3 bit with strided x, strided y, bias + a strided residual of its own, and the residual in place (aliased to y: NaN in the gaps,
    sentinel in the bands).  The route is the caller's, and _route_workspace asserts with the library's predicates that the kernel meant is the one
    that runs: tiled = gemm_kernel in one pass (x at amq_gemm.hip:77, epilogue :168-169); skinny = skinny_body (:328, :445-449); splitk = AUTO with
    the partials' workspace, gemm_kernel + splitk_reduce_kernel (16-byte residual loads / y stores at :190, :198); ring128 / ring / ws =
    amq_gemm_ring.hip:122, :369, :387 and amq_gemm_ws.hip:108, :402, :420; deq = dequantize into the exactly-sized workspace, then amq_gemm_f16.hip
    (:149, :376, :394).  Same route, same shape, validated strides -> the same kernel as the dense call (amq_gemm.hip launch_gemm_nogate): bits."""
    _route(family, variant)


@pytest.mark.parametrize("variant", ("x", "y", "bias"))
def test_gemm_splitk_f16_direct(variant):
    """amq_gemm_splitk_f16 itself (it has no residual argument): strided x, strided y, and a bias with both strided.  The same two kernels as the AUTO
    split-K case (gemm_kernel + splitk_reduce_kernel, amq_capi.hip amq_gemm_splitk_f16 -> launch_gemm with the partials' workspace): bits."""
    if variant != "bias":
        _route("splitk", variant, direct_splitk=True)
    else:
        m, n, k = ROUTE_SHAPES["splitk"]
        L = _layer(3, n, k, bias=True)
        wsb = _route_workspace("splitk", m, n, k, 128)

        def call(lib, x, y, r, gate, sx, sy, ws, b):
            return lib.amq_gemm_splitk_f16(3, HQQ, x, _p(L["qn"]), _p(L["mn"]), _p(L["bias"]), y, m, n, k, 128, sx, sy, ws, b, _stream())
        _single(call, L, m, k, k + 64, n + 24, "amq_gemm_splitk_f16 bias, x and y strided", ws_bytes=wsb)


@pytest.mark.parametrize("family", ("tiled", "skinny"))
@pytest.mark.parametrize("variant", ("bias_res", "inplace"))
def test_gemm_route_f16_groups_of_64(family, variant):
    """the pair-aware instantiations (GP = 2) of the tiled and the few-row kernel"""
    _route(family, variant, group=64)


@pytest.mark.parametrize("family", list(ROUTE_SHAPES))
@pytest.mark.parametrize("bits,mode", [(2, HQQ), (4, HQQ), (3, FMA)])
def test_gemm_route_f16_other_widths_and_arithmetic(family, bits, mode):
    """every route's representative case (bias + a strided residual of its own, x and y strided) at 2 and 4 bit and in the reference kernels'
    arithmetic (AMQ_MODE_FMA): the BITS / MODE instantiations of the kernels test_gemm_route_f16 names, selected by the same lines
    (amq_gemm.hip launch_gemm_nogate, the predicates asserted in _route_workspace) -- the same kernel as the dense call, so bits."""
    _route(family, "bias_res", bits=bits, mode=mode)


# --------------------------------------------------------------------------------------------------- amq_gemm_gated_f16: x_stride only
@pytest.mark.parametrize("family", ("skinny", "tiled"))
@pytest.mark.parametrize("bits,mode", [(3, HQQ), (2, HQQ), (4, HQQ), (3, FMA)])
def test_gemm_gated_f16_strided_x(family, bits, mode):
    """y and gate are contiguous by contract; x is strided.  skinny: the gate is applied in skinny_body's epilogue (amq_gemm.hip:445); tiled: by the
    element-wise launch behind gemm_kernel (launch_gemm, amq_gemm.hip:804).  y still lies between guard bands."""
    from amq_amd import _lib
    m, n, k = ROUTE_SHAPES[family]
    L = _layer(bits, n, k, mode=mode)
    route = _route_id(family)
    assert _lib.load().amq_gemm_gated_fused(route, m, n, k, 0) == (1 if family == "skinny" else 0)

    def call(lib, x, y, r, gate, sx, sy, ws, b):
        return lib.amq_gemm_gated_f16(route, bits, mode, x, _p(L["qn"]), _p(L["mn"]), None, gate, y, m, n, k, 128, sx, None, 0, _stream())
    _single(call, L, m, k, k + 8, 0, f"gated {family} {bits} bit mode {mode}", gate="dense")


# --------------------------------------------------------------------------------------------------- amq_gemm_f16w_f16
@pytest.mark.parametrize("side", ("residual", "inplace", "gate"))
def test_gemm_f16w_f16(side):
    """dense fp16 weights (the dequantized layer), M = 129, N = 2048, K = 256, x and y strided, with a residual (own buffer / in place) or a gate at
    y's stride (amq_gemm_f16.hip:376 reads either through the same `side` pointer).  One kernel for every call: bits."""
    m, n, k = 129, 2048, 256
    L = _layer(3, n, k)

    def call(lib, x, y, r, gate, sx, sy, ws, b):
        return lib.amq_gemm_f16w_f16(x, _p(L["w16"]), None, r, gate, y, m, n, k, sx, sy, _stream())
    _single(call, L, m, k, k + 8, n + 8, f"f16w {side}", res={"residual": "own", "inplace": "inplace"}.get(side), gate="strided" if side == "gate" else None)


# --------------------------------------------------------------------------------------------------- amq_gemm_xfrag_f16, amq_gemm_xfrag_grouped_f16
def _xf(k):
    from amq_amd import ops
    return lambda x: ops.xfrag(x, x.shape[0], k)


@pytest.mark.parametrize("bits,mode,side", [(3, HQQ, None), (3, HQQ, "own"), (3, HQQ, "inplace"), (3, HQQ, "gate"), (2, HQQ, "own"), (4, HQQ, "own"),
                                            (3, FMA, "own")])
def test_gemm_xfrag_f16_strided_y(bits, mode, side):
    """M = 40, N = 144, K = 384, y_stride = N + 8 (x is fragment-ordered: no stride): skinny_body's XF instantiation, the one kernel of this entry
    point (launch_gemm_xfrag), so bits.  side: a residual of its own (with bias) or in place, read at amq_gemm.hip:448, or a SiLU gate at y's stride
    (NaN in its gaps), read at :445 -- the only caller that runs that load with y_stride != N (amq_gemm_gated_f16 keeps gate and y contiguous)."""
    m, n, k = 40, 144, 384
    L = _layer(bits, n, k, mode=mode, bias=side == "own")

    def call(lib, x, y, r, gate, sx, sy, ws, b):
        return lib.amq_gemm_xfrag_f16(bits, mode, x, _p(L["qn"]), _p(L["mn"]), _p(L["bias"]), gate, r, y, m, n, k, 128, sy, _stream())
    _single(call, L, m, k, 0, n + 8, f"xfrag {bits} bit mode {mode} side {side}", res=side if side in ("own", "inplace") else None,
            gate="strided" if side == "gate" else None, x_of=_xf(k))


@pytest.mark.parametrize("gap", (0, 8))
def test_gemm_xfrag_grouped_f16_fused_buffer(gap):
    """two segments (N = 144 at 3 bit with a residual at its stride, N = 64 at 4 bit) into one [40, 208 (+ 8)] buffer: amq_gemm_fewrow.hip:173-174 and
    the grouped forms (:202, amq_gemm.hip:481) take each segment's own y_stride; dense: two contiguous outputs"""
    from amq_amd import _lib, ops
    m, k, ns, bits = 40, 384, (144, 64), (3, 4)
    Ls = [_layer(bits[i], ns[i], k, seed=i) for i in range(2)]
    offs, total = (0, 144), 208
    x = _randn((m, k), 31)
    r = _randn((m, ns[0]), 32)

    def fn():
        lib = _lib.load()
        xf = ops.xfrag(x, m, k)
        outs = []
        for strided in (True, False):
            stride = total + gap if strided else 0
            if strided:
                Y = _ybuf(m, total, stride)
                ys, ptrs = [Y, Y], [Y.ptr(o) for o in offs]
            else:
                ys = [_ybuf(m, ns[i], 0) for i in range(2)]
                ptrs = [b.ptr() for b in ys]
            R = Guarded(m, ns[0], stride, NAN, NAN, data=r)
            segs = (_lib.Segment * 2)(*[_lib.Segment(Ls[i]["qn"].data_ptr(), Ls[i]["mn"].data_ptr(), None, R.ptr().value if i == 0 else None, ptrs[i].value, ns[i], bits[i],
                                                     HQQ, stride) for i in range(2)])
            rc = lib.amq_gemm_xfrag_grouped_f16(segs, 2, _p(xf), m, k, 128, _stream())
            assert rc == 0, (rc, lib.amq_last_error())
            torch.cuda.synchronize()
            for b in set(ys):
                b.check(f"xfrag grouped gap {gap} [{'fused buffer' if strided else 'dense'}]")
            assert torch.equal(R.buf, R.before)
            outs.append(Y.out() if strided else torch.cat([b.out() for b in ys], dim=1))
        _bits_equal(outs[0], outs[1], f"xfrag grouped gap {gap}")
        return outs[0]
    y = torch.from_numpy(_both(fn)).to(_dev())
    for i in range(2):
        _judge(y[:, offs[i]:offs[i] + ns[i]], x.double() @ Ls[i]["w64"].t(), [r] if i == 0 else [], f"xfrag grouped gap {gap}, segment {i}")
