"""GPU: the activation side of every matmul kernel, read back BIT FOR BIT.  The dual of test_gpu_metadomain.py's one-hot x: a "selection" layer
(codes 1 on a diagonal, 0 elsewhere, scale 1, zero 0 -- exact at 2, 3 and 4 bit in both arithmetics) makes every accumulation hold one non-zero
term, so y[m, n] IS the staged activation x'[m, col(n)], with no rounding of its own; N = K reads every column.  What comes back is held to
tests/actdomain_ref.py: the RMSNorm prologues and SiLU*mul to a band whose width is DERIVED there (RMS_EPS = SILU_EPS = 2^-17 relative on the
first rounding only: the staged half is one of the band's two ends, the second rounding -- gamma * nrm, silu * up -- is exact), the epilogue
(bias, act, residual, gate) exactly.  The GPU tests assert actdomain_ref's caps on the ambiguous share of their own inputs, so a band never
swallows a launch.  Longest summation chain of any staging path: D = 134 additions (stage_x, 16 rows of K = 8192) -> 71 u < 2^-17.

Control first: a PRO_NONE launch over the same layer returns x itself, fp16 subnormals included, on every path judged below.
Every case runs through the product library and the conservative-waits twin (_both).  Each judged launch prints one line: path, ambiguous share,
elements that took the band's far end (differ from RN16 of the fp64 value)."""
import functools

import numpy as np
import pytest
import torch

import actdomain_ref as ref
from test_gpu_metadomain import _both, _dev, _t

pytestmark = pytest.mark.gpu

EPS = ref.NORM_EPS


# ------------------------------------------------------------------------------------------------------------------ layers
@functools.lru_cache(maxsize=None)
def _sel(bits, group, k, n=None, fma=False):
    """selection layer [n, k] (n = k: every column) in native form -> (qn, mn, cols); built once, never modified"""
    from amq_amd import ops
    n = k if n is None else n
    cols = ref.selection_cols(n, k)
    q = ref.selection_codes(n, k, cols)
    if fma:
        qw, sc, zr = ref.gptq_selection(q, bits, group)
        qn, mn = ops.repack_from_gptq(_t(qw), _t(sc), _t(zr), bits, n, k, group=group)
    else:
        wq, s, z = ref.hqq_selection(q, bits, group)
        qn, mn = ops.repack_from_hqq(_t(wq), _t(s), _t(z), bits, n, k, group=group)
    return qn, mn, cols


@functools.lru_cache(maxsize=None)
def _two_hot(bits, k):
    """[k / 2, k]: row i selects columns i and i + k / 2 -- acc = x[i] + x[i + k / 2], exact in fp32 for actdomain_ref.epilogue_case's inputs"""
    from amq_amd import ops
    n = k // 2
    wq, s, z = ref.hqq_selection(ref.selection_codes(n, k, np.arange(n), np.arange(n) + n), bits, 128)
    return ops.repack_from_hqq(_t(wq), _t(s), _t(z), bits, n, k)


def _seg(layer, bits, n, y, fma=False, **kw):
    from amq_amd import ops
    return dict(qn=layer[0], mn=layer[1], bits=bits, mode=ops.MODE_FMA if fma else ops.MODE_HQQ, N=n, y=y, **kw)


def _empty(m, n):
    return torch.empty(m, n, dtype=torch.float16, device=_dev())


def _gemv(x, layer, bits, k, fma=False, seg_kw=None, **kw):
    """one gemv_grouped launch over a selection layer -> y [M, N] (device)"""
    from amq_amd import ops
    n = len(layer[2])
    y = _empty(x.shape[0], n)
    ops.gemv_grouped(x, [_seg(layer, bits, n, y, fma=fma, **(seg_kw or {}))], k, **kw)
    return y


# ------------------------------------------------------------------------------------------------------------------ judging
def _hex(v):
    return f"{float(v)!r} (0x{int(np.asarray(v, np.float16).view(np.uint16)):04x})"


def _judge(y, band, what, classes=None, cols=None, cap=None, inputs=None):
    """y [M, N] must be one of the band's two ends at EVERY element (+0 / -0 equal).  The kernel is not rerun on failure."""
    y = np.asarray(y, np.float16)
    assert y.shape == band.lo.shape, (y.shape, band.lo.shape)
    if cap is not None:
        share = band.amb.reshape(band.amb.shape[0], -1).mean(axis=1) if cap == ref.RMS_AMBIGUOUS_CAP else np.asarray([band.amb.mean()])
        assert (share <= cap).all(), f"{what}: the band leaves {share.max():.4f} of a launch open (cap {cap})"
    ok = band.accepts(y)
    far = int((~ref.same16(y, band.mid) & ok).sum())
    print(f"actdomain | {what} | elements {y.size} | ambiguous {band.amb.mean():.5f} | far end {far} | rejected {int((~ok).sum())}")
    if not ok.all():
        m, j = (int(v) for v in np.argwhere(~ok)[0])
        col = int(cols[j]) if cols is not None else j
        by_row = {int(r): int((~ok[r]).sum()) for r in np.unique(np.argwhere(~ok)[:, 0])}
        cls = ref.X_CLASSES[int(classes[m])] if classes is not None else "-"
        src = f", input {_hex(inputs[m, j])}" if inputs is not None else ""
        pytest.fail(f"{what}: {int((~ok).sum())} of {ok.size} elements outside the band (by row: {by_row}); first at row {m}, column {col}, class {cls}: "
                    f"kernel {_hex(y[m, j])}, band ends {_hex(band.lo[m, j])} / {_hex(band.hi[m, j])}, RN16 of the fp64 value {_hex(band.mid[m, j])}{src}")


def _exact(y, want, what, classes=None, cols=None):
    want = np.asarray(want, np.float16)
    b = ref.Band.__new__(ref.Band)
    b.lo = b.hi = b.mid = want
    b.amb = np.zeros(want.shape, bool)
    _judge(y, b, what, classes, cols)


# ------------------------------------------------------------------------------------------------------------------ GEMV shapes
def _rows_for(rows, k, plain=True):
    """the issue's row counts, held to what the kernel stages at this K (ops.gemv_max_rows)"""
    from amq_amd import ops
    return min(rows, ops.gemv_max_rows(k, plain=plain, norm=True))


# (rows, K, group, math, N or None = K): what launch_gemv (amq_gemv.hip) picks for each --
NORM_CASES = [
    (1, 1024, 128, None, None),      # G = 8 < 16: 4 waves, x_finish, one chunk per thread, half of the lanes idle
    (1, 2048, 128, None, None),      # G = 16: 8 waves, 256 chunks on 512 threads: tail lanes
    (1, 4096, 128, None, None),      # 8 waves, exact fit
    (1, 5120, 128, None, None),      # G = 40 > 32 -> 16 waves, mid_k -> 8 waves with two chunks per thread (second pass part full); K not a power of two: MeanDiv divides
    (1, 11008, 128, None, None),     # 16 waves, XCH = 2
    (1, 28672, 128, None, 4096),     # 16 waves, the four-chunk form; every seventh column, every chunk sampled
    (2, 4096, 128, None, None), (3, 4096, 128, None, None), (4, 4096, 128, None, None),       # RS = 64: x_dma_rows / x_finish_dma, 8 waves
    (2, 5120, 128, None, None), (3, 5120, 128, None, None), (4, 5120, 128, None, None),       # RS = 64 on 16 waves
    (5, 4096, 128, None, None), (8, 4096, 128, None, None),                                   # RS = 128, 8 waves
    (8, 11008, 128, None, None),     # (held to gemv_max_rows(11008, plain, norm) = 6): RS = 128 on 16 waves
    (2, 1024, 128, None, None), (4, 1024, 128, None, None),     # 4 waves: the row kernels do not exist (nw == 4) -> generic stage_x, WPR = 2 / 1 waves per row
    (9, 512, 128, None, None), (16, 512, 128, None, None),      # generic stage_x, 4 waves: three / four rounds of rows
    (9, 4096, 128, None, None), (16, 4096, 128, None, None),    # generic stage_x (16 -> gemv_max_rows(4096) = 15), one wave per row
    (1, 4096, 64, None, None), (4, 4096, 64, None, None),       # groups of 64: GP = 2 bodies, generic staging beyond one row
    (1, 4096, 32, None, None), (4, 4096, 32, None, None),       # groups of 32: GP = 4
    (1, 2048, 128, "linear", None), (4, 2048, 128, "linear", None),     # MATH_LINEAR: x_finish<LIN> / stage_x's row-by-row form with group sums
]
NORM_IDS = [f"m{r}-K{k}-g{g}{'-' + m if m else ''}" for r, k, g, m, _ in NORM_CASES]


def _opts(math):
    from amq_amd import ops
    return ops.GemvOpts(math=ops.MATH_LINEAR) if math == "linear" else None


@pytest.mark.parametrize("bits", (2, 4))
@pytest.mark.parametrize("rows,k,group,math,n", NORM_CASES, ids=NORM_IDS)
def test_gemv_control_then_rmsnorm_prologue(rows, k, group, math, n, bits):
    """per shape: (control) PRO_NONE returns x bit for bit; then PRO_RMSNORM is gamma * fp16(x * rstd) within the band"""
    from amq_amd import ops
    rows = _rows_for(rows, k, plain=(group == 128 and math is None))
    layer = _sel(bits, group, k, n)
    cols = layer[2]
    gamma = ref.gamma_vec(k)
    xs, cs = ref.launches(rows, k)
    gd = _t(gamma)
    for j, (x, cl) in enumerate(zip(xs, cs)):
        xd = _t(x)
        what = f"gemv {rows} rows, K {k}, group {group}, {bits} bit{', linear math' if math else ''}, launch {j}"
        y0 = _both(lambda: _gemv(xd, layer, bits, k, opts=_opts(math)))
        _exact(y0, x[:, cols], "control (PRO_NONE) " + what, cl, cols)
        y = _both(lambda: _gemv(xd, layer, bits, k, prologue=ops.PRO_RMSNORM, gamma=gd, eps=EPS, opts=_opts(math)))
        band = ref.rmsnorm_band(x, gamma)
        assert (band.amb.mean(axis=1) <= ref.RMS_AMBIGUOUS_CAP).all()
        _judge(y, band.take((slice(None), cols)), "RMSNorm prologue " + what, cl, cols, inputs=x[:, cols])


@pytest.mark.parametrize("bits,group,fma", [(3, 128, False), (4, 128, True), (2, 64, True), (3, 32, False)])
def test_control_in_the_other_arithmetic_and_at_3_bit(bits, group, fma):
    """the selection layer is exact at 3 bit and in reference-kernel arithmetic (MODE_FMA) too: x comes back, and so does the normed x"""
    from amq_amd import ops
    k = 1024
    layer = _sel(bits, group, k, None, fma)
    gamma = ref.gamma_vec(k)
    for rows in (1, 4):
        xs, cs = ref.launches(rows, k)
        for j, (x, cl) in enumerate(zip(xs, cs)):
            xd = _t(x)
            what = f"{rows} rows, K {k}, {bits} bit, group {group}, {'FMA' if fma else 'HQQ'}, launch {j}"
            _exact(_both(lambda: _gemv(xd, layer, bits, k, fma=fma)), x, "control " + what, cl)
            y = _both(lambda: _gemv(xd, layer, bits, k, fma=fma, prologue=ops.PRO_RMSNORM, gamma=_t(gamma), eps=EPS))
            _judge(y, ref.rmsnorm_band(x, gamma), "RMSNorm prologue " + what, cl, cap=ref.RMS_AMBIGUOUS_CAP, inputs=x)


# ------------------------------------------------------------------------------------------------------------------ partial sums
@pytest.mark.parametrize("rows,k", [(5, 4096), (8, 4096), (5, 8192), (8, 8192)])
def test_gemv_partial_sums_then_norm_from_them(rows, k):
    """launch A (PRO_NONE + sums_out over the selection layer): y == x and the partials are the per-16-column sums of squares of y -- squares exact,
    row16_total a 4-step tree: (1 + u)^4 - 1 < 4.5 u relative.  Launch B (sums_in + gamma; 5 .. 8-row kernels, RS = 128): the band."""
    from amq_amd import ops
    bits = 2
    rows = min(rows, ops.gemv_max_rows(k, plain=True, norm=True))
    layer = _sel(bits, 128, k)
    gamma = ref.gamma_vec(k)
    xs, cs = ref.launches(rows, k)
    for j, (x, cl) in enumerate(zip(xs, cs)):
        xd = _t(x)
        what = f"{rows} rows, K {k}, launch {j}"
        sums = torch.zeros(rows, k // 16, dtype=torch.float32, device=_dev())

        def launch_a():
            y = _empty(rows, k)
            ops.gemv_grouped_sums(xd, [_seg(layer, bits, k, y)], k, sums_out=sums)
            return y
        _exact(_both(launch_a), x, "control (sums_out launch) " + what, cl)
        want = (ref.f64(x) ** 2).reshape(rows, k // 16, 16).sum(axis=2)
        got = sums.cpu().numpy().astype(np.float64)
        assert (np.abs(got - want) <= 4.5 * 2.0 ** -24 * want).all(), f"partial sums {what}: worst relative error {np.max(np.abs(got - want) / np.maximum(want, 1e-300))}"

        def launch_b():
            y = _empty(rows, k)
            ops.gemv_grouped_sums(xd, [_seg(layer, bits, k, y)], k, gamma=_t(gamma), eps=EPS, sums_in=sums)
            return y
        _judge(_both(launch_b), ref.rmsnorm_band(x, gamma), "RMSNorm from partial sums " + what, cl, cap=ref.RMS_AMBIGUOUS_CAP, inputs=x)


# ------------------------------------------------------------------------------------------------------------------ the other RMSNorm sites
@pytest.mark.parametrize("k", [128, 4096, 5120, 8192])
@pytest.mark.parametrize("rows", [1, 5, 8])
def test_rmsnorm_kernel(rows, k):
    from amq_amd import ops
    gamma = ref.gamma_vec(k)
    xs, cs = ref.launches(rows, k)
    for j, (x, cl) in enumerate(zip(xs, cs)):
        y = _both(lambda: ops.rmsnorm(_t(x), _t(gamma), EPS))
        _judge(y, ref.rmsnorm_band(x, gamma), f"ops.rmsnorm {rows} rows, K {k}, launch {j}", cl, cap=ref.RMS_AMBIGUOUS_CAP, inputs=x)


@pytest.mark.parametrize("rows", [1, 2, 8])
@pytest.mark.parametrize("k", [1024, 4096])
def test_gemv_f16w_with_gamma(k, rows):
    """fp16-weight GEMV (lm_head) with the final norm fused: the identity is just a tensor.  Control: without gamma, x comes back."""
    from amq_amd import ops
    w = torch.eye(k, dtype=torch.float16, device=_dev())
    gamma = ref.gamma_vec(k)
    xs, cs = ref.launches(rows, k)
    for j, (x, cl) in enumerate(zip(xs, cs)):
        xd = _t(x[0] if rows == 1 else x)
        what = f"gemv_f16w {rows} rows, K {k}, launch {j}"
        _exact(_both(lambda: ops.gemv_f16w(xd, w)).reshape(rows, k), x, "control " + what, cl)
        y = _both(lambda: ops.gemv_f16w(xd, w, gamma=_t(gamma), eps=EPS)).reshape(rows, k)
        _judge(y, ref.rmsnorm_band(x, gamma), "RMSNorm " + what, cl, cap=ref.RMS_AMBIGUOUS_CAP, inputs=x)


def test_rmsnorm_xfrag_read_back_through_gemm_xfrag():
    from amq_amd import ops
    k, m, bits = 1024, 16, 4
    layer = _sel(bits, 128, k)
    gamma = ref.gamma_vec(k)
    xs, cs = ref.launches(m, k)
    for j, (x, cl) in enumerate(zip(xs, cs)):
        xd = _t(x)
        _exact(_both(lambda: ops.gemm_xfrag(ops.xfrag(xd, m, k), m, layer[0], layer[1], bits, ops.MODE_HQQ, k, k)), x, f"control gemm_xfrag launch {j}", cl)
        y = _both(lambda: ops.gemm_xfrag(ops.rmsnorm_xfrag(xd, _t(gamma), EPS), m, layer[0], layer[1], bits, ops.MODE_HQQ, k, k))
        _judge(y, ref.rmsnorm_band(x, gamma), f"rmsnorm_xfrag K {k}, launch {j}", cl, cap=ref.RMS_AMBIGUOUS_CAP, inputs=x)


@pytest.mark.parametrize("m,split", [(16, False), (128, True)])
def test_gemm_res_norm_xfrag(m, split):
    """residual + x over the selection layer, then the norm of THAT row in fragment order: 16 rows run the skinny kernel in one pass (rmsnorm_kernel
    behind it), 128 rows the tiled kernel split-K, whose reduce carries the norm (splitk_reduce_norm_kernel)"""
    from amq_amd import ops, _lib
    k, bits = 1024, 4
    assert (_lib.load().amq_gemm_route_workspace_bytes_g(ops.GEMM_AUTO, m, k, k, 128) > 0) == split
    layer = _sel(bits, 128, k)
    gamma = ref.gamma_vec(k)
    xs, cs = ref.launches(16, k)
    x = np.concatenate(xs * (m // 16 // len(xs) + 1))[:m]
    cl = np.concatenate(cs * (m // 16 // len(cs) + 1))[:m]
    res = ref.rn16(np.where(np.abs(ref.f64(x)) > 30000, 0.0, np.random.default_rng(5).standard_normal((m, k))))
    xd, rd = _t(x), _t(res)

    def run():
        y, xf = ops.gemm_res_norm_xfrag(xd, layer[0], layer[1], bits, ops.MODE_HQQ, k, k, _t(gamma), EPS, residual=rd)
        return torch.cat([y, ops.gemm_xfrag(xf, m, layer[0], layer[1], bits, ops.MODE_HQQ, k, k)])
    out = _both(run)
    h = ref.epilogue(ref.f64(x), residual=res).lo
    _exact(out[:m], h, f"gemm_res_norm_xfrag {m} rows: residual + x", cl)
    _judge(out[m:], ref.rmsnorm_band(h, gamma), f"gemm_res_norm_xfrag {m} rows ({'split-K' if split else 'one pass'}): the norm", cl, cap=ref.RMS_AMBIGUOUS_CAP, inputs=h)


# ------------------------------------------------------------------------------------------------------------------ SiLU sites
def test_silu_mul_kernel_over_every_finite_gate():
    from amq_amd import ops
    g = ref.gate_rows(4096)
    one = np.ones_like(g)
    y = _both(lambda: ops.silu_mul(_t(g), _t(one)))
    _judge(y, ref.silu_band(g, one), "ops.silu_mul, all finite gates, up = 1", cap=ref.SILU_AMBIGUOUS_CAP, inputs=g)
    up = ref.up_rows(g.shape[0], 4096, gate=g)
    y = _both(lambda: ops.silu_mul(_t(g), _t(up)))
    _judge(y, ref.silu_band(g, up), "ops.silu_mul, all finite gates, Gaussian up", inputs=g)


# (rows, K, group): one row 8 waves / two chunks / 16 waves; RS = 64 and RS = 128 row kernels; 8 rows of K = 11008 in two K phases; generic 16 rows; fine groups
SILU_CASES = [(1, 4096, 128), (1, 8192, 128), (1, 11008, 128), (4, 4096, 128), (8, 4096, 128), (8, 11008, 128), (16, 1024, 128), (1, 4096, 64), (4, 4096, 32)]


@pytest.mark.parametrize("rows,k,group", SILU_CASES, ids=[f"m{r}-K{k}-g{g}" for r, k, g in SILU_CASES])
def test_gemv_silu_mul_prologue(rows, k, group):
    """PRO_SILU_MUL over the selection layer: every finite gate with up = 1 (dealt to launches of ``rows`` rows of K), then the fixture rows as gates
    with Gaussian up"""
    from amq_amd import ops
    bits = 4
    if (rows, k) == (8, 11008):
        assert ops.gemv_max_rows(k, plain=True, norm=False) == 8 and ops.gemv_max_rows(k, plain=True, norm=True) < 8      # (what selects the phased form)
    layer = _sel(bits, group, k)
    g = ref.gate_rows(k)
    g = np.concatenate([g, np.zeros((-len(g) % rows, k), np.float16)])
    one = np.ones((rows, k), np.float16)
    ys = _both(lambda: torch.cat([_gemv(_t(g[i:i + rows]), layer, bits, k, prologue=ops.PRO_SILU_MUL, x2=_t(one)) for i in range(0, len(g), rows)]))
    _judge(ys, ref.silu_band(g, np.ones_like(g)), f"SiLU*mul prologue, all finite gates, {rows} rows, K {k}, group {group}", cap=ref.SILU_AMBIGUOUS_CAP, inputs=g)
    xs, cs = ref.launches(rows, k)
    for j, (x, cl) in enumerate(zip(xs, cs)):
        up = ref.up_rows(rows, k, seed=j, gate=x)
        y = _both(lambda: _gemv(_t(x), layer, bits, k, prologue=ops.PRO_SILU_MUL, x2=_t(up)))
        _judge(y, ref.silu_band(x, up), f"SiLU*mul prologue, fixture gates, {rows} rows, K {k}, group {group}, launch {j}", cl, inputs=x)


@pytest.mark.parametrize("rows", [1, 4, 8])
def test_activated_segment_then_multiply_only_prologue(rows):
    """act=True over the selection layer: y = fp16(silu(x)); then x_activated=True (PRO_MUL) with up: the bits of SiLU*mul on the plain gate, and
    the restatement's"""
    from amq_amd import ops
    k, bits = 4096, 4
    layer = _sel(bits, 128, k)
    g = ref.gate_rows(k)
    assert len(g) % rows == 0
    up = ref.up_rows(len(g), k, gate=g)
    for i in range(0, len(g), rows):
        gd, ud = _t(g[i:i + rows]), _t(up[i:i + rows])
        act = _both(lambda: _gemv(gd, layer, bits, k, seg_kw=dict(act=True)))
        _judge(act, ref.silu_band(g[i:i + rows]), f"act segment, {rows} rows, gates {i}..", inputs=g[i:i + rows])
        y_mul = _both(lambda: _gemv(_t(act), layer, bits, k, prologue=ops.PRO_SILU_MUL, x2=ud, x_activated=True))
        y_old = _both(lambda: _gemv(gd, layer, bits, k, prologue=ops.PRO_SILU_MUL, x2=ud))
        assert ref.same16(y_mul, y_old).all(), f"PRO_MUL over the activated gate differs from SiLU*mul, {rows} rows, gates {i}.."
        _judge(y_mul, ref.silu_band(g[i:i + rows], up[i:i + rows]), f"act + PRO_MUL, {rows} rows, gates {i}..", inputs=g[i:i + rows])


# every route that amq_gemm_gated_fused_g reports as fused at these sizes (the tiled kernel does not apply the gate itself: asserted below), the
# fragment-ordered few-row kernel and the fp16-weight GEMM.  (ring: GEMM_RING picks its tile rows itself -- 128-row tiles at this size; the 256-row
# tiles need a launch of ~10 M outputs, test_gpu_metadomain.py's ring case.)
GATED = ["skinny", "ring", "ring128", "ws", "deq", "auto", "xfrag", "f16w"]


@pytest.mark.parametrize("family", GATED)
def test_gated_gemm(family):
    """y = fp16(silu(gate)) * fp16(x . W^T) with W the selection layer: ``up`` is x, known exactly.  Every finite gate (124 rows of 512, padded)."""
    from amq_amd import ops, _lib
    k, bits = 512, 4
    layer = _sel(bits, 128, k)
    g = ref.gate_rows(k)
    m = {"skinny": 64, "xfrag": 64, "auto": 64}.get(family, 128)
    g = np.concatenate([g, np.zeros((-len(g) % m, k), np.float16)])
    up = ref.up_rows(len(g), k, gate=g)
    routes = dict(skinny=ops.GEMM_SKINNY, ring=ops.GEMM_RING, ring128=ops.GEMM_RING128, ws=ops.GEMM_WS, deq=ops.GEMM_DEQ, auto=ops.GEMM_AUTO)
    lib = _lib.load()
    for mm in (64, 128):
        need = lib.amq_gemm_route_workspace_bytes_g(ops.GEMM_TILED, mm, k, k, 128)
        assert not lib.amq_gemm_gated_fused_g(ops.GEMM_TILED, mm, k, k, 1 if need else 0, 128), "the tiled route applies the gate now: add it to GATED"
    if family in routes:
        need = lib.amq_gemm_route_workspace_bytes_g(routes[family], m, k, k, 128)
        assert lib.amq_gemm_gated_fused_g(routes[family], m, k, k, 1 if need else 0, 128), "this route no longer applies the gate itself"
    w16 = torch.eye(k, dtype=torch.float16, device=_dev())

    def one(gd, ud):
        if family == "xfrag":
            return ops.gemm_xfrag(ops.xfrag(ud, m, k), m, layer[0], layer[1], bits, ops.MODE_HQQ, k, k, gate=gd)
        if family == "f16w":
            return ops.gemm_f16w(ud, w16, gate=gd)
        return ops.gemm(ud, layer[0], layer[1], bits, ops.MODE_HQQ, k, k, gate=gd, route=routes[family])
    y = _both(lambda: torch.cat([one(_t(g[i:i + m]), _t(up[i:i + m])) for i in range(0, len(g), m)]))
    _judge(y, ref.silu_band(g, up), f"gated GEMM, {family}", cap=ref.SILU_AMBIGUOUS_CAP, inputs=g)


# ------------------------------------------------------------------------------------------------------------------ epilogue order
EPI_K = 512


def _epi_inputs(m, k=EPI_K):
    c = ref.epilogue_case(m, k // 2)
    single = ref.mutant_epilogue_single_rounding(c["acc"], c["bias"], c["residual"])
    want = ref.epilogue(c["acc"], c["bias"], c["residual"]).lo
    share = (~ref.same16(single, want)).mean()
    assert share >= 0.20, share            # a single rounding of acc + bias + residual differs on this share of THESE inputs (~0.4)
    return c, np.concatenate([c["xa"], c["xb"]], axis=1)


@pytest.mark.parametrize("rows", [1, 4, 8, 16])
def test_gemv_epilogue_order(rows):
    """GEMV with bias, residual and both over the two-hot layer (acc = xa + xb: not an fp16 value): fp16(acc), + bias, residual +, each its own
    rounding, every element exact; row 0 overflows to inf in the bias add"""
    from amq_amd import ops
    bits = 4
    EPI_N = EPI_K // 2
    qn, mn = _two_hot(bits, EPI_K)
    c, x = _epi_inputs(rows)
    for use_b, use_r in ((True, False), (False, True), (True, True)):
        b, r = (c["bias"] if use_b else None), (c["residual"] if use_r else None)

        def run():
            y = _empty(rows, EPI_N)
            ops.gemv_grouped(_t(x), [dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=EPI_N, y=y, bias=None if b is None else _t(b),
                                           residual=None if r is None else _t(r))], EPI_K)
            return y
        y = _both(run)
        _exact(y, ref.epilogue(c["acc"], b, r).lo, f"gemv epilogue, {rows} rows, bias {use_b}, residual {use_r}")
        if use_b:
            assert np.isinf(y[0].astype(np.float32)).any()
    # bias, then act: fp16(silu(fp16(fp16(acc) + bias))) -- SiLU's band on an exactly known argument (the overflowing row left out: non-finite gates are
    # out of scope)
    c2 = ref.epilogue_case(rows + 1, EPI_N, seed=1)
    x2 = np.concatenate([c2["xa"], c2["xb"]], axis=1)[1:]

    def run_act():
        y = _empty(rows, EPI_N)
        ops.gemv_grouped(_t(x2), [dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=EPI_N, y=y, bias=_t(c2["bias"]), act=True)], EPI_K)
        return y
    _judge(_both(run_act), ref.epilogue(c2["acc"][1:], c2["bias"], act=True), f"gemv epilogue, {rows} rows, bias then act")


EPI_FAMILIES = ["tiled", "splitk", "skinny", "ring", "ring128", "ws", "deq", "xfrag", "xfrag_grouped", "f16w"]


@pytest.mark.parametrize("family", EPI_FAMILIES)
def test_gemm_epilogue_order(family):
    """the same probe through every GEMM route that owns an epilogue: tiled in one pass and split-K (splitk_reduce_kernel), skinny, ring (128-row
    tiles at this size), ring128, wave-specialised, dequantize-once, the fragment-ordered few-row kernel alone and as a grouped launch, the
    fp16-weight GEMM"""
    from amq_amd import ops, _lib
    bits = 4
    lib = _lib.load()
    m = {"tiled": 64, "splitk": 64, "skinny": 64, "xfrag": 64, "xfrag_grouped": 64}.get(family, 128)
    EPI_K = 256 if family == "tiled" else 512       # (two tiles of K: gemm_pick_splits keeps such a launch in one pass)
    EPI_N = EPI_K // 2
    qn, mn = _two_hot(bits, EPI_K)
    c, x = _epi_inputs(m, EPI_K)
    routes = dict(tiled=ops.GEMM_TILED, splitk=ops.GEMM_TILED, skinny=ops.GEMM_SKINNY, ring=ops.GEMM_RING, ring128=ops.GEMM_RING128, ws=ops.GEMM_WS, deq=ops.GEMM_DEQ)
    if family in ("tiled", "splitk"):           # (split-K: the partials go through splitk_reduce_kernel, which owns the epilogue)
        assert (lib.amq_gemm_route_workspace_bytes_g(ops.GEMM_TILED, m, EPI_N, EPI_K, 128) > 0) == (family == "splitk")
    w16 = _t(ref.selection_codes(EPI_N, EPI_K, np.arange(EPI_N), np.arange(EPI_N) + EPI_N).astype(np.float16))
    for use_b, use_r in ((True, False), (False, True), (True, True)):
        b, r = (c["bias"] if use_b else None), (c["residual"] if use_r else None)
        bd, rd = (None if b is None else _t(b)), (None if r is None else _t(r))

        def run():
            if family == "xfrag":
                return ops.gemm_xfrag(ops.xfrag(_t(x), m, EPI_K), m, qn, mn, bits, ops.MODE_HQQ, EPI_N, EPI_K, bias=bd, residual=rd)
            if family == "xfrag_grouped":
                y = _empty(m, EPI_N)
                ops.gemm_xfrag_grouped(ops.xfrag(_t(x), m, EPI_K), m, [dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=EPI_N, y=y, bias=bd, residual=rd)], EPI_K)
                return y
            if family == "f16w":
                return ops.gemm_f16w(_t(x), w16, bias=bd, residual=rd)
            return ops.gemm(_t(x), qn, mn, bits, ops.MODE_HQQ, EPI_N, EPI_K, bias=bd, residual=rd, route=routes[family])
        _exact(_both(run), ref.epilogue(c["acc"], b, r).lo, f"gemm epilogue, {family}, {m} rows, bias {use_b}, residual {use_r}")
