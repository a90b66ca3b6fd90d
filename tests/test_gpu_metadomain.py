"""GPU: the weights every matmul kernel family actually multiplies by, recovered with one-hot x rows (row m of x is 1.0 at column k_m: y[m, :] is
column k_m of W -- one product, exact in fp32, rounded to the fp16 value it already is), held BIT FOR BIT to the restatement of the arithmetic
amq_common.cuh documents (tests/metadomain_ref.py; its distance from the reference is tests/test_metadomain_cpu.py's business) at every
element, over fixture layers whose (scale, zero) span the fp16 range: negative zero points, zero points beyond the code range, +-0, zero points
next to rounding ties, subnormal, huge and negative scales -- all mixed inside every 16-row tile.  Every case runs through the product library and
through the conservative-waits twin."""
import functools

import numpy as np
import pytest
import torch

import metadomain_ref as ref
from oracle import gptq_ref, hqq_ref

pytestmark = pytest.mark.gpu

BITS = (2, 3, 4)
GROUPS = (128, 64, 32)
N, K = 144, 512                 # GEMM probes: one full 128-column tile plus a ragged 16, x = I_512
NV = 64                         # GEMV probes
MODE_NAMES = {0: "HQQ", 1: "FMA", 2: "FMA1"}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@functools.lru_cache(maxsize=None)
def _twin():
    from amq_amd import _lib
    return _lib.open_twin()


def _both(fn):
    """fn() through the product library and through the conservative-waits twin: the same bits; -> numpy"""
    from amq_amd import _lib
    y = fn()
    with _lib.routed_to(_twin()):
        y2 = fn()
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), "the conservative-waits twin computes other bits"
    return y.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _fixture(bits, group, n, k, fma1=False):
    """layer + native buffers (HQQ and reference-kernel arithmetic) + the expected weights per arithmetic; computed once, never modified"""
    from amq_amd import ops
    L = ref.make_layer(bits, group, n, k, fma1=fma1)
    wq, s, z = ref.hqq_buffers(L)
    qw, sc, zr = ref.gptq_buffers(L)
    f = dict(L=L, hqq=ops.repack_from_hqq(_t(wq), _t(s.reshape(-1)), _t(z.reshape(-1)), bits, n, k, group=group),
             fma=ops.repack_from_gptq(_t(qw), _t(sc), _t(zr), bits, n, k, group=group))
    assert torch.equal(f["hqq"][0], f["fma"][0])                      # one payload, two metas
    q = L["q"]
    f["oracle_hqq"] = hqq_ref.dequantize(wq, s, z, bits, (n, k), group_size=group)
    f["oracle_fma"] = np.asarray(gptq_ref.dequant_kernel(qw, sc, zr, bits, group_size=group), np.float16)
    f["exact"] = {0: ref.hqq_exact(q, L["scale"], L["zero"], bits, group), 1: ref.fma_exact(q, L["scale"], L["c"], bits, group)}
    f["exact"][2] = ref.fma1_exact(q, L["scale"], L["c"], bits, group) if fma1 else f["exact"][1]
    f["gs"] = ref.gs_weight(q, L["scale"], L["zero"], group)
    f["linear"] = {0: ref.linear_weight(q, L["scale"], L["zero"], group, False), 1: ref.linear_weight(q, L["scale"], L["c"], group, True)}
    f["linear"][2] = f["linear"][1]
    for w in (f["oracle_hqq"], f["oracle_fma"], f["exact"][0], f["exact"][1], f["exact"][2], f["gs"], f["linear"][0], f["linear"][1]):
        assert np.isfinite(w.astype(np.float64)).all()                # no 0 * inf in a one-hot product
    return f


def _native(f, mode):
    return f["hqq"] if mode == 0 else f["fma"]


def _onehot(cols, k):
    x = torch.zeros(len(cols), k, dtype=torch.float16)
    x[torch.arange(len(cols)), torch.as_tensor(np.asarray(cols), dtype=torch.long)] = 1.0
    return x.to(_dev())


def _check(y, want, L, cols, what):
    """y [M, N]: row i must be column cols[i] of ``want`` [N, K], bit for bit (+0 / -0 equal) at EVERY element"""
    y = np.asarray(y, np.float16)
    w = np.ascontiguousarray(np.asarray(want, np.float16)[:, np.asarray(cols)].T)
    assert y.shape == w.shape, (y.shape, w.shape)
    bad = (y.view(np.uint16) != w.view(np.uint16)) & ~((y == 0) & (w == 0))
    if bad.any():
        i, n = (int(v) for v in np.argwhere(bad)[0])
        kk = int(cols[i])
        g = kk // L["group"]
        pos = kk % 128
        counts = {}
        cls_of = L["cls"][:, np.asarray(cols) // L["group"]].T              # [M, N]
        for c in np.unique(cls_of[bad]):
            counts[ref.CLASSES[int(c)]] = int((bad & (cls_of == c)).sum())
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} weights differ (by class: {counts}); first at row n = {n}, k = {kk} (position {pos}, "
                    f"lane pair {4 * (pos // 32) + (pos % 8) // 2}, class {ref.CLASSES[int(L['cls'][n, g])]}): kernel {float(y[i, n])!r} (0x{int(y.view(np.uint16)[i, n]):04x}), "
                    f"restatement {float(w[i, n])!r} (0x{int(w.view(np.uint16)[i, n]):04x}); q = {int(L['q'][n, kk])}, scale = {float(L['scale'][n, g])!r}, "
                    f"zero = {float(L['zero'][n, g])!r}, c = {float(L['c'][n, g])!r}")


# ------------------------------------------------------------------------------------------------------------- the other unpack: dequantize
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("bits", BITS)
def test_dequantize_equals_the_oracle_on_every_class(bits, group):
    """ops.dequantize / ops.dequantize_hqq (magic-number unpack, the reference's two roundings as written): the oracle bit for bit, no mask"""
    from amq_amd import ops
    f = _fixture(bits, group, N, K)
    L = f["L"]
    cols = np.arange(K)
    for mode in (0, 1, 2):
        qn, mn = _native(f, mode)
        w = _both(lambda: ops.dequantize(qn, mn, bits, mode, N, K))
        _check(w.T, f["oracle_hqq"] if mode == 0 else f["oracle_fma"], L, cols, f"dequantize {bits} bit group {group} mode {MODE_NAMES[mode]}")
    wq, s, z = ref.hqq_buffers(L)
    w = _both(lambda: ops.dequantize_hqq(_t(wq), _t(s.reshape(-1)), _t(z.reshape(-1)), bits, N, K, group=group))
    _check(w.T, f["oracle_hqq"], L, cols, f"dequantize_hqq {bits} bit group {group}")


# ------------------------------------------------------------------------------------------------------------- GEMM families, x = I_512
def _slices(fn):
    """the few-row kernels: 64 one-hot rows per launch"""
    eye = torch.eye(K, dtype=torch.float16, device=_dev())
    return torch.cat([fn(eye[i:i + 64].contiguous()) for i in range(0, K, 64)])


RING_N, RING_REPS = 1040, 19     # the ring kernel's 256-row tiles: see _ring256_is_chosen


def _ring256_is_chosen(m, n):
    """GEMM_RING picks its tile rows itself (amq_gemm_ring.hip gemm_ring_rows): 256 where at least 150 such tiles score no worse than the 128-row
    ones by their last-round fill, else 128 -- which GEMM_RING128 forces anyway.  The smallest launch that takes the 256-row tiles is ~10 M outputs:
    I_512 stacked 19 times against N = 1040 (four full 256-column tiles and a ragged 16)."""
    slots = torch.cuda.get_device_properties(0).multi_processor_count
    nt = -(-n // 256)
    t256, t128 = -(-m // 256) * nt, -(-m // 128) * nt

    def fill(t):
        return t / (slots * -(-t // slots))
    return t256 >= 150 and fill(t256) >= 0.85 * fill(t128)


def _run_gemm(family, qn, mn, bits, mode):
    from amq_amd import ops, _lib
    routes = dict(tiled=ops.GEMM_TILED, ring128=ops.GEMM_RING128, ws=ops.GEMM_WS, deq=ops.GEMM_DEQ)
    if family in routes:
        return ops.gemm(torch.eye(K, dtype=torch.float16, device=_dev()), qn, mn, bits, mode, N, K, route=routes[family])
    if family == "ring":
        assert _ring256_is_chosen(RING_REPS * K, RING_N)
        y = ops.gemm(torch.eye(K, dtype=torch.float16, device=_dev()).repeat(RING_REPS, 1), qn, mn, bits, mode, RING_N, K, route=ops.GEMM_RING)
        assert torch.equal(y.view(torch.int16).view(RING_REPS, K, RING_N), y[:K].view(torch.int16).expand(RING_REPS, K, RING_N))       # every copy of I_512 recovers the same weights
        return y[:K]
    if family == "skinny":
        return _slices(lambda x: ops.gemm(x, qn, mn, bits, mode, N, K, route=ops.GEMM_SKINNY))
    if family == "xfrag":
        return _slices(lambda x: ops.gemm_xfrag(ops.xfrag(x, 64, K), 64, qn, mn, bits, mode, N, K))
    form, blocks = {"xfrag_tile": (_lib.FEWROW_TILE, 0), "xfrag_stream3": (_lib.FEWROW_STREAM, 3), "xfrag_stream1": (_lib.FEWROW_STREAM, 1)}[family]

    def grouped(x):
        y = torch.empty(64, N, dtype=torch.float16, device=_dev())
        ops.gemm_xfrag_grouped(ops.xfrag(x, 64, K), 64, [dict(qn=qn, mn=mn, bits=bits, mode=mode, N=N, y=y)], K, form=form, blocks_per_wg=blocks)
        return y
    return _slices(grouped)


GEMM_FAMILIES = ("tiled", "skinny", "ring", "ring128", "ws", "deq", "xfrag", "xfrag_tile", "xfrag_stream3", "xfrag_stream1")
FINE_FAMILIES = ("tiled", "skinny", "deq")      # the routes that serve groups of 64 / 32


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("family,group", [(fam, 128) for fam in GEMM_FAMILIES] + [(fam, g) for g in (64, 32) for fam in FINE_FAMILIES])
def test_gemm_family_weights(family, group, bits):
    """every GEMM kernel family (ring: 256-row tiles, ring128: 128-row tiles), modes HQQ / FMA / FMA1 (these kernels run FMA1 as FMA).  The dequantize-once route multiplies by the OTHER
    unpack's weights: the oracle's, on every class."""
    f = _fixture(bits, group, RING_N if family == "ring" else N, K)
    cols = np.arange(K)
    for mode in (0, 1, 2):
        qn, mn = _native(f, mode)
        y = _both(lambda: _run_gemm(family, qn, mn, bits, mode))
        want = (f["oracle_hqq"] if mode == 0 else f["oracle_fma"]) if family == "deq" else f["exact"][min(mode, 1)]
        _check(y, want, f["L"], cols, f"gemm family {family}, {bits} bit, group {group}, mode {MODE_NAMES[mode]}")


@pytest.mark.parametrize("group", (64, 32))
def test_gemm_families_that_read_one_pair_per_tile_refuse_finer_groups(group):
    from amq_amd import ops
    f = _fixture(3, group, N, K)
    qn, mn = f["hqq"]
    eye = torch.eye(K, dtype=torch.float16, device=_dev())
    for route in (ops.GEMM_RING, ops.GEMM_RING128, ops.GEMM_WS):
        with pytest.raises(Exception, match="dequantize-once"):
            ops.gemm(eye, qn, mn, 3, ops.MODE_HQQ, N, K, route=route)
    xf = ops.xfrag(eye[:64].contiguous(), 64, K)
    with pytest.raises(ValueError, match="groups of 128"):
        ops.gemm_xfrag(xf, 64, qn, mn, 3, ops.MODE_HQQ, N, K)
    with pytest.raises(ValueError, match="groups of 128"):
        ops.gemm_xfrag_grouped(xf, 64, [dict(qn=qn, mn=mn, bits=3, mode=ops.MODE_HQQ, N=N, y=torch.empty(64, N, dtype=torch.float16, device=_dev()))], K)
    with pytest.raises(Exception, match="default form"):
        ops.gemv(eye[:1].contiguous(), qn, mn, 3, ops.MODE_HQQ, N, K, opts=ops.GemvOpts(math=ops.MATH_LINEAR))


# ------------------------------------------------------------------------------------------------------------- GEMV families
def _probe_cols(k, rows):
    """128 probes: probe i reads position i of group i mod K / 128 -- every position of a group and (K <= 16384) every group; dealt to launches of
    ``rows`` one-hot rows (the last launch wraps around)"""
    g = k // 128
    idx = np.arange(-(-128 // rows) * rows) % 128
    return (idx + 128 * (idx % g)).reshape(-1, rows)


def _run_gemv(launches, k, qn, mn, bits, mode, n, opts):
    from amq_amd import ops
    return torch.cat([ops.gemv(_onehot(c, k), qn, mn, bits, mode, n, k, opts=opts) for c in launches])


GEMV_SHAPES = [(1, 512), (2, 512), (4, 512), (5, 512), (8, 512), (16, 512), (1, 8192), (2, 8192), (4, 8192), (5, 8192), (8, 8192)]


# (groups of 64 / 32 keep the generic staging, whose larger cross-wave buffer leaves room for 7 rows of K = 8192, not 8)
GEMV_CASES = [(r, k, 128) for r, k in GEMV_SHAPES] + [(7 if (r, k) == (8, 8192) else r, k, g) for g in (64, 32) for r, k in GEMV_SHAPES]


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("rows,k,group", GEMV_CASES)
def test_gemv_exact_weights(rows, k, group, bits):
    """MATH_EXACT: the one-row kernel (K = 512: 4 waves; K = 8192: 8 waves, two x chunks per thread), 2 - 4 / 5 - 8 rows (K = 8192: the RS = 64 /
    128 LDS-DMA kernels on 16 waves; K = 512 and the finer groups: the generic staging), 16 rows (generic); groups of 64 / 32: the GP = 2 / 4
    bodies.  MODE_FMA1 runs the one-op unpack on a layer within its scale bound (groups of 128; finer groups run it as MODE_FMA)."""
    from amq_amd import ops
    launches = _probe_cols(k, rows)
    opts = ops.GemvOpts(math=ops.MATH_EXACT)
    for mode in (0, 1, 2):
        f = _fixture(bits, group, NV, k, fma1=(mode == 2))
        qn, mn = _native(f, mode)
        if mode == 2 and group == 128:
            assert ops.fma_mode_for(mn, bits) == ops.MODE_FMA1
        y = _both(lambda: _run_gemv(launches, k, qn, mn, bits, mode, NV, opts))
        _check(y, f["exact"][mode], f["L"], launches.reshape(-1), f"gemv exact, {rows} rows, K {k}, {bits} bit, group {group}, mode {MODE_NAMES[mode]}")


@pytest.mark.parametrize("bits", BITS)
def test_gemv_two_k_phases_weights(bits):
    """8 rows of K = 11008 (x does not fit LDS whole: staged in two K phases, boundary at group 43).  16 launches, 128 probes: every position, the
    first and the last group, both sides of the phase boundary including its two edge columns"""
    from amq_amd import ops
    k, g = 11008, 86
    assert ops.gemv_max_rows(k, plain=True, norm=False) == 8 and ops.gemv_max_rows(k, plain=True, norm=True) < 8      # (what selects the phased form)
    idx = np.arange(128)
    grp = np.where(idx % 5 == 0, 0, np.where(idx % 5 == 1, g // 2 - 1, np.where(idx % 5 == 2, g // 2, np.where(idx % 5 == 3, g - 1, (11 * idx) % g))))
    grp[127], grp[0], grp[1] = g // 2 - 1, g // 2, 0            # columns 5503 | 5504: the last of phase 0, the first of phase 1
    cols = idx + 128 * grp
    assert {0, g // 2 - 1, g // 2, g - 1} <= set(grp.tolist()) and k // 2 - 1 in cols and k // 2 in cols and len(set(cols % 128)) == 128
    launches = cols.reshape(16, 8)
    opts = ops.GemvOpts(math=ops.MATH_EXACT)
    for mode in (0, 1, 2):
        f = _fixture(bits, 128, NV, k, fma1=(mode == 2))
        qn, mn = _native(f, mode)
        y = _both(lambda: _run_gemv(launches, k, qn, mn, bits, mode, NV, opts))
        _check(y, f["exact"][mode], f["L"], cols, f"gemv two K phases, 8 rows, K {k}, {bits} bit, mode {MODE_NAMES[mode]}")


@pytest.mark.parametrize("group", (128, 64))
def test_gemv_grouped_segments_keep_their_own_meta(group):
    """one launch, three segments of different bit-widths and modes over the same one-hot rows: no segment sees another's scale / zero"""
    from amq_amd import ops
    k = 512
    segs = [(4, 0), (2, 2), (3, 1)]
    fx = [_fixture(b, group, NV, k, fma1=(m == 2)) for b, m in segs]
    launches = _probe_cols(k, 4)

    def run():
        outs = []
        for c in launches:
            ys = [torch.empty(4, NV, dtype=torch.float16, device=_dev()) for _ in segs]
            ops.gemv_grouped(_onehot(c, k), [dict(qn=_native(f, m)[0], mn=_native(f, m)[1], bits=b, mode=m, N=NV, y=y) for (b, m), f, y in zip(segs, fx, ys)], k,
                             opts=ops.GemvOpts(math=ops.MATH_EXACT))
            outs.append(torch.cat(ys, dim=1))
        return torch.cat(outs)
    y = _both(run)
    for i, ((b, m), f) in enumerate(zip(segs, fx)):
        _check(y[:, i * NV:(i + 1) * NV], f["exact"][m], f["L"], launches.reshape(-1), f"gemv_grouped segment {i} ({b} bit, mode {MODE_NAMES[m]}), group {group}")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("rows,k", GEMV_SHAPES + [(8, 11008)])
def test_gemv_groupscale_weights(rows, k, bits):
    """MATH_GROUPSCALE (MODE_HQQ, groups of 128): the first rounding d = RN16(q 2^-9 + RN16(-z 2^-9)) per weight, the scale applied to the fp32 sum --
    with a one-hot row the sum is the one product (s 2^9) d, 22 bits: exact, and y is its rounding to fp16"""
    from amq_amd import ops
    launches = _probe_cols(k, rows)
    f = _fixture(bits, 128, NV, k)
    qn, mn = f["hqq"]
    y = _both(lambda: _run_gemv(launches, k, qn, mn, bits, ops.MODE_HQQ, NV, ops.GemvOpts(math=ops.MATH_GROUPSCALE)))
    _check(y, f["gs"], f["L"], launches.reshape(-1), f"gemv group-scale, {rows} rows, K {k}, {bits} bit")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("group", (64, 32))
def test_gemv_groupscale_option_on_exact_bodies(group, bits):
    """the finer groups and the one-rounding modes run their exact bodies under the group-scale option: the exact restatement's bits"""
    from amq_amd import ops
    launches = _probe_cols(K, 4)
    opts = ops.GemvOpts(math=ops.MATH_GROUPSCALE)
    f = _fixture(bits, group, NV, K)
    y = _both(lambda: _run_gemv(launches, K, f["hqq"][0], f["hqq"][1], bits, ops.MODE_HQQ, NV, opts))
    _check(y, f["exact"][0], f["L"], launches.reshape(-1), f"gemv group-scale option, group {group}, {bits} bit, mode HQQ")
    f = _fixture(bits, 128, NV, K)
    y = _both(lambda: _run_gemv(launches, K, f["fma"][0], f["fma"][1], bits, ops.MODE_FMA, NV, opts))
    _check(y, f["exact"][1], f["L"], launches.reshape(-1), f"gemv group-scale option, group 128, {bits} bit, mode FMA")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("rows,k", [(1, 512), (4, 512), (16, 512), (1, 8192), (5, 8192)])
def test_gemv_linear_weights(rows, k, bits):
    """MATH_LINEAR (groups of 128), amq_gemv_body.cuh: per tile y += fmaf(s 2^(24-SH), sum_k x_k q_k 2^(SH-24), fmaf(zx, sum_g x, y)) in fp32 with
    zx = -(s z) (HQQ; 22 bits: exact) or c.  With a one-hot row both sums are exact (q 2^(SH-24), 1.0) and y = RN16(RN32(s q + zx)) of the EXACT
    s q + zx -- one fp32 and one fp16 rounding of the real-valued weight, restated as such: exact, no tolerance"""
    from amq_amd import ops
    launches = _probe_cols(k, rows)
    f = _fixture(bits, 128, NV, k)
    for mode in (0, 1, 2):
        qn, mn = _native(f, mode)
        y = _both(lambda: _run_gemv(launches, k, qn, mn, bits, mode, NV, ops.GemvOpts(math=ops.MATH_LINEAR)))
        _check(y, f["linear"][mode], f["L"], launches.reshape(-1), f"gemv linear, {rows} rows, K {k}, {bits} bit, mode {MODE_NAMES[mode]}")


# ------------------------------------------------------------------------------------------------------------- the FMA1 boundary
@pytest.mark.parametrize("bits", BITS)
def test_fma1_boundary_layers(bits):
    """largest |scale| = the fp16 value AT amq_fma1_scale_bound: MODE_FMA1; the next fp16 value: MODE_FMA.  Both multiply by the oracle's weights."""
    from amq_amd import ops, _lib
    from amq_amd.quant_linear import HIPQuantLinear
    k = 512
    at, nxt = ref.fma1_bound16(bits)
    assert float(at) <= float(_lib.load().amq_fma1_scale_bound(bits)) < float(nxt)
    for above in (False, True):
        L = ref.make_boundary_layer(bits, NV, k, above)
        qw, sc, zr = ref.gptq_buffers(L)
        want = np.asarray(gptq_ref.dequant_kernel(qw, sc, zr, bits), np.float16)
        assert np.array_equal(want.view(np.uint16), (ref.fma_exact if above else ref.fma1_exact)(L["q"], L["scale"], L["c"], bits, 128).view(np.uint16))
        mod = HIPQuantLinear.from_gptq_buffers(_t(qw), _t(sc), _t(zr), bits)
        expect = ops.MODE_FMA if above else ops.MODE_FMA1
        assert mod.mode == expect and ops.fma_mode_for(mod.meta, bits) == expect
        for rows in (1, 4):
            launches = _probe_cols(k, rows)
            y = _both(lambda: _run_gemv(launches, k, mod.qweight, mod.meta, bits, mod.mode, NV, ops.GemvOpts(math=ops.MATH_EXACT)))
            _check(y, want, L, launches.reshape(-1), f"FMA1 boundary ({'above' if above else 'at'}), {rows} rows, {bits} bit")


# ------------------------------------------------------------------------------------------------------------- the unpack's scale limit
@pytest.mark.parametrize("bits", BITS)
def test_constructors_refuse_a_scale_past_the_unpack_limit(bits):
    """one scale just past ops.scale_limit: the module constructors and load_state_dict refuse the layer by name; ops.dequantize (the other unpack)
    of the same buffers still equals the oracle.  (No matmul kernel is run on such a layer.)"""
    from amq_amd import ops
    from amq_amd.hqq_format import HQQWeights
    from amq_amd.quant_linear import HIPQuantLinear
    n, k = NV, 512
    L = ref.make_boundary_layer(bits, n, k, False)
    good = dict(L)
    s, z = L["scale"].copy(), L["zero"].copy()
    past = np.nextafter(np.float16(ops.scale_limit(bits)), np.float16(np.inf))
    s[3, 2], z[3, 2] = past, np.float16((2 ** bits - 1) / 2.0)          # (|q - z| <= 7.5: the weights stay finite)
    L["scale"], L["zero"] = s, z
    L["c"] = ref.rn16(-(z.astype(np.float64) * s.astype(np.float64)))
    wq, s1, z1 = ref.hqq_buffers(L)
    want = hqq_ref.dequantize(wq, s1, z1, bits, (n, k))
    assert np.isfinite(want.astype(np.float64)).all()
    qn, mn = ops.repack_from_hqq(_t(wq), _t(s1.reshape(-1)), _t(z1.reshape(-1)), bits, n, k)
    got = _both(lambda: ops.dequantize(qn, mn, bits, ops.MODE_HQQ, n, k))
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    h = HQQWeights(torch.from_numpy(np.ascontiguousarray(wq)), torch.from_numpy(s1.copy()), torch.from_numpy(z1.copy()), bits, (n, k), name="blk.7.down_proj")
    with pytest.raises(ValueError, match=r"blk\.7\.down_proj.*exceeds"):
        HIPQuantLinear.from_hqq(h, device=_dev())
    qw, sc, zr = ref.gptq_buffers(L)
    with pytest.raises(ValueError, match="exceeds"):
        HIPQuantLinear.from_gptq_buffers(_t(qw), _t(sc), _t(zr), bits, name="blk.7.down_proj")
    m0 = HIPQuantLinear(bits, 128, k, n).to(_dev())
    with pytest.raises(ValueError, match="exceeds"):
        m0.pack(_t(want), _t(s), _t(z))
    # a good layer loads; the same state with one scale raised past the limit does not
    wq, s0, z0 = ref.hqq_buffers(good)
    ok = HIPQuantLinear.from_hqq(HQQWeights(torch.from_numpy(np.ascontiguousarray(wq)), torch.from_numpy(s0.copy()), torch.from_numpy(z0.copy()), bits, (n, k)), device=_dev())
    ok.to_kernel_arithmetic()
    state = {kk: v.clone() for kk, v in ok.state_dict().items()}
    m1 = HIPQuantLinear(bits, 128, k, n).to(_dev())
    m1.load_state_dict(state)
    assert m1.mode == ok.mode
    state["meta"].view(-1, 2)[5, 0] = float(past)
    with pytest.raises(ValueError, match="exceeds"):
        HIPQuantLinear(bits, 128, k, n).to(_dev()).load_state_dict(state)
