"""CPU-only: the restatements of the kernels' weight unpacks (tests/metadomain_ref.py -- what test_gpu_metadomain.py holds every matmul kernel
to, bit for bit) against the oracle, over fixture layers whose (scale, zero) span the fp16 range: equal bit for bit on the safe set, within the
derived bound outside it; the one-rounding modes equal the reference kernels' fma everywhere.  And ops.check_scale_range, the load-time refusal
of a scale the scaled-subnormal unpack cannot take."""
import numpy as np
import pytest
import torch

import metadomain_ref as ref
from oracle import gptq_ref, hqq_ref

BITS = (2, 3, 4)
GROUPS = (128, 64, 32)
N, K = 144, 512


def _same(a, b):
    a, b = np.asarray(a, np.float16), np.asarray(b, np.float16)
    return (a.view(np.uint16) == b.view(np.uint16)) | ((a == 0) & (b == 0))          # +0 / -0 counted equal


def _oracle_hqq(layer):
    wq, s, z = ref.hqq_buffers(layer)
    return hqq_ref.dequantize(wq, s, z, layer["bits"], (layer["n"], layer["k"]), group_size=layer["group"])


def _oracle_fma(layer):
    qw, sc, zr = ref.gptq_buffers(layer)
    return np.asarray(gptq_ref.dequant_kernel(qw, sc, zr, layer["bits"], group_size=layer["group"]), np.float16)


def _ratio(err, bound):
    """worst err / bound over elements with err > 0 (0 / 0 counts as 0)"""
    nz = err > 0
    if not nz.any():
        return 0.0
    with np.errstate(divide="ignore"):
        return float(np.max(err[nz] / bound[nz]))


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("bits", BITS)
def test_fixture_covers_what_it_claims(bits, group):
    L = ref.make_layer(bits, group, N, K)
    q, cls = L["q"], L["cls"]
    assert q.min() == 0 and q.max() == 2 ** bits - 1
    for pos in range(128):                                          # every code value at every position of a 128-column tile
        assert len(np.unique(q[:, pos::128])) == 2 ** bits
    # every class contributes at least one full (row, group) pair -- to the layer, to every 16-row tile, and to every column of groups
    assert set(np.unique(cls)) == set(range(len(ref.CLASSES)))
    for t in range(N // 16):
        assert len(np.unique(cls[16 * t:16 * t + 16])) == len(ref.CLASSES)
    s, z = L["scale"].astype(np.float64), L["zero"].astype(np.float64)
    maxq = 2 ** bits - 1
    c = {name: cls == i for i, name in enumerate(ref.CLASSES)}
    assert (z[c["neg_zero"]] < 0).all() and z[c["neg_zero"]].min() < -30
    assert (z[c["zero_above"]] >= maxq).all() and z[c["zero_above"]].max() > 250
    zi = L["zero"][c["int_zero"]]
    assert (zi.astype(np.float64) == np.rint(zi.astype(np.float64))).all()
    assert (zi.view(np.uint16) == 0x0000).any() and (zi.view(np.uint16) == 0x8000).any()       # +0 and -0
    assert (np.abs(z[c["tiny_zero"]]) <= 0.03).all() and (z[c["tiny_zero"]] < 0).any()
    assert (np.abs(s[c["subnormal_scale"]]) < 2.0 ** -14).all() and (s[c["subnormal_scale"]] > 0).all()
    assert (s[c["neg_scale"]] < 0).all()
    lim = ref.F16_MAX * 2.0 ** ref.SD_E[bits]
    assert (np.abs(s) <= lim).all() and s[c["large_scale"]].max() > 0.5 * min(lim, ref.F16_MAX / maxq)
    # finite weights in every arithmetic
    for w in (_oracle_hqq(L), _oracle_fma(L), ref.hqq_exact(q, L["scale"], L["zero"], bits, group), ref.fma_exact(q, L["scale"], L["c"], bits, group),
              ref.gs_weight(q, L["scale"], L["zero"], group), ref.linear_weight(q, L["scale"], L["zero"], group, False)):
        assert np.isfinite(w.astype(np.float64)).all()
    # the comparison is not vacuous: at least 80 % of the layer in the exact path's safe set
    safe, _, _ = ref.masks(q, L["zero"], group, ref.safe_threshold(bits))
    assert safe.mean() >= 0.8, safe.mean()


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("bits", BITS)
def test_exact_restatement_against_the_oracle(bits, group):
    """MODE_HQQ, scaled-subnormal form == Quantizer.dequantize bit for bit on |z|, |q - z| >= 2^(-14-E); within metadomain_ref.exact_bound outside
    (and the first rounding alone within first_rounding_bound).  Prints, per class, the share of the safe set and the worst error / bound."""
    L = ref.make_layer(bits, group, N, K)
    q = L["q"]
    w_ref = _oracle_hqq(L)
    w = ref.hqq_exact(q, L["scale"], L["zero"], bits, group)
    safe, z_small, d_small = ref.masks(q, L["zero"], group, ref.safe_threshold(bits))
    same = _same(w, w_ref)
    err = np.abs(w.astype(np.float64) - w_ref.astype(np.float64))
    bound = ref.exact_bound(q, L["scale"], L["zero"], w_ref, bits, group)
    old = np.maximum(2.0 ** -24 * 2.0 ** -ref.SD_E[bits] * np.abs(ref.expand(L["scale"], group)), 2.0 ** -24)      # the bound the header used to state
    # the first rounding on its own, in units of (q - z)
    e = ref.SD_E[bits]
    zc = ref.rn16(-ref.expand(L["zero"], group) * 2.0 ** e).astype(np.float64)
    d = ref.rn16(q * 2.0 ** e + zc).astype(np.float64) * 2.0 ** -e
    d_ref = ref.rn16(q - ref.expand(L["zero"], group)).astype(np.float64)
    derr = np.abs(d - d_ref)
    dbound = ref.first_rounding_bound(q, L["zero"], bits, group)
    cn = ref.class_names(L)
    print(f"\nexact {bits} bit, group {group}: class, safe share, differing (unsafe), worst err/bound, worst err/old bound, worst first-rounding err/bound")
    for i, name in enumerate(ref.CLASSES):
        m = cn == i
        u = m & ~safe
        print(f"  {name:16s} {safe[m].mean():6.3f} {(~same[u]).mean() if u.any() else 0.0:6.3f} {_ratio(err[u], bound[u]):8.3f} "
              f"{_ratio(err[u], old[u]):9.2f} {_ratio(derr[u], dbound[u]):8.3f}")
        assert same[m & safe].all(), f"class {name}: {(~same[m & safe]).sum()} safe elements differ from the oracle"
        assert (err[u] <= bound[u]).all(), f"class {name}: beyond the derived bound"
        assert (derr[m] <= dbound[m]).all(), f"class {name}: first rounding beyond its bound"
    assert (derr[safe] == 0).all()
    assert safe.mean() >= 0.8


@pytest.mark.parametrize("bits", (2, 3))
def test_small_zero_points_do_exceed_the_formerly_documented_bound(bits):
    """the reason the header's words changed: with |z| below the threshold the fixture meets fp16 rounding ties, and the weights leave
    2^-24 2^-E |s| by orders of magnitude (while staying inside one ulp of (q - z) times |s| + an ulp of the weight)"""
    L = ref.make_layer(bits, 128, N, K)
    w_ref = _oracle_hqq(L).astype(np.float64)
    w = ref.hqq_exact(L["q"], L["scale"], L["zero"], bits, 128).astype(np.float64)
    _, z_small, d_small = ref.masks(L["q"], L["zero"], 128, ref.safe_threshold(bits))
    m = z_small & ~d_small
    old = np.maximum(2.0 ** -24 * 2.0 ** -ref.SD_E[bits] * np.abs(ref.expand(L["scale"], 128)), 2.0 ** -24)
    assert (np.abs(w - w_ref)[m] > 50 * old[m]).any()


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("bits", BITS)
def test_one_rounding_restatements_equal_the_reference_kernels(bits, group):
    """MODE_FMA (two-op form) == fma(q, s, -zeros) of the reference's kernels on every class; MODE_FMA1 the same wherever it applies: the
    boundary layer whose largest scale is the fp16 value AT amq_fma1_scale_bound"""
    L = ref.make_layer(bits, group, N, K)
    want = _oracle_fma(L)
    got = ref.fma_exact(L["q"], L["scale"], L["c"], bits, group)
    cn = ref.class_names(L)
    for i, name in enumerate(ref.CLASSES):
        assert _same(got, want)[cn == i].all(), f"MODE_FMA, class {name}"
    if group == 128:
        at, nxt = ref.fma1_bound16(bits)
        assert float(at) == 65504.0 / 2 ** (24 - ref.fma1_shift(bits)) and float(nxt) > float(at)
        for above in (False, True):
            B = ref.make_boundary_layer(bits, 64, 512, above)
            assert np.abs(B["scale"].astype(np.float64)).max() == float(nxt if above else at)
            want = _oracle_fma(B)
            assert _same(ref.fma_exact(B["q"], B["scale"], B["c"], bits, 128), want).all()
            if above:
                with pytest.raises(AssertionError, match="amq_fma1_scale_bound"):
                    ref.fma1_exact(B["q"], B["scale"], B["c"], bits, 128)
            else:
                assert _same(ref.fma1_exact(B["q"], B["scale"], B["c"], bits, 128), want).all()


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("bits", BITS)
def test_groupscale_restatement_against_the_oracle(bits, group):
    """group-scale first rounding d 2^9 == RN16(q - z) on |z|, |q - z| >= 2^-5, so the recovered weight RN16(d s 2^9) is the oracle's there; the
    weights elsewhere within (2^-9 |q - z| + 2^-15) |s|"""
    L = ref.make_layer(bits, group, N, K)
    q = L["q"]
    w_ref = _oracle_hqq(L)
    safe, _, _ = ref.masks(q, L["zero"], group, ref.safe_threshold(gs=True))
    d = ref.gs_first(q, L["zero"], group) * 2.0 ** -ref.GS_E
    d_ref = ref.rn16(q - ref.expand(L["zero"], group)).astype(np.float64)
    assert (d[safe] == d_ref[safe]).all()
    w = ref.gs_weight(q, L["scale"], L["zero"], group)
    assert _same(w, w_ref)[safe].all()
    err = np.abs(w.astype(np.float64) - w_ref.astype(np.float64))
    bound = ref.gs_bound(q, L["scale"], L["zero"], group)
    cn = ref.class_names(L)
    print(f"\ngroup-scale {bits} bit, group {group}: class, safe share, worst err/bound outside")
    for i, name in enumerate(ref.CLASSES):
        u = (cn == i) & ~safe
        print(f"  {name:16s} {safe[cn == i].mean():6.3f} {_ratio(err[u], bound[u]):8.3f}")
        assert (err[u] <= bound[u] * 1.0001).all(), f"class {name}"


@pytest.mark.parametrize("bits", BITS)
def test_linear_restatement_is_the_real_valued_weight_rounded(bits):
    """MATH_LINEAR recovers RN16(RN32(s (q - z))): within one fp16 ulp of the real-valued weight (in fact half an ulp plus fp32's share)"""
    L = ref.make_layer(bits, 128, N, K)
    real = (L["q"] - ref.expand(L["zero"], 128)) * ref.expand(L["scale"], 128)
    w = ref.linear_weight(L["q"], L["scale"], L["zero"], 128, False).astype(np.float64)
    assert (np.abs(w - real) <= 0.5 * ref.ulp16(real) * (1 + 2.0 ** -12) + 2.0 ** -25).all()
    wf = ref.linear_weight(L["q"], L["scale"], L["c"], 128, True).astype(np.float64)
    realf = L["q"] * ref.expand(L["scale"], 128) + ref.expand(L["c"], 128)
    assert (np.abs(wf - realf) <= 0.5 * ref.ulp16(realf) * (1 + 2.0 ** -12) + 2.0 ** -25).all()


# ---------------------------------------------------------------------------------------------------------------- ops.check_scale_range
def _meta(scales, zeros=None):
    s = torch.tensor(scales, dtype=torch.float16)
    z = torch.zeros_like(s) if zeros is None else torch.tensor(zeros, dtype=torch.float16)
    return torch.stack([s, z], dim=1).reshape(-1)


@pytest.mark.parametrize("bits,limit", [(4, 8188.0), (3, 2047.0), (2, 2047.0)])
def test_check_scale_range(bits, limit):
    from amq_amd import ops
    assert ops.scale_limit(bits) == limit
    nxt = float(np.nextafter(np.float16(limit), np.float16(np.inf)))
    for mode in (ops.MODE_HQQ, ops.MODE_FMA, ops.MODE_FMA1):
        ops.check_scale_range(_meta([1e-3, limit, -limit, 6e-8]), bits, mode)            # at the limit, either sign: s 2^-E = +-65504
        ops.check_scale_range(torch.empty(0, dtype=torch.float16), bits, mode)
        for bad in (nxt, -nxt, float("inf")):
            with pytest.raises(ValueError) as ei:
                ops.check_scale_range(_meta([1e-3, 0.5, bad, 0.25]), bits, mode, name="model.layers.3.mlp.up_proj")
            msg = str(ei.value)
            assert "model.layers.3.mlp.up_proj" in msg and str(abs(bad)) in msg and str(limit) in msg, msg
        with pytest.raises(ValueError, match="NaN"):
            ops.check_scale_range(_meta([1e-3, float("nan")]), bits, mode)
    # the zero point / c column is not a scale
    ops.check_scale_range(_meta([1e-3, 2e-3], [60000.0, -60000.0]), bits, ops.MODE_HQQ)
    # bfloat16 modules: their kernels do not use this unpack
    ops.check_scale_range(_meta([1e-3, 30000.0]).to(torch.bfloat16), bits, ops.MODE_HQQ)
    with pytest.raises(ValueError, match="bits"):
        ops.check_scale_range(_meta([1e-3]), 5, ops.MODE_HQQ)
    # the limit IS where the restated unpack stops being finite
    q = np.full((1, 128), 2 ** bits - 1)
    z = np.zeros((1, 1), np.float16)
    assert np.isfinite(ref.hqq_exact(q, np.full((1, 1), limit / 16, np.float16), z, bits, 128).astype(np.float64)).all()
    sc = ref.rn16(np.float64(nxt) * 2.0 ** -ref.SD_E[bits])
    assert np.isinf(sc)
