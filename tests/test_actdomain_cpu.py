"""No GPU: the activation-domain restatements (tests/actdomain_ref.py) against Hugging Face's own fp16 arithmetic run by torch on the CPU, the caps
on how much of a launch the band may leave open, and the mutants the band check must reject (it would be no check if it let them through)."""
import numpy as np
import pytest
import torch

import actdomain_ref as ref
from metadomain_ref import rn16

K = 4096
CLASS_IDS = range(len(ref.X_CLASSES))
DEGENERATE = ("zero", "one_hot", "const")       # rows whose normalised values are one number (or 0): a share of them says nothing


def _rows(k=K):
    return np.stack([ref.x_row(c, k) for c in CLASS_IDS])


# ------------------------------------------------------------------------------------------------------------------ HF arithmetic is inside
def _hf_band_check(y, band, what):
    y = np.asarray(y, np.float16)
    ok = band.accepts(y)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} elements outside the band"
    clear = ~band.amb
    assert ref.same16(y, band.mid)[clear].all(), f"{what}: differs from RN16 of the fp64 value at an unambiguous element"


@pytest.mark.parametrize("k", [128, 4096, 5120, 11008])
def test_llama_rmsnorm_expression_lies_in_the_band(k):
    """LlamaRMSNorm.forward as written: weight * (h * rsqrt(h.pow(2).mean(-1) + eps)).to(fp16), h = x.float()"""
    x, gamma = _rows(k), ref.gamma_vec(k)
    h = torch.from_numpy(x).float()
    var = h.pow(2).mean(-1, keepdim=True)
    y = torch.from_numpy(gamma) * (h * torch.rsqrt(var + ref.NORM_EPS)).to(torch.float16)
    assert y.dtype == torch.float16
    _hf_band_check(y.numpy(), ref.rmsnorm_band(x, gamma), f"LlamaRMSNorm, K {k}")


def test_silu_mul_expression_lies_in_the_band():
    """LlamaMLP: act_fn(gate) * up in fp16, over every finite gate with up = 1 and with Gaussian up"""
    g = ref.gate_rows(K)
    for up in (np.ones_like(g), ref.up_rows(g.shape[0], K, gate=g)):
        y = torch.nn.functional.silu(torch.from_numpy(g)) * torch.from_numpy(up)
        _hf_band_check(y.numpy(), ref.silu_band(g, up), "F.silu(gate) * up")


def test_residual_plus_linear_plus_bias_is_the_epilogue_order():
    """residual + F.linear(x, W, bias) over the two-hot layer: the restatement's bits at every element, the overflowing row included"""
    m, n = 8, 256
    c = ref.epilogue_case(m, n)
    x = torch.from_numpy(np.concatenate([c["xa"], c["xb"]], axis=1))
    w = torch.from_numpy(ref.selection_codes(n, 2 * n, np.arange(n), np.arange(n) + n).astype(np.float16))
    lin = (x.float() @ w.float().t()).to(torch.float16) + torch.from_numpy(c["bias"])         # (Linear's bias add, as its own fp16 rounding)
    y = (torch.from_numpy(c["residual"]) + lin).numpy()
    want = ref.epilogue(c["acc"], c["bias"], c["residual"])
    assert ref.same16(y, want.lo).all()
    assert np.isinf(y[0].astype(np.float32)).any() and np.isfinite(y[1:].astype(np.float32)).all()


# ------------------------------------------------------------------------------------------------------------------ caps
def test_rmsnorm_band_leaves_at_most_4_percent_of_a_row_open():
    for k in (128, 1024, 4096, 5120, 11008):
        band = ref.rmsnorm_band(_rows(k), ref.gamma_vec(k))
        share = band.amb.mean(axis=1)
        assert (share <= ref.RMS_AMBIGUOUS_CAP).all(), (k, dict(zip(ref.X_CLASSES, share.round(4))))


def test_silu_band_leaves_at_most_3_5_percent_of_the_gates_open():
    g = ref.all_finite_halves()
    for rel in (2.0 ** -17, 2.0 ** -16):
        assert ref.silu_band(g, None, rel).amb.mean() <= ref.SILU_AMBIGUOUS_CAP
    assert ref.SILU_EPS <= 2.0 ** -16


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def test_band_rejects_a_single_rounding_rmsnorm():
    x, gamma = _rows(), ref.gamma_vec(K)
    band = ref.rmsnorm_band(x, gamma)
    rejected = ~band.accepts(ref.mutant_rms_single_rounding(x, gamma))
    for c in CLASS_IDS:
        if ref.X_CLASSES[c] not in DEGENERATE:
            assert rejected[c].mean() >= 0.10, (ref.X_CLASSES[c], rejected[c].mean())


def test_band_rejects_a_statistic_that_lost_a_share():
    x, gamma = _rows(), ref.gamma_vec(K)
    band = ref.rmsnorm_band(x, gamma)
    rejected = ~band.accepts(ref.mutant_rms_lost_share(x, gamma))
    share = {ref.X_CLASSES[c]: rejected[c].mean() for c in CLASS_IDS}
    for name in ("gauss3", "const", "gauss_small"):               # 1/8 of the sum gone: rstd 7 % off, 70 fp16 ulps
        assert share[name] >= 0.95, share
    assert share["massive"] >= 0.90, share                         # the -2500 channel sits in a dropped chunk: 0.17 % of the sum, rstd an ulp or two off
    # rows that cannot see this mutant, listed so that nobody expects them to: subnormal_grid (the sum is far below eps), massive_tiny (its sum IS
    # the channel at K / 3, in a kept chunk), zero, one_hot.  With the channel moved into a dropped chunk massive_tiny sees it:
    xm = x[ref.X_CLASSES.index("massive_tiny")].copy()
    xm[K // 3], xm[59] = xm[59], xm[K // 3]                        # column 59: chunk 7, a dropped one
    rej = ~ref.rmsnorm_band(xm[None], gamma).accepts(ref.mutant_rms_lost_share(xm[None], gamma))
    assert rej.mean() >= 0.95, rej.mean()


def test_band_rejects_g_times_rounded_sigmoid():
    g = ref.all_finite_halves()
    rejected = ~ref.silu_band(g).accepts(ref.mutant_silu_sigmoid_rounded(g))
    assert rejected.sum() >= 5000, int(rejected.sum())


def test_epilogue_rejects_a_single_rounding():
    c = ref.epilogue_case(8, 256)
    want = ref.epilogue(c["acc"], c["bias"], c["residual"])
    differs = ~ref.same16(ref.mutant_epilogue_single_rounding(c["acc"], c["bias"], c["residual"]), want.lo)
    assert differs.mean() >= 0.20, differs.mean()
    # ... and the bias add alone, without a residual
    with np.errstate(over="ignore"):
        one = rn16(c["acc"] + ref.f64(c["bias"]))
    assert (~ref.same16(one, ref.epilogue(c["acc"], c["bias"]).lo)).mean() >= 0.20


def test_fixture_rows_are_what_they_claim():
    x = _rows()
    t = np.abs(ref.rms_t(x[ref.X_CLASSES.index("massive_tiny")]))
    assert (t < 2.0 ** -14).mean() > 0.99                          # normalised values in the fp16 subnormal range
    sub = ref.f64(x[ref.X_CLASSES.index("subnormal_grid")])
    assert (np.abs(sub) < 2.0 ** -14).all() and (sub * sub).sum() / K < ref.NORM_EPS * 1e-3
    g = ref.f64(ref.gamma_vec(K))
    assert (g < 0).sum() > K // 10 and (np.log2(np.abs(g)) % 1 == 0).sum() > K // 20
    for rows in (1, 2, 3, 4, 5, 8, 16):
        _, cs = ref.launches(rows, 128)
        assert set(np.concatenate(cs).tolist()) == set(CLASS_IDS)
        if rows > 1:
            assert all(len({int(c[i]) for c in cs}) >= 2 for i in range(rows))
