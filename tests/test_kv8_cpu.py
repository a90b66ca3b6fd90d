"""CPU-only: properties of the 8-bit KV cache's storage format as tests/kv8_ref.py restates it -- the restatement the GPU tests
hold the kernels to bit for bit -- and of the exact-score cases and the bound built on it."""
import numpy as np
import pytest
import torch

import attndomain_ref as A
import kv8_ref


def _rows(seed, n=64):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(n, 128, generator=g)
    r[1] *= 100.0
    r[2] *= 65504.0 / r[2].abs().max()                       # a row scaled to the largest fp16
    r[3] *= 2.0 ** -20                                       # fp16 subnormals
    r[4] = r[4] * 2.0 ** -24 * 4                             # a few subnormal steps only
    r = r.half()
    assert float(r[2].abs().max()) == 65504.0 and float(r[3].abs().max()) < 2.0 ** -14
    return r


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rounding_error_is_half_a_step(seed):
    r = _rows(seed)
    c, s = kv8_ref.quantize(r)
    assert c.dtype is torch.int8 and s.dtype is torch.float32 and torch.isfinite(s).all()
    err = np.abs(kv8_ref.dequantize(c, s) - r.double().numpy())
    lim = s.double().numpy()[:, None] / 2 * (1 + 2.0 ** -22)
    assert (err <= lim).all(), float((err / lim).max())
    # the absmax element codes to +-127; codes never reach -128
    idx = r.float().abs().argmax(-1)
    top = c[torch.arange(r.shape[0]), idx].int()
    assert (top.abs() == 127).all() and torch.equal(top.sign(), r[torch.arange(r.shape[0]), idx].float().sign().int())
    assert int(c.int().min()) >= -127 and int(c.int().max()) <= 127


def test_zero_rows_and_exact_integer_rows():
    r = torch.zeros(3, 128, dtype=torch.float16)
    r[1, 5] = -0.0
    c, s = kv8_ref.quantize(r)
    assert (s == 0).all() and (c == 0).all() and (kv8_ref.dequantize(c, s) == 0).all()
    g = torch.Generator().manual_seed(3)
    ints = torch.randint(-127, 128, (40, 128), generator=g)
    ints[:, 7] = 127
    ints[::2, 7] = -127
    c, s = kv8_ref.quantize(ints.half())
    assert (s == 1.0).all() and torch.equal(c.long(), ints)
    assert np.array_equal(kv8_ref.dequantize(c, s), ints.double().numpy())


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_nonfinite_row_gets_a_nan_scale(bad):
    r = _rows(5, 8)
    r[1, 77] = bad
    r[2, 0] = bad
    r[2, 127] = 65504.0
    c, s = kv8_ref.quantize(r)
    assert torch.isnan(s[1]) and torch.isnan(s[2]) and torch.isfinite(s[0]) and torch.isfinite(s[3])
    assert int(c.int().min()) >= -127
    d = kv8_ref.dequantize(c, s)
    assert np.isnan(d[1]).all() and np.isnan(d[2]).all() and np.isfinite(d[0]).all()


def test_every_step_is_one_fp32_operation():
    """the scale is RN32(a / 127) and a code is rint(RN32(r / s)) moved by the sign of the fp32 residual where that exceeds half a step: checked
    against float64 arithmetic rounded once"""
    r = _rows(9)
    c, s = kv8_ref.quantize(r)
    a = r.double().abs().amax(-1).numpy()
    assert np.array_equal(s.numpy(), (a / 127.0).astype(np.float32))          # fp64 quotient of two short operands, rounded once: the fp32 quotient
    q32 = (r.double().numpy() / s.double().numpy()[:, None]).astype(np.float32)
    x = np.rint(q32).astype(np.float64)
    e32 = (r.double().numpy() - x * s.double().numpy()[:, None]).astype(np.float32)
    hs = (s.numpy() * np.float32(0.5))[:, None]
    assert np.array_equal(c.numpy(), np.clip(x + (e32 > hs) - (e32 < -hs), -127, 127).astype(np.int8))
    assert np.abs(c.numpy().astype(np.float64) - np.rint(q32)).max() <= 1


@pytest.mark.parametrize("profile", kv8_ref.EXACT_PROFILES)
@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 2), (8, 1)])
def test_exact_cases_survive_the_cache(profile, nh, nkv):
    """every exact case: K and V rows come back from the quantizer as the integers they are (scale 1.0), the designed scores are kept, and the
    bound is attndomain_ref's plus the two terms of this kernel"""
    pos = 300
    sk = A.seams("single", pos)
    q, K, V, raw = kv8_ref.exact_case(profile, 2, nh, nkv, pos, sk)
    for X in (K, V):
        c, s = kv8_ref.quantize(torch.from_numpy(X))
        assert (s == 1.0).all()
        assert np.array_equal(kv8_ref.dequantize(c, s), X.astype(np.float64))
    s = raw * A.SCALE
    r = kv8_ref.reference(s, V.astype(np.float64))
    plain = A.reference(s, V, kernel="kv8")
    assert (r.bound >= plain.bound).all() and np.array_equal(r.ref, plain.ref)
    assert A.KERNELS["kv8"] == dict(model="f32", D=44, N=5)
    got = kv8_ref.attention64(q, K.astype(np.float64), V.astype(np.float64))
    assert np.abs(got - r.ref).max() <= 1e-9 * 127
    assert (r.bound < 0.02 * 127).all()                                       # a bound that would hide a lost key is no bound
