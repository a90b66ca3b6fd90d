"""The 8-bit lm_head's matrix-core kernel on the GPU (ops.lm8_gemm, QuantLlama(lm8_kernel="mfma")) against tests/lm8_ref.py.

Bars.  One-hot rows of x: bit for bit (one exact product, every other term an exact zero) -- this pins the k permutation of both operands, the
meta indexing and the weight rule.  Parity: |y - ref| <= 1e-3 |ref| + 1e-3 rms(ref) per row against the fp64 product of the bit-exact weights with
the (restated) normed x, the bar tests/test_gpu_lm8.py holds ops.lm8_gemv to (fp32 accumulation of exact fp16 products, another order).  Runner
logits, "mfma" against "dot" over the same packed layer: twice that bar, one for each kernel."""
import functools

import numpy as np
import pytest
import torch

import lm8_ref
from test_gpu_lm8 import SCALES, ZEROS, _bar, _domain_layer, _guarded, _guards_intact, _layer, _prompt, _runner
from test_gpu_metadomain import _both, _dev

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ 1. operand map and unpack
@pytest.mark.parametrize("scale", [s for s in SCALES if s != 300.0])      # (300 overflows to inf with a small zero: 0 * inf is no exact zero)
def test_one_hot_rows_read_the_weights_back_bit_for_bit(scale):
    """x row m = e(16 t + m), t = 0 .. 15, over the all-codes rows of one scale (the fp16 subnormal 2^-20 included): y[m, n] = w[n, 16 t + m]"""
    from amq_amd import ops
    codes, meta, want = _domain_layer()
    rows = [i * len(SCALES) + SCALES.index(scale) for i in range(len(ZEROS))]
    want = want[rows]
    assert bool(torch.isfinite(want).all()) and bool((want != 0).any())
    w8 = _layer(codes[rows], meta[rows])
    eye = torch.eye(256, dtype=torch.float16, device=_dev())
    for t in range(16):
        y = ops.lm8_gemm(eye[16 * t:16 * t + 16], w8)
        assert y.shape == (16, len(rows))
        expect = want[:, 16 * t:16 * t + 16].t().contiguous().numpy().view(np.uint16)
        assert np.array_equal(y.cpu().numpy().view(np.uint16), expect), (scale, t)


# ------------------------------------------------------------------------------------------------------------------ 2. parity
@functools.lru_cache(maxsize=None)
def _random_layer16(n, k):
    """the recipe of test_gpu_lm8._random_layer with 16 rows of x; the fp64 references without and with the norm, computed once"""
    g = torch.Generator().manual_seed(1000 * n + k)
    W = (torch.randn(n, k, generator=g) * 0.03).to(torch.float16)
    codes, meta = lm8_ref.quantize(W)
    w = lm8_ref.dequantize(codes, meta).to(torch.float64)
    x = torch.randn(16, k, generator=g).to(torch.float16)
    gamma = (1 + 0.1 * torch.randn(k, generator=g)).to(torch.float16)
    refs = {False: x.to(torch.float64) @ w.t(), True: lm8_ref.rmsnorm_f16(x, gamma, 1e-5).to(torch.float64) @ w.t()}
    return _layer(codes, meta), x.to(_dev()), gamma.to(_dev()), refs


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("n,k", [(1000, 128), (1031, 640), (520, 3584)])
def test_gemm_parity_rows_and_guards(n, k, norm):
    """one group / a K that is no multiple of a register buffer, an odd N (rows of y unaligned) / 28 groups, N no multiple of 16; M = 1, 2, 9, 16"""
    from amq_amd import ops
    w8, x, gamma, refs = _random_layer16(n, k)
    kw = dict(gamma=gamma, eps=1e-5) if norm else {}
    single = [ops.lm8_gemm(x[m], w8, **kw) for m in range(16)]
    for M in (1, 2, 9, 16):
        buf, y = _guarded(M, n)
        ops.lm8_gemm(x[:M].contiguous() if M > 1 else x[0], w8, out=y if M > 1 else y[0], **kw)
        assert _guards_intact(buf, M * n), (M, "guard bands")
        ref = refs[norm][:M].to(_dev())
        err = (y.double() - ref).abs()
        bar = 1e-3 * ref.abs() + 1e-3 * ref.pow(2).mean(dim=1, keepdim=True).sqrt()
        print(f"lm8_gemm N {n} K {k} M {M} norm {norm}: worst err / bar {float((err / bar).max()):.4f}")
        assert bool((err <= bar).all()), (M, float((err / bar).max()))
        for m in range(M):                              # rows of an M-row call equal single-row calls bit for bit
            assert torch.equal(y[m].view(torch.int16), single[m].view(torch.int16)), (M, m)
    if norm and (n, k) == (1031, 640):                  # ... and through the conservative-waits twin: the same bits
        _both(lambda: ops.lm8_gemm(x[:9].contiguous(), w8, **kw))


# ------------------------------------------------------------------------------------------------------------------ 3. the runner
@pytest.mark.parametrize("kw", [dict(batch=3), dict(lookup=3)], ids=["batch3", "lookup3"])
def test_runner_mfma_against_dot_over_the_same_packed_lm_head(kw, monkeypatch):
    from amq_amd import ops
    calls = []
    monkeypatch.setattr(ops, "lm8_gemm", (lambda f: lambda *p, **k: (calls.append(1), f(*p, **k))[1])(ops.lm8_gemm))
    a = _runner(8, **kw)
    ids = _prompt(batch=kw.get("batch", 1), seed=21)
    a.prefill(ids)
    first, fed, points = a.token.clone(), [], [a.logits.clone()]
    for _ in range(3):                                  # (set_token: a lookup runner then runs its rows without drafts, one token a step)
        fed.append(a.token[:a.B].clone())
        a.set_token(fed[-1].clone())
        a.decode_step()
        points.append(a.logits.clone())
    a.check()
    assert not calls                                    # "dot": every launch as it was
    b = _runner(8, lm8_kernel="mfma", lm_head_packed=a.lm_head_q, **kw)
    assert b.lm_head_q is a.lm_head_q
    b.prefill(ids)
    assert torch.equal(b.token[:b.B], first[:a.B])      # the first generated token
    got = [b.logits.clone()]
    for tok in fed:
        b.set_token(tok.clone())
        b.decode_step()
        got.append(b.logits.clone())
    b.check()
    assert calls
    for i, (la, lb) in enumerate(zip(points, got)):
        err = (lb.double() - la.double()).abs()
        bar = _bar(la)
        worst = float((err / bar.clamp_min(1e-30)).max())       # (a lookup runner's prompt pass leaves rows 1 .. D of the logits as they were: 0 / 0)
        print(f"{kw}, point {i}: worst |mfma - dot| / bar {worst:.4f}")
        assert bool((err <= bar).all()), (i, worst)
