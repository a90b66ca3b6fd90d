"""The 8-bit lm_head's tiled many-row kernel on the GPU (ops.lm8_gemm_rows, QuantLlama(lm8_kernel="tiled")) against tests/lm8_ref.py.

Bars.  One-hot rows of x: bit for bit (one exact product, every other term an exact zero) -- the k permutation of both operands, the meta indexing,
the weight rule and the tile-to-y map.  Parity: |y - ref| <= 1e-3 |ref| + 1e-3 rms(ref) per row against the fp64 product of the bit-exact weights,
the bar tests/test_gpu_lm8_gemm.py holds ops.lm8_gemm to (fp32 accumulation of exact fp16 products, another order).  Runner logits, "tiled" against
"dot" over the same packed layer: twice that bar (_bar), one for each kernel; NLL rows: twice the tolerance of tests/test_gpu_lm8.py line 276."""
import functools

import numpy as np
import pytest
import torch

import lm8_ref
from test_gpu_lm8 import SCALES, ZEROS, _bar, _domain_layer, _guarded, _guards_intact, _layer, _prompt, _runner
from test_gpu_metadomain import _both, _dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scale", [s for s in SCALES if s != 300.0])      # (300 overflows to inf with a small zero: 0 * inf is no exact zero)
def test_one_hot_rows_read_the_weights_back_bit_for_bit(scale):
    """x = eye(256) in one call (two M panels) over the all-codes rows of one scale: y[m, n] = w[n, m]"""
    from amq_amd import ops
    assert ops.LM8_ROWS_BM < 256
    codes, meta, want = _domain_layer()
    rows = [i * len(SCALES) + SCALES.index(scale) for i in range(len(ZEROS))]
    want = want[rows]
    assert bool(torch.isfinite(want).all()) and bool((want != 0).any())
    y = ops.lm8_gemm_rows(torch.eye(256, dtype=torch.float16, device=_dev()), _layer(codes[rows], meta[rows]))
    assert y.shape == (256, len(rows))
    assert np.array_equal(y.cpu().numpy().view(np.uint16), want.t().contiguous().numpy().view(np.uint16)), scale


@functools.lru_cache(maxsize=None)
def _random_layer(n, k, rows):
    """the recipe of test_gpu_lm8._random_layer with ``rows`` rows of x; the fp64 reference computed once"""
    g = torch.Generator().manual_seed(1000 * n + k)
    W = (torch.randn(n, k, generator=g) * 0.03).to(torch.float16)
    codes, meta = lm8_ref.quantize(W)
    x = torch.randn(rows, k, generator=g).to(torch.float16)
    return _layer(codes, meta), x.to(_dev()), x.to(torch.float64) @ lm8_ref.dequantize(codes, meta).to(torch.float64).t()


@pytest.mark.parametrize("n,k", [(1000, 128), (1031, 640), (520, 3584)])
def test_parity_edges_guards_and_row_independence(n, k):
    """one group (the pipeline's prologue only) / an odd N (rows of y unaligned) and an odd group count / 28 groups; N no multiple of the tile;
    M = 17 and one row past an M panel"""
    from amq_amd import ops
    big = ops.LM8_ROWS_BM + 1
    w8, x, ref = _random_layer(n, k, big)
    got = {}
    for M in (17, big):
        buf, y = _guarded(M, n)
        ops.lm8_gemm_rows(x[:M].contiguous(), w8, out=y)
        assert _guards_intact(buf, M * n), (M, "guard bands")
        r = ref[:M].to(_dev())
        err = (y.double() - r).abs()
        bar = 1e-3 * r.abs() + 1e-3 * r.pow(2).mean(dim=1, keepdim=True).sqrt()
        print(f"lm8_gemm_rows N {n} K {k} M {M}: worst err / bar {float((err / bar).max()):.4f}")
        assert bool((err <= bar).all()), (M, float((err / bar).max()))
        got[M] = y
    assert torch.equal(got[big][:17].view(torch.int16), got[17].view(torch.int16))       # row m does not depend on the call it is in
    if (n, k) == (1031, 640):                           # ... and through the conservative-waits twin: the same bits
        _both(lambda: ops.lm8_gemm_rows(x[:17].contiguous(), w8))


def _counted(monkeypatch):
    from amq_amd import ops
    calls = []
    monkeypatch.setattr(ops, "lm8_gemm_rows", (lambda f: lambda *p, **k: (calls.append(1), f(*p, **k))[1])(ops.lm8_gemm_rows))
    return calls


def test_runner_all_logits_prompt_pass_tiled_against_dot(monkeypatch):
    calls = _counted(monkeypatch)
    ids = _prompt(n=20, seed=5)
    a = _runner(8)
    a.all_logits = True
    a.prefill(ids)
    assert not calls                                    # "dot": every launch as it was
    b = _runner(8, lm8_kernel="tiled", lm_head_packed=a.lm_head_q)
    b.all_logits = True
    b.prefill(ids)
    a.check()
    b.check()
    assert calls and b._lm8_scratch is None and b.lm_head_q is a.lm_head_q
    assert torch.equal(a.token[:1], b.token[:1])
    la, lb = a.logits_rows, b.logits_rows
    assert la.shape[-2] == 20 and lb.shape == la.shape
    err, bar = (lb.double() - la.double()).abs(), _bar(la)
    print(f"all-logits prompt pass of 20 rows: worst |tiled - dot| / bar {float((err / bar).max()):.4f}")
    assert bool((err <= bar).all())


def test_runner_score_rows_tiled_against_dot(monkeypatch):
    from amq_amd.llama import QuantLlama
    import evalmetrics_ref as eref
    monkeypatch.setattr(QuantLlama, "SCORE_ROWS", 24)   # pieces of 24 and 15 rows: the tiled launch and, below 17 rows, the 16-row kernel
    calls = _counted(monkeypatch)
    a = _runner(8)
    b = _runner(8, lm8_kernel="tiled", lm_head_packed=a.lm_head_q)
    ids = torch.randint(0, 1024, (2, 40), generator=torch.Generator().manual_seed(77))
    na = a.score_rows(ids)
    assert not calls
    nb = b.score_rows(ids)
    assert calls and b._lm8_scratch is None
    # tests/test_gpu_lm8.py line 276: 2 d + 2 NLL_FLOOR, d the runner bar's worst value over the window's logits; twice that, one for each kernel
    d = float(_bar(a._lm_logits_many(a._rows_pass(ids.to(_dev()), 0, cache=False))).max())
    tol = 2.0 * (2.0 * d + 2.0 * eref.NLL_FLOOR)
    print(f"score_rows: worst |nll tiled - nll dot| {float((na - nb).abs().max()):.3e}, tolerance {tol:.3e}")
    assert bool(((na - nb).abs() <= tol).all())
