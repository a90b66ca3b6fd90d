"""The packed lm_head on the GPU: the 8-bit layer's kernels (ops.lm8_dequantize / ops.lm8_gemv) against tests/lm8_ref.py, and
QuantLlama(lm_head_bits=8 / 4) against a default runner whose fp16 lm_head holds the packed layer's own dequantized weights.

Bars.  Weights: bit for bit.  The norm prologue: the band of tests/actdomain_ref.py, as test_gpu_actdomain.py::test_gemv_f16w_with_gamma judges the
fp16 kernel.  GEMV: |y - ref| <= 1e-3 |ref| + 1e-3 rms(ref) against the fp64 dot of the bit-exact weights with the (restated) normed x -- the bar
tests/test_gpu_decode.py::test_gemv_f16w holds the fp16 kernel to (the accumulation has the same form).  Runner logits: twice that bar, one for each
of the two lm_head kernels compared (their hidden rows are identical: the block kernels and weights are the same)."""
import functools

import numpy as np
import pytest
import torch

import actdomain_ref as aref
import lm8_ref
from test_gpu_metadomain import _both, _dev, _t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = aref.NORM_EPS
GUARD = 64              # halves in front of and behind an output (keeps it 16-byte aligned)
SENTINEL = -1234.0


def _layer(codes, meta):
    from amq_amd.hqq_format import LM8Weights
    return LM8Weights(codes.contiguous().to(_dev()), meta.contiguous().to(_dev()), tuple(codes.shape))


def _guarded(rows, cols):
    """-> (whole buffer, its [rows, cols] middle), the buffer filled with a sentinel"""
    buf = torch.full((GUARD + rows * cols + GUARD,), SENTINEL, dtype=torch.float16, device=_dev())
    return buf, buf[GUARD:GUARD + rows * cols].view(rows, cols)


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------ 1. weights, bit for bit
ZEROS = (0.0, 0.5, 1.0 / 3.0, 127.25, 254.5, 255.0)
SCALES = (2.0 ** -20, 2.0 ** -14, 1e-3, 1.0, 300.0)      # an fp16 subnormal, the smallest normal, ..., one that overflows to inf with a small zero


@functools.lru_cache(maxsize=None)
def _domain_layer():
    """[30, 256]: row (zero, scale) holds all 256 codes, in order in its first group and reversed in its second"""
    n = len(ZEROS) * len(SCALES)
    codes = torch.empty(n, 256, dtype=torch.uint8)
    codes[:, :128] = torch.arange(128, dtype=torch.uint8)
    codes[:, 128:] = torch.arange(255, 127, -1, dtype=torch.int32).to(torch.uint8)
    codes[1::2] = codes[1::2].flip(1)                   # (odd rows: the other half of the codes in the first group)
    meta = torch.empty(n, 2, 2, dtype=torch.float16)
    for i, z in enumerate(ZEROS):
        for j, s in enumerate(SCALES):
            meta[i * len(SCALES) + j, :, 0] = s
            meta[i * len(SCALES) + j, :, 1] = z
    return codes, meta, lm8_ref.dequantize(codes, meta)


def test_dequantize_bit_for_bit_over_codes_zeros_and_scales():
    from amq_amd import ops
    codes, meta, want = _domain_layer()
    assert bool(torch.isinf(want).any()) and bool((want[torch.isfinite(want)] != 0).any())      # (the overflowing scale is in, and so are subnormal results)
    w8 = _layer(codes, meta)
    got = _both(lambda: ops.lm8_dequantize(w8))
    assert got.shape == (30, 256)
    assert np.array_equal(got.view(np.uint16), want.numpy().view(np.uint16))
    n = codes.shape[0]
    for row0, rows in ((0, 1), (7, 5), (n - 1, 1), (n - 3, 3)):
        buf, out = _guarded(rows, 256)
        ops.lm8_dequantize(w8, row0, rows, out=out)
        assert np.array_equal(out.cpu().numpy().view(np.uint16), want[row0:row0 + rows].numpy().view(np.uint16)), (row0, rows)
        assert _guards_intact(buf, rows * 256), (row0, rows)
    for row0, rows in ((n, 1), (n - 1, 2), (-1, 1), (0, 0)):
        with pytest.raises(ValueError):
            ops.lm8_dequantize(w8, row0, rows)


# ------------------------------------------------------------------------------------------------------------------ 2. the norm prologue read back
@functools.lru_cache(maxsize=None)
def _identity(k):
    meta = torch.zeros(k, k // 128, 2, dtype=torch.float16)
    meta[..., 0] = 1.0
    return _layer(torch.eye(k, dtype=torch.uint8), meta)


@pytest.mark.parametrize("rows", [1, 3, 8])
@pytest.mark.parametrize("k", [128, 640, 1024])
def test_identity_layer_returns_x_and_the_normed_x(k, rows):
    """the identity as an LM8 layer (codes 0 / 1, scale 1, zero 0).  Control: without gamma, x comes back exactly.  With gamma: the band."""
    from amq_amd import ops
    from test_gpu_actdomain import _exact, _judge
    w8 = _identity(k)
    gamma = aref.gamma_vec(k)
    xs, cs = aref.launches(rows, k)
    for j, (x, cl) in enumerate(zip(xs, cs)):
        xd = _t(x[0] if rows == 1 else x)
        what = f"lm8_gemv {rows} rows, K {k}, launch {j}"
        _exact(_both(lambda: ops.lm8_gemv(xd, w8)).reshape(rows, k), x, "control " + what, cl)
        y = _both(lambda: ops.lm8_gemv(xd, w8, gamma=_t(gamma), eps=EPS)).reshape(rows, k)
        _judge(y, aref.rmsnorm_band(x, gamma), "RMSNorm " + what, cl, cap=aref.RMS_AMBIGUOUS_CAP, inputs=x)


# ------------------------------------------------------------------------------------------------------------------ 3. GEMV parity
@functools.lru_cache(maxsize=None)
def _random_layer(n, k):
    """a quantized random layer + 8 rows of x + gamma; the fp64 references without and with the norm, computed once"""
    g = torch.Generator().manual_seed(1000 * n + k)
    W = (torch.randn(n, k, generator=g) * 0.03).to(torch.float16)
    codes, meta = lm8_ref.quantize(W)
    w = lm8_ref.dequantize(codes, meta).to(torch.float64)
    x = torch.randn(8, k, generator=g).to(torch.float16)
    gamma = (1 + 0.1 * torch.randn(k, generator=g)).to(torch.float16)
    refs = {False: x.to(torch.float64) @ w.t(), True: lm8_ref.rmsnorm_f16(x, gamma, 1e-5).to(torch.float64) @ w.t()}
    return _layer(codes, meta), x.to(_dev()), gamma.to(_dev()), refs


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("n,k", [(1000, 128), (1000, 640), (1031, 1024), (520, 3584)])
def test_gemv_parity_rows_and_guards(n, k, norm):
    """one group / a partial last wave-load / N no multiple of the wave count or of the row pair / 28 groups; M = 1, 2, 3, 5, 8"""
    from amq_amd import ops
    w8, x, gamma, refs = _random_layer(n, k)
    kw = dict(gamma=gamma, eps=1e-5) if norm else {}
    single = [ops.lm8_gemv(x[m], w8, **kw) for m in range(8)]
    for M in (1, 2, 3, 5, 8):
        buf, y = _guarded(M, n)
        ops.lm8_gemv(x[:M].contiguous() if M > 1 else x[0], w8, out=y if M > 1 else y[0], **kw)
        assert _guards_intact(buf, M * n), (M, "guard bands")
        ref = refs[norm][:M].to(_dev())
        err = (y.double() - ref).abs()
        bar = 1e-3 * ref.abs() + 1e-3 * ref.pow(2).mean(dim=1, keepdim=True).sqrt()
        print(f"lm8_gemv N {n} K {k} M {M} norm {norm}: worst err / bar {float((err / bar).max()):.4f}")
        assert bool((err <= bar).all()), (M, float((err / bar).max()))
        for m in range(M):                              # rows of an M-row call equal single-row calls bit for bit
            assert torch.equal(y[m].view(torch.int16), single[m].view(torch.int16)), (M, m)
    if norm and (n, k) == (1000, 640):                  # ... and through the conservative-waits twin: the same bits
        _both(lambda: ops.lm8_gemv(x[:5].contiguous(), w8, **kw))


def test_ops_wrappers_refuse_what_the_kernels_cannot_take():
    from amq_amd import ops
    w8, x, gamma, _ = _random_layer(1000, 128)
    with pytest.raises(ValueError):
        ops.lm8_gemv(torch.zeros(9, 128, dtype=torch.float16, device=_dev()), w8)
    with pytest.raises(ValueError):
        ops.lm8_gemv(x[0].float(), w8)
    with pytest.raises(ValueError):
        ops.lm8_gemv(x[0], w8, gamma=gamma[:64])
    with pytest.raises(ValueError):
        ops.lm8_gemv(x[0], w8, out=torch.zeros(999, dtype=torch.float16, device=_dev()))
    with pytest.raises(ValueError):
        ops.lm8_gemv(x[0].cpu(), w8)


# ------------------------------------------------------------------------------------------------------------------ 4. the runner
def _cfg(vocab=1024):
    from amq_amd import arch
    return dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=vocab))


def _runner(bits, **kw):
    from amq_amd.llama import QuantLlama
    return QuantLlama(_cfg(), None, device=DEV, max_seq=64, seed=3, lm_head_bits=bits, **kw)


def _pair(bits, **kw):
    """A: the packed runner; B: a default runner of the same seed whose fp16 lm_head holds A's dequantized weights (before any capture)"""
    a, b = _runner(bits, **kw), _runner(16, **kw)
    b.lm_head.copy_(a.lm_head_weights())
    return a, b


def _bar(ref):
    ref = ref.double()
    return 2.0 * (1e-3 * ref.abs() + 1e-3 * ref.pow(2).mean(dim=-1, keepdim=True).sqrt())


def _close(la, lb, what):
    err = (la.double() - lb.double()).abs()
    bar = _bar(lb)
    print(f"{what}: worst |A - B| / bar {float((err / bar).max()):.4f}")
    assert bool((err <= bar).all()), (what, float((err / bar).max()))
    lb2 = lb.double().reshape(-1, lb.shape[-1])
    top = lb2.topk(2, dim=-1)
    # the arg-max must agree wherever B's top-2 gap exceeds the runner bar (at the top two logits, the larger of their two bars)
    clear = (top.values[:, 0] - top.values[:, 1]) > _bar(lb).reshape(-1, lb.shape[-1]).gather(1, top.indices).max(dim=-1).values
    am_a, am_b = la.reshape(-1, la.shape[-1]).float().argmax(-1), lb2.argmax(-1)
    assert torch.equal(am_a[clear], am_b[clear]), what


def _prompt(batch=1, n=12, seed=9):
    return torch.randint(1, 1024, (batch, n) if batch > 1 else (n,), generator=torch.Generator().manual_seed(seed))


def _lockstep(a, b, ids, steps=6, use_graph=True):
    """both runners fed the same tokens (the prompt, then B's choices) -> [(logits A, logits B)] after the prompt and after every step"""
    out = []
    a.prefill(ids, use_graph=use_graph)
    b.prefill(ids, use_graph=use_graph)
    out.append((a.logits.clone(), b.logits.clone()))
    for _ in range(steps):
        a.set_token(b.token.clone())
        a.decode_step(use_graph)
        b.decode_step(use_graph)
        out.append((a.logits.clone(), b.logits.clone()))
    torch.cuda.synchronize()
    a.check()
    b.check()
    return out


@pytest.mark.parametrize("bits", [8, 4])
def test_runner_against_the_default_runner_over_the_same_weights(bits):
    a, b = _pair(bits)
    assert a.lm_head is None and a.lm_head_q is not None and a.lm_head_bits == bits      # a standalone packed runner holds no fp16 lm_head
    assert b.lm_head is not None and b.lm_head_q is None
    packed = a.lm_head_q.nbytes()
    assert packed == (1024 * 512 + 1024 * 4 * 4 if bits == 8 else a.lm_head_q.qn.numel() * 4 + a.lm_head_q.mn.numel() * 2)
    assert b.total_bytes_per_token(40) - a.total_bytes_per_token(40) == 1024 * 512 * 2 - packed
    ids = _prompt()
    graph = _lockstep(a, b, ids, use_graph=True)
    for i, (la, lb) in enumerate(graph):
        _close(la, lb, f"lm_head_bits={bits}, after {'the prompt' if i == 0 else f'step {i}'}")
    a2, b2 = _pair(bits)
    eager = _lockstep(a2, b2, ids, use_graph=False)
    for (la, _), (le, _) in zip(graph, eager):          # eager equals graph replay bit for bit
        assert torch.equal(la.view(torch.int16), le.view(torch.int16))


@pytest.mark.parametrize("bits", [8, 4])
def test_runner_batch_rows_equal_single_runs(bits):
    a3, b3 = _pair(bits, batch=3)
    ids = _prompt(batch=3, seed=21)
    a3.prefill(ids)
    b3.prefill(ids)
    points, fed = [(a3.logits.clone(), b3.logits.clone())], []
    for _ in range(3):
        fed.append(b3.token.clone())
        a3.set_token(fed[-1].clone())
        a3.decode_step()
        b3.decode_step()
        points.append((a3.logits.clone(), b3.logits.clone()))
    a3.check()
    for i, (la, lb) in enumerate(points):
        _close(la, lb, f"lm_head_bits={bits}, batch 3, point {i}")
    # ... and the three sequences alone, fed the batch's tokens: the same logits within the bar
    for s in range(3):
        a1 = _runner(bits)
        a1.prefill(ids[s])
        _close(points[0][0][s], a1.logits, f"lm_head_bits={bits}, sequence {s} alone, prompt")
        for i, tok in enumerate(fed):
            a1.set_token(tok[s:s + 1].clone())
            a1.decode_step()
            _close(points[i + 1][0][s], a1.logits, f"lm_head_bits={bits}, sequence {s} alone, step {i + 1}")
        a1.check()


@pytest.mark.parametrize("bits", [8, 4])
def test_runner_scores_the_packed_lm_head(bits, monkeypatch):
    from amq_amd.llama import QuantLlama
    import evalmetrics_ref as eref
    monkeypatch.setattr(QuantLlama, "SCORE_ROWS", 16)
    a, b = _pair(bits)
    ids = torch.randint(0, 1024, (2, 40), generator=torch.Generator().manual_seed(77))
    na, nb = a.score_rows(ids), b.score_rows(ids)
    # NLL = lse - logit[label]: a change of every logit by at most d moves each term by at most d; d is the runner bar on B's logits (rows of
    # roughly unit logits: the bar's worst value over the window), plus the metric kernel's own floor once per side
    x = b._rows_pass(ids.to(DEV), 0, cache=False)
    lb = b._lm_logits_many(x)
    la = a._lm_logits_many(x)
    _close(la, lb, f"lm_head_bits={bits}, all-logits rows")
    d = float(_bar(lb).max())
    tol = 2.0 * d + 2.0 * eref.NLL_FLOOR
    print(f"score_rows lm_head_bits={bits}: worst |nll A - nll B| {float((na - nb).abs().max()):.3e}, tolerance {tol:.3e}")
    assert bool(((na - nb).abs() <= tol).all())
    assert a.lm_head is None                           # (nothing dense was there to be scored)


def test_four_bit_route_beyond_the_prologue_rows(monkeypatch):
    """the two other branches of the 4-bit route: an rmsnorm launch + the plain GEMV above ops.gemv_max_rows(H), ops.gemm past the plain launch's
    rows.  At H = 512 eight rows fit the prologue launch, so the row limits are lowered for the call: the same 8 hidden rows through the three
    branches, each against the fp64 product of the layer's dequantized weights with the restated normed rows, at the GEMV bar"""
    from amq_amd import ops
    a = _runner(4)
    x = torch.randn(8, 512, generator=torch.Generator().manual_seed(31)).to(torch.float16).to(DEV)
    ref = lm8_ref.rmsnorm_f16(x.cpu(), a.norm.cpu(), a.eps).double() @ a.lm_head_weights().cpu().double().t()
    bar = 1e-3 * ref.abs() + 1e-3 * ref.pow(2).mean(dim=1, keepdim=True).sqrt()
    real, calls = ops.gemv_max_rows, []
    for name in ("gemv_grouped", "rmsnorm", "gemm"):
        monkeypatch.setattr(ops, name, (lambda n, f: lambda *p, **k: (calls.append(n), f(*p, **k))[1])(name, getattr(ops, name)))
    for limits, want in (((8, 8), ["gemv_grouped"]), ((2, 8), ["rmsnorm", "gemv_grouped"]), ((2, 2), ["rmsnorm", "gemm"])):
        monkeypatch.setattr(ops, "gemv_max_rows", lambda K, plain=False, norm=True, lim=limits: min(real(K, plain, norm), lim[1] if plain else lim[0]))
        calls.clear()
        out = torch.empty(8, 1024, dtype=torch.float16, device=DEV)
        a._lm_logits(x, out)
        assert calls == want, (limits, calls)
        err = (out.cpu().double() - ref).abs()
        print(f"4-bit route {want}: worst err / bar {float((err / bar).max()):.4f}")
        assert bool((err <= bar).all()), (want, float((err / bar).max()))


def test_many_row_logits_through_dequantized_slices(monkeypatch):
    """8 bits, many rows: slices of vocabulary rows dequantized into a bounded scratch + the fp16 GEMM per slice (three slices here, the last one
    shorter) against B's fp16 GEMM over the same weights at the runner bar, and against the 8-rows-a-launch route; fewer rows keep the latter"""
    from amq_amd import ops
    from amq_amd.llama import QuantLlama
    monkeypatch.setattr(QuantLlama, "LM8_SLICE_ROWS", 384)
    a, b = _pair(8)
    x = torch.randn(100, 512, generator=torch.Generator().manual_seed(8)).to(torch.float16).to(DEV)
    calls = []
    monkeypatch.setattr(ops, "lm8_dequantize", (lambda f: lambda *p, **k: (calls.append("deq"), f(*p, **k))[1])(ops.lm8_dequantize))
    monkeypatch.setattr(ops, "lm8_gemv", (lambda f: lambda *p, **k: (calls.append("gemv"), f(*p, **k))[1])(ops.lm8_gemv))
    buf, out = _guarded(100, 1024)
    a._lm_logits_many(x, out)
    assert calls == ["deq"] * 3 and _guards_intact(buf, 100 * 1024) and tuple(a._lm8_scratch.shape) == (384, 512)
    lb = b._lm_logits_many(x)
    _close(out, lb, "lm_head_bits=8, 100 rows through dequantized slices")
    calls.clear()
    streamed = a._lm_head_streamed(x, torch.empty(100, 1024, dtype=torch.float16, device=DEV))
    _close(streamed, lb, "lm_head_bits=8, 100 rows, 8 rows a launch")
    calls.clear()
    a._lm_logits_many(x[:63].contiguous())
    assert calls == ["gemv"] * 8


def test_runner_combinations_run_clean():
    """lm_head_bits=8 with kv_bits=8, ragged=True, lookup=3 and the sampled tail; 4 bits with the sampled tail and a batch"""
    ids = _prompt()
    a, b = _pair(8, kv_bits=8)
    for la, lb in _lockstep(a, b, ids, steps=4):
        _close(la, lb, "lm_head_bits=8 with kv_bits=8")
    r = _runner(8, batch=2, ragged=True)
    out = r.generate(_prompt(batch=2, n=10, seed=4), 6, lengths=[10, 7])
    r.check()
    assert out.shape == (2, 6) and int(out.min()) >= 0 and int(out.max()) < 1024
    plain = _runner(8)
    want = plain.generate(ids, 10)
    look = _runner(8, lookup=3)
    got = look.generate(ids, 10)
    look.check()
    assert got.shape == (10,)
    assert torch.equal(got[:1], want[:1])               # (the verify rows run 4-row launches: later tokens may part at a near-tie, the first cannot)
    for bits in (8, 4):
        s = _runner(bits)
        s.set_sampling(0.8, 20, 0.9, seed=5)
        t1 = s.generate(ids, 8).clone()
        t2 = s.generate(ids, 8).clone()
        s.check()
        assert torch.equal(t1, t2) and t1.shape == (8,)
    r4 = _runner(4, batch=2)
    r4.generate(_prompt(batch=2, n=10, seed=4), 4)
    r4.check()


def test_runner_refusals():
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    with pytest.raises(ValueError, match="engine"):
        _runner(8, engine=True)
    with pytest.raises(ValueError, match="N % 16"):
        QuantLlama(dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=1001)), None, device=DEV, max_seq=64, lm_head_bits=4)
    r = QuantLlama(dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=1001)), None, device=DEV, max_seq=64, lm_head_bits=8)      # any vocabulary at 8 bits
    r.generate(_prompt() % 1001, 3)                     # (ids inside THIS vocabulary)
    r.check()


# ------------------------------------------------------------------------------------------------------------------ 5. the HF surface
def test_hf_surface_shares_one_packed_lm_head():
    pytest.importorskip("transformers")
    from amq_amd import hf_fast
    from amq_amd.llama import QuantLlama
    from test_gpu_hf_fast import _hf_generate, _prepared
    model, _ = _prepared("llama3.1")                                 # (max_position_embeddings 512: a runner of 256 positions can grow)
    ids = torch.randint(1, 1000, (1, 9), generator=torch.Generator().manual_seed(6)).to(DEV)
    direct = QuantLlama.from_hf(model, max_seq=256, lm_head_bits=8)
    assert direct.lm_head is None
    want = direct.generate(ids[0], 12)
    try:
        hf_fast.convert_model_to_hip(model)
        with torch.inference_mode():
            plain = _hf_generate(model, ids, 12)
        assert hf_fast._RUNNERS[model][1].lm_head_bits == 16 and "_amq_lm_head_packed" not in model.__dict__      # without the flag: as before
        hf_fast.convert_model_to_hip(model, lm_head_bits=8)
        assert model not in hf_fast._RUNNERS                         # (the fp16 runners are gone)
        with torch.inference_mode():
            fast = _hf_generate(model, ids, 12)
        r1 = hf_fast._RUNNERS[model][1]
        assert r1.lm_head_bits == 8 and r1.lm_head is None
        assert torch.equal(fast[0, 9:], want)                        # token for token the direct runner
        assert plain.shape == fast.shape
        packed = model.__dict__["_amq_lm_head_packed"][1]
        assert r1.lm_head_q is packed
        with torch.inference_mode():                                 # growth: a longer call rebuilds the runner over the SAME packed object
            ids2 = torch.randint(1, 1000, (1, 250), generator=torch.Generator().manual_seed(7)).to(DEV)
            _hf_generate(model, ids2, 12)
            two = torch.cat([ids, ids], dim=0)
            _hf_generate(model, two, 4)                              # another batch size
        r2, rb = hf_fast._RUNNERS[model][1], hf_fast._RUNNERS[model][2]
        assert r2 is not r1 and r2.lm_head_q is packed and rb.lm_head_q is packed
        assert isinstance(model.lm_head, torch.nn.Linear) and model.lm_head.weight.dtype == torch.float16      # the module keeps its weight
    finally:
        hf_fast.revert_model_to_hf(model)
    assert not [k for k in model.__dict__ if k.startswith("_amq")] and model not in hf_fast._RUNNERS
    assert "forward" not in model.__dict__ and "generate" not in model.__dict__


# ------------------------------------------------------------------------------------------------------------------ 6. the default, untouched
def test_default_runner_launch_list_still_ends_in_the_fp16_lm_head(monkeypatch):
    from amq_amd import ops
    r = _runner(16)
    r.prefill(_prompt(n=4), use_graph=False)
    calls = []

    def recorder(name, fn):
        def wrapped(*args, **kwargs):
            calls.append(name)
            return fn(*args, **kwargs)
        return wrapped

    names = ("gemv_grouped", "gemv_grouped_sums", "attn_decode", "rmsnorm", "silu_mul", "gemm", "gemv_f16w", "lm8_gemv", "decode_tail")
    for name in names:
        monkeypatch.setattr(ops, name, recorder(name, getattr(ops, name)))
    r._step()
    torch.cuda.synchronize()
    r.check()
    assert calls[-2:] == ["gemv_f16w", "decode_tail"] and "lm8_gemv" not in calls
    calls.clear()
    p = _runner(8)
    p.prefill(_prompt(n=4), use_graph=False)
    p._step()
    assert calls[-2:] == ["lm8_gemv", "decode_tail"] and "gemv_f16w" not in calls
    calls.clear()
    q = _runner(4)
    q.prefill(_prompt(n=4), use_graph=False)
    q._step()
    torch.cuda.synchronize()
    assert calls[-2:] == ["gemv_grouped", "decode_tail"] and "gemv_f16w" not in calls and "lm8_gemv" not in calls
