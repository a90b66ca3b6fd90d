"""GPU: sampled prompt-lookup decoding inside the captured token step.

1. the sampled verify-and-propose tail (amq_decode_tail_lookup_sample_f16) bit for bit against the kernels the project already trusts: every row's
   token is what amq_sample_f16 draws from that row with draw counter c + j, and everything behind the draws is tests/lookup_sample_ref.py;
2. the runner (QuantLlama(lookup=D, lookup_sampling=True)) replays its own decisions: after every step the draws are recomputed from the step's own
   logits rows, drafts and counter; graph replay == eager; step counts; the three draft sources against each other;
3. proposals are accepted under sampling on a model built to repeat;
4. the runner's surface; 5. the HF surface (convert_model_to_hip(model, lookup=True, sampling=True))."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_ref  # noqa: E402
import lookup_sample_ref  # noqa: E402
import sampling_ref  # noqa: E402
from test_gpu_lookup import SUP, _prompt, _swap_linears, _tiny  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SMP_DRAW, SMP_ARRIVE = 6, 25


def _dev():
    return torch.device(DEV)


def _counter(state):
    """the 64-bit draw counter of a sampling block"""
    lo, hi = state[SMP_DRAW:SMP_DRAW + 2].tolist()
    return (lo & 0xFFFFFFFF) | ((hi & 0xFFFFFFFF) << 32)


def _set_counter(state, c):
    host = torch.tensor([c & 0xFFFFFFFF, c >> 32], dtype=torch.int64)
    state[SMP_DRAW:SMP_DRAW + 2].copy_(torch.where(host >= 1 << 31, host - (1 << 32), host).to(torch.int32))


def _draws(ops, logits, state, c, suppress=None, u=None, kept=None):
    """what the trusted sampler draws from each row: row j with a copy of ``state`` whose draw counter is c + j (sequence 0), or with u[j]"""
    out = []
    for j in range(logits.shape[0]):
        sj = state.clone()
        _set_counter(sj, (c + j) & ((1 << 64) - 1))
        tok = ops.sample(logits[j], sj, suppress=suppress, u=None if u is None else u[j:j + 1].contiguous(),
                         kept_out=None if kept is None else kept[j])
        out.append(int(tok.item()))
        assert int(sj[SMP_ARRIVE].item()) == 0
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. the tail kernel
HID, ROPE_ROWS = 16, 48
_EMBED = {}


def _embed(vocab):
    if vocab not in _EMBED:
        g = torch.Generator().manual_seed(vocab)
        _EMBED[vocab] = (torch.randn(vocab, HID, generator=g).half().to(_dev()), torch.randn(ROPE_ROWS, 128, generator=g).half().to(_dev()))
    return _EMBED[vocab]


def _tail_case(ops, vocab, logits, params, c, history, make_drafts, ngram=2, external=False, suppress=(), use_u=False, steps0=3, twin=None):
    """one launch of the sampled tail on ``logits`` [R, vocab] with sampling parameters ``params`` and draw counter ``c``; ``make_drafts(t)`` builds
    the D drafts the step ran with from the expected draws t.  Everything tests/test_gpu_lookup.py::_tail_case asserts, with the draws for the
    arg-maxes, plus the draw words, the untouched sampling words and LK_ARGMAX + j == t_j.  -> (n, t)"""
    from amq_amd import _lib
    dev, R = _dev(), logits.shape[0]
    D = R - 1
    embed, tab = _embed(vocab)
    smp = ops.new_sampling_state(dev)
    ops.set_sampling_state(smp, temperature=params[0], top_k=params[1], top_p=params[2], seed=0x1234567887654321 ^ vocab, eos_ids=(3, 4), pad_id=2)
    _set_counter(smp, c)
    sup = torch.tensor(list(suppress) + [-1] * (8 - len(suppress)), dtype=torch.int32, device=dev) if suppress else None
    u = torch.rand(R, generator=torch.Generator().manual_seed(c % 1000 + R)).to(dev) if use_u else None
    kept_ref = torch.zeros(R, vocab, dtype=torch.uint8, device=dev) if use_u else None
    t = _draws(ops, logits, smp, c, suppress=sup, u=u, kept=kept_ref)
    drafts = make_drafts(t)
    state, hist = ops.new_lookup_state(dev, D, ngram, ROPE_ROWS)
    hist[:len(history)].copy_(torch.tensor(history, dtype=torch.int32))
    host = state.cpu()
    host[ops.LOOKUP_MODE], host[ops.LOOKUP_COUNT], host[ops.LOOKUP_STEPS] = int(external), len(history), steps0
    for i, d in enumerate(drafts):
        host[ops.LOOKUP_DRAFT + 1 + i] = d
    state.copy_(host)
    p = len(history) - 1
    cur, pos, err = ops.new_step_state(dev, batch=R)
    pos.copy_(torch.tensor([p + j for j in range(R)], dtype=torch.int32))
    token = torch.full((R,), -7, dtype=torch.int64, device=dev)
    x = torch.zeros(R, HID, dtype=torch.float16, device=dev)
    kept = torch.full((R, vocab), 7, dtype=torch.uint8, device=dev) if use_u else None
    before = smp.clone()

    def launch():
        ops.decode_tail_lookup_sample(logits, embed, token, pos, x, state, hist, tab, cur, smp, suppress=sup, u=u, kept_out=kept)
    if twin is not None:
        with _lib.routed_to(twin):
            launch()
    else:
        launch()
    torch.cuda.synchronize()
    n, new_hist, nxt, c_new = lookup_sample_ref.step(history, drafts, t, D, ngram, external, counter=c)
    st = state.tolist()
    assert st[ops.LOOKUP_ARGMAX:ops.LOOKUP_ARGMAX + R] == t, (st[ops.LOOKUP_ARGMAX:ops.LOOKUP_ARGMAX + R], t)
    assert st[ops.LOOKUP_ACCEPTED] == n and st[ops.LOOKUP_COUNT] == len(new_hist) and st[ops.LOOKUP_STEPS] == steps0 + 1 and st[ops.LOOKUP_TICKET] == 0
    assert hist[:len(new_hist)].tolist() == new_hist
    assert st[ops.LOOKUP_DRAFT + 1:ops.LOOKUP_DRAFT + 1 + D] == nxt, (st[ops.LOOKUP_DRAFT:ops.LOOKUP_DRAFT + 8], nxt)
    toks = [t[n]] + [min(max(d, 0), vocab - 1) for d in nxt]
    assert token.tolist() == toks
    assert torch.equal(x, embed[torch.tensor(toks, device=dev)])
    newp = [min(p + n + 1 + j, ROPE_ROWS) for j in range(R)]
    assert pos.tolist() == newp
    assert torch.equal(cur, tab[torch.tensor([min(q, ROPE_ROWS - 1) for q in newp], device=dev)])
    assert err.tolist() == [0] * R
    # the sampling block: the draw words moved on by n + 1 (a 64-bit add), every other word as it was, nobody counted in
    assert _counter(smp) == c_new == (c + n + 1) & ((1 << 64) - 1), (_counter(smp), c, n)
    after = smp.clone()
    after[SMP_DRAW:SMP_DRAW + 2] = before[SMP_DRAW:SMP_DRAW + 2]
    assert torch.equal(after, before) and int(smp[SMP_ARRIVE].item()) == 0
    if use_u:
        assert torch.equal(kept, kept_ref)
    return n, t


def _wrong(tok, vocab):
    return (tok + 1) % vocab


_LOGITS = {}


def _logits(vocab, R, scale):
    key = (vocab, R, scale)
    if key not in _LOGITS:
        import numpy as np
        rows = np.stack([sampling_ref.logits_row(vocab, scale, seed=1000 * R + 10 * j + int(scale)) for j in range(R)])
        _LOGITS[key] = torch.from_numpy(rows).to(_dev())
    return _LOGITS[key]


COUNTERS = (0, 5, (1 << 32) - 2)        # the last one crosses the 32-bit carry inside one step


@pytest.mark.parametrize("twin", [False, True], ids=["product", "safe"])
@pytest.mark.parametrize("R", [2, 4, 8])
@pytest.mark.parametrize("vocab", [1000, 32000, 128256])
def test_tail_draws_what_the_sampler_draws(vocab, R, twin):
    from amq_amd import _lib, ops
    lib = _lib.open_twin() if twin else None
    D = R - 1
    i = 0
    seen = set()
    for n in list(range(D + 1)) + ["hole"]:
        for scale in (1.0, 6.0):
            params = sampling_ref.GRID[(i + R) % len(sampling_ref.GRID)]
            c = COUNTERS[i % 3]
            use_u = i % 4 == 3
            i += 1
            lg = _logits(vocab, R, scale)
            if n == "hole":                             # a -1 draft in the middle stops the acceptance although the drafts behind it are right
                hole = D // 2
                make = lambda t: [t[k] if k != hole else -1 for k in range(D)]
                want = hole
            else:
                make = lambda t, n=n: [t[k] if k < n else _wrong(t[k], vocab) for k in range(D)]
                want = n
            # a history in which the emitted run's first token has occurred before: the proposal finds it
            got, t = _tail_case(ops, vocab, lg, params, c, [5, 6, 7, 8, 5], make, use_u=use_u, twin=lib)
            assert got == want, (got, want, t)
            hist2 = [5, t[0], 9, 11, 5]                  # ... ends in (5, t[0]) once t[0] is out: drafts 9, 11, 5, t[0], ...
            got, _ = _tail_case(ops, vocab, lg, params, c, hist2, make, ngram=2 + i % 3, use_u=use_u, twin=lib)
            assert got == want
            seen.add(c)
    assert seen == set(COUNTERS)


def test_tail_suppressed_nan_external_and_the_end_of_the_cache():
    from amq_amd import ops
    vocab, R = 1000, 4
    D = R - 1
    base = _logits(vocab, R, 1.0).clone()
    # a suppressed id that is the largest logit of every row is never drawn, and a draft of it is never accepted
    lg = base.clone()
    lg[:, 40] = 30.0
    lg[:, 41] = 29.0
    for params in ((1.0, 0, 1.0), (1.0, 1, 1.0), (0.8, 20, 0.9)):
        n, t = _tail_case(ops, vocab, lg, params, 5, [1, 2, 1, 2, 1], lambda t: [40, t[1], t[2]], suppress=(40, 41))
        assert n == 0 and 40 not in t and 41 not in t
        n, t = _tail_case(ops, vocab, lg, params, 5, [1, 2, 1, 2, 1], lambda t: [t[0], 41, t[2]], suppress=(40, 41), use_u=True)
        assert n == 1 and 40 not in t and 41 not in t
    # without the suppress list the same rows draw it (temperature 1, a gap of > 20: weight ~ 1)
    n, t = _tail_case(ops, vocab, lg, (1.0, 1, 1.0), 0, [1, 2, 1, 2, 1], lambda t: [40, 40, 40])
    assert n == 3 and t == [40] * 4
    # a row of NaNs draws token 0 (and a draft of 0 behind it is accepted)
    lg = base.clone()
    lg[1] = float("nan")
    n, t = _tail_case(ops, vocab, lg, (0.8, 20, 0.9), 0, [3, 4, 3], lambda t: [t[0], 0, _wrong(t[2], vocab)], use_u=True)
    assert t[1] == 0 and n == 2
    lg[:] = float("-inf")
    n, t = _tail_case(ops, vocab, lg, (1.0, 0, 1.0), (1 << 32) - 1, [3, 4, 3], lambda t: [0, 0, 7])
    assert t == [0] * 4 and n == 2
    # external mode: the tail proposes nothing
    n, _ = _tail_case(ops, vocab, base, (0.7, 50, 1.0), 5, [1, 2, 1, 2, 1], lambda t: list(t[:D]), external=True)
    assert n == D
    # the end of the cache: positions saturate at rope_rows; a history that fills history_cap exactly
    full = [(7 * i) % 5 for i in range(ROPE_ROWS - 3)]
    n, _ = _tail_case(ops, vocab, base[:3].contiguous(), (0.9, 200, 0.8), (1 << 32) - 2, full, lambda t: list(t[:2]))
    assert n == 2                                        # 45 + 3 tokens = history_cap; positions 47, 48, 48


# ------------------------------------------------------------------------------------------------------------------ 2. the runner
SEED = 77


def _run(m, ids, n, mode, sampler, ref=None, use_graph=False, seed=SEED):
    """prompt pass + sampled verify steps until n tokens are out; after EVERY step the draws are recomputed from the step's own logits rows (the
    trusted one-row sampler, draw counter c + j) and the emitted tokens, the accepted count and the counter must be what follows from them and the
    drafts the step ran with.  mode as in tests/test_gpu_lookup.py::_run.  -> (tokens [n], {emitted index: logits row that computed it}, steps)"""
    from amq_amd import ops
    S, D, R = ids.numel(), m.lookup, m.R
    m.reset()
    m.set_suppressed([SUP])
    m.set_lookup_mode(mode != "lookup")
    m.set_sampling(*sampler, seed=seed)                 # (writes the block: draw counter 0)
    m.prefill(ids, use_graph=use_graph)
    lg = m.logits.view(R, -1)
    first = _draws(ops, lg[:1], m.sample_state, 0, suppress=m.suppress)[0]
    count, steps_dev = m.lookup_sync()
    assert count == S + 1 and steps_dev == 0 and int(m.history[S].item()) == first and _counter(m.sample_state) == 1
    rows = {0: lg[0].clone()}
    steps = 0
    while count - S < n:
        e = count - S
        c = _counter(m.sample_state)
        assert c == e                                   # the token emitted at index i is drawn with counter i
        if mode == "never":
            drafts = [SUP] * D
            m.verify_step(drafts, use_graph=use_graph)
        elif mode == "right":
            d = ref[e:e + D].tolist()
            drafts = d + [-1] * (D - len(d))
            m.verify_step(drafts, use_graph=use_graph)
        else:
            drafts = m.lookup_state[ops.LOOKUP_DRAFT + 1:ops.LOOKUP_DRAFT + 1 + D].tolist()
            m.decode_step(use_graph)
        steps += 1
        count, _ = m.lookup_sync()
        acc = int(m.lookup_state[ops.LOOKUP_ACCEPTED].item())
        lg = m.logits.view(R, -1)
        t = _draws(ops, lg, m.sample_state, c, suppress=m.suppress)
        n_ref, emitted = lookup_ref.accept(drafts, t)
        assert acc == n_ref and count - S == e + acc + 1, (e, acc, n_ref, drafts, t)
        assert m.history[S + e:S + e + acc + 1].tolist() == emitted
        assert m.lookup_state[ops.LOOKUP_ARGMAX:ops.LOOKUP_ARGMAX + R].tolist() == t
        assert _counter(m.sample_state) == c + acc + 1
        for j in range(acc + 1):
            rows[e + j] = lg[j].clone()
    m.check()
    assert _counter(m.sample_state) == count - S        # draw counter == tokens emitted
    assert int(m.sample_state[SMP_ARRIVE].item()) == 0
    return m.history[S:S + n].to(torch.int64).clone(), rows, steps


def _equal_until_the_logits_part(name, ta, rows_a, tb, rows_b, n):
    """the tokens of two runs are equal up to the first emitted position at which the logits rows that computed it differ in bits (from there on the
    two runs draw from different distributions) -> that position, or None: the equality is total"""
    for e in range(n):
        if not torch.equal(rows_a[e].view(torch.int16), rows_b[e].view(torch.int16)):
            print(f"{name}: the logits rows of emitted position {e} differ in bits (max|diff| = "
                  f"{(rows_a[e].float() - rows_b[e].float()).abs().max().item():.3e}); tokens compared up to there")
            return e
        assert int(ta[e]) == int(tb[e]), (name, e, ta.tolist(), tb.tolist())
    print(f"{name}: every emitted position's logits row has the same bits in both runs; all {n} tokens equal")
    return None


RUNNERS = [    # (blocks, hidden, inter, heads, kv heads, D, max_seq)
    (2, 512, 1024, 4, 2, 4, 1024),          # grouped-query, R = 5: the split / rows kernels
    (1, 4096, 11008, 32, 32, 7, 128),       # 7B width, R = 8: the two-phase down_proj
]
SAMPLERS = [(0.8, 20, 0.9), (1.0, 0, 1.0)]


@pytest.mark.parametrize("nb,H,I,nh,nkv,D,max_seq", RUNNERS)
def test_the_runner_replays_its_own_decisions(nb, H, I, nh, nkv, D, max_seq):
    """every step's tokens, accepted count and counter follow from the step's own logits rows, drafts and counter (checked inside _run); never-accepted
    drafts take n - 1 steps; graph replay == eager; and across the three draft sources the tokens are equal up to the first emitted position at
    which the runs' logits rows differ in bits.  Always-right drafts take ceil((n - 1) / R) steps -- "always right" holds as long as the run's
    tokens are those of the never-accepted run the drafts were taken from, i.e. when that equality is total, so the count is asserted then (and the
    other case is printed)."""
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = dict(arch._cfg(nb, H, I, nh, nkv, 1, vocab=1024))
    R, n, S = D + 1, 34, 40
    ids = _prompt(S, 10, seed=D + nb)
    m = QuantLlama(cfg, None, device=DEV, max_seq=max_seq, seed=4, lookup=D, ngram_max=2, lookup_sampling=True)
    for sampler in SAMPLERS:
        tb, rows_b, steps_b = _run(m, ids, n, "never", sampler)
        assert steps_b == n - 1
        tc, rows_c, steps_c = _run(m, ids, n, "right", sampler, ref=tb)
        part_c = _equal_until_the_logits_part(f"R={R} H={H} {sampler} right/never", tc, rows_c, tb, rows_b, n)
        if part_c is None:
            assert torch.equal(tc, tb) and steps_c == math.ceil((n - 1) / R), (steps_c, n, R)
        ta, rows_a, steps_a = _run(m, ids, n, "lookup", sampler)
        part_a = _equal_until_the_logits_part(f"R={R} H={H} {sampler} lookup/never", ta, rows_a, tb, rows_b, n)
        stats = m.lookup_stats()
        assert stats["steps"] == steps_a <= n - 1 and stats["tokens"] >= n - 1
        print(f"R={R} H={H} {sampler}: steps never {steps_b} right {steps_c} lookup {steps_a}; parted: right {part_c} lookup {part_a}")
        # graph replay == eager, token for token (same runner, same seed), and the logits of every emitted position bit for bit
        tg, rows_g, steps_g = _run(m, ids, n, "right", sampler, ref=tb, use_graph=True)
        assert torch.equal(tg, tc) and steps_g == steps_c and all(torch.equal(rows_g[e], rows_c[e]) for e in rows_c)
        tl, _, steps_l = _run(m, ids, n, "lookup", sampler, use_graph=True)
        assert torch.equal(tl, ta) and steps_l == steps_a
        # generate(): the same loop from the public surface
        m.reset()
        m.set_lookup_mode(False)
        m.set_sampling(*sampler, seed=SEED)
        assert torch.equal(m.generate(ids, n), ta)
        assert _counter(m.sample_state) == m.lookup_sync()[0] - S
        m.check()
    m.set_sampling(None)


# ------------------------------------------------------------------------------------------------------------------ 3. proposals come true
def test_proposals_are_accepted_under_sampling_on_a_model_that_repeats():
    """the repeating model of tests/test_gpu_lookup.py (logit gap ~ 500: at temperature 1 every other token's weight rounds to 0 in 2^-40 fixed
    point, so the draw is the arg-max): the tokens follow sigma, the tail's own proposals come true"""
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = dict(arch._cfg(2, 512, 1024, 4, 4, 1, vocab=1024))
    g = torch.Generator().manual_seed(11)
    e = torch.randn(1024, 512, generator=g)
    sigma = torch.tensor([(t & ~3) | ((t + 1) & 3) for t in range(1024)])
    lm = torch.empty_like(e)
    lm[sigma] = e / 16.0
    ones = torch.ones(512, dtype=torch.float16)
    dense = dict(embed=(16.0 * e).half(), lm_head=lm.half(), norm=ones, ln1=[ones, ones], ln2=[ones, ones])
    D, n, S = 4, 41, 24
    ids = _prompt(S, 6, seed=2)
    m = QuantLlama(cfg, None, device=DEV, max_seq=128, seed=4, lookup=D, ngram_max=2, dense=dense, lookup_sampling=True)
    exp = [int(sigma[int(ids[-1])])]
    for _ in range(n - 1):
        exp.append(int(sigma[exp[-1]]))
    tb, _, steps_b = _run(m, ids, n, "never", (1.0, 0, 1.0))
    assert tb.tolist() == exp and steps_b == n - 1      # (the construction holds: the sampled model continues with sigma)
    ta, _, steps_a = _run(m, ids, n, "lookup", (1.0, 0, 1.0))
    stats = m.lookup_stats()
    assert ta.tolist() == exp
    assert steps_a < stats["tokens"] and steps_a < steps_b and stats["tokens"] / stats["steps"] > 1.0 and stats["mean_accepted"] > 0.0, stats
    assert steps_a <= 8 + math.ceil((n - 1 - 8) / (D + 1))      # once a period is in the history every draft is right
    m.set_sampling(None)


# ------------------------------------------------------------------------------------------------------------------ 4. the runner's surface
RECORDED = ("gemv_grouped", "gemv_grouped_sums", "rmsnorm", "silu_mul", "attn_decode", "attn_decode_rows", "gemm", "gemv_f16w", "decode_tail",
            "decode_tail_sample", "decode_tail_lookup", "decode_tail_lookup_sample")


def _record_step(m, sampled, monkeypatch):
    """one eager ``_step`` with pass-through recorders over the ops functions of RECORDED (the recorder of tests/test_gpu_step_plan.py) -> the names"""
    from amq_amd import ops
    calls = []

    def recorder(name, fn):
        def wrapped(*args, **kwargs):
            calls.append((name, len(args[1]) if name.startswith("gemv_grouped") else 0))
            return fn(*args, **kwargs)
        return wrapped

    with monkeypatch.context() as mp:
        for name in RECORDED:
            mp.setattr(ops, name, recorder(name, getattr(ops, name)))
        m._step(sampled)
        torch.cuda.synchronize()
    m.check()
    return calls


def test_runner_surface(monkeypatch):
    from amq_amd import arch
    from amq_amd.llama import DenseLlama, QuantLlama
    cfg = dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=1024))
    D, S, n = 3, 20, 24
    ids = _prompt(S, 7, seed=9)
    # a default lookup runner refuses sampling, with the words it always had; a sampling flag without lookup is refused at construction
    plain = QuantLlama(cfg, None, device=DEV, max_seq=64, seed=4, lookup=D)
    with pytest.raises(ValueError, match="rejection sampling"):
        plain.set_sampling(0.8)
    with pytest.raises(ValueError, match="greedy"):
        plain._tail(True)
    with pytest.raises(ValueError):
        QuantLlama(cfg, None, device=DEV, max_seq=64, lookup_sampling=True)
    with pytest.raises(ValueError):
        DenseLlama(cfg, device=DEV, max_seq=64, lookup=D)
    greedy_ref = plain.generate(ids, n)
    m = QuantLlama(cfg, None, device=DEV, max_seq=64, seed=4, lookup=D, lookup_sampling=True)
    greedy = m.generate(ids, n)
    assert torch.equal(greedy, greedy_ref)
    g1 = m.graph
    assert g1 is not None and m.sample_graph is None
    m.set_sampling(0.9, 30, 0.95, seed=1)
    a = m.generate(ids, n)
    s1 = m.sample_graph
    assert a.shape == (n,) and a.dtype == torch.int64 and s1 is not None and m.graph is g1
    assert torch.equal(m.generate(ids, n), a)                                # one seed: the same tokens
    assert torch.equal(m.generate(ids, n, use_graph=False), a)
    assert torch.equal(m.generate(ids, 9), a[:9])                            # another length: the captured step serves it
    m.set_sampling(0.9, 30, 0.95, seed=2)
    b = m.generate(ids, n)
    assert not torch.equal(a, b)                                             # another seed (24 draws from 30 candidates each)
    assert m.sample_graph is s1 and m.graph is g1
    m.check()
    # EOS stop under sampling: the output ends in the first EOS id and holds no EOS before min_new_tokens
    eos = int(b[6])
    first = int((b == eos).nonzero()[0])
    m.set_eos([eos])
    cut = m.generate(ids, n, stop_at_eos=True)
    assert torch.equal(cut, b[:first + 1])
    held = m.generate(ids, n, stop_at_eos=True, min_new_tokens=first + 3)
    # (holding the EOS id back changes every draw's candidates, so the tokens in front of it need not be b's)
    assert held.numel() >= first + 3 and eos not in held[:first + 3].tolist()
    if held.numel() < n:
        assert int(held[-1]) == eos and eos not in held[:-1].tolist()
    m.set_eos(())
    assert torch.equal(m.generate(ids, n), b)
    # one eager sampled verify step: the greedy step's launches except the last
    m.prefill(ids, use_graph=False)
    sampled_calls = _record_step(m, True, monkeypatch)
    m.set_sampling(None)
    m.prefill(ids, use_graph=False)
    greedy_calls = _record_step(m, False, monkeypatch)
    print(sampled_calls)
    assert greedy_calls[-1] == ("decode_tail_lookup", 0) and sampled_calls[-1] == ("decode_tail_lookup_sample", 0)
    assert sampled_calls[:-1] == greedy_calls[:-1] and len(greedy_calls) > 4
    # back to greedy: the greedy tokens, and the graph captured before
    assert torch.equal(m.generate(ids, n), greedy) and m.graph is g1 and m.sample_graph is s1
    m.check()
    # the other lookup surfaces under sampling: external drafts, ngram_max, stats
    m.set_sampling(0.9, 30, 0.95, seed=2)
    m.set_ngram_max(3)
    assert torch.equal(m.generate(ids, n), b)                                # (the proposals do not change the tokens)
    st = m.lookup_stats()
    assert st["tokens"] >= n - 1 and st["steps"] >= 1 and torch.equal(m.lookup_tokens()[:n], b)
    m.set_sampling(None)


# ------------------------------------------------------------------------------------------------------------------ 5. the HF surface
@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_sampled_prompt_lookup_generate_on_the_converted_object(family):
    pytest.importorskip("transformers")
    import transformers
    from amq_amd import hf_fast
    from amq_amd.patching import prepare_for_inference
    model = _swap_linears(_tiny(family))
    prepare_for_inference(model, backend="hip")
    S, n = 18, 20
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, 1000, (6,), generator=g).repeat(3)[None].to(DEV)
    kw = dict(prompt_lookup_num_tokens=3, do_sample=True, top_k=5, min_new_tokens=n, max_new_tokens=n, num_beams=1, pad_token_id=0)
    hf_takes_it = hasattr(transformers.GenerationConfig(), "prompt_lookup_num_tokens")

    def call(seed):
        torch.manual_seed(seed)
        with torch.inference_mode():
            return model.generate(ids, **kw)

    def through_hf():
        if hf_takes_it:
            out = call(0)
            assert out.shape == (1, S + n)
        else:
            with pytest.raises(ValueError):
                call(0)

    # either flag off: the call binds nothing and goes to HF's own generate
    hf_fast.convert_model_to_hip(model, lookup=True, sampling=False)
    through_hf()
    assert not any(isinstance(k, tuple) for k in hf_fast._RUNNERS.get(model, {}))
    hf_fast.convert_model_to_hip(model, lookup=False, sampling=True)
    through_hf()
    assert not any(isinstance(k, tuple) for k in hf_fast._RUNNERS.get(model, {}))
    # both on: served by the lookup runner
    hf_fast.convert_model_to_hip(model, lookup=True, sampling=True)
    a = call(1)
    lr = hf_fast._RUNNERS[model][("lookup", 3)]
    assert lr.lookup == 3 and lr.lookup_sampling and lr.sample_graph is not None
    assert [k for k in hf_fast._RUNNERS[model] if isinstance(k, tuple)] == [("lookup", 3)]
    assert a.shape == (1, S + n) and a.dtype == ids.dtype and torch.equal(a[:, :S], ids)
    eos = model.generation_config.eos_token_id
    eos = [] if eos is None else (list(eos) if isinstance(eos, (list, tuple)) else [eos])
    assert not any(int(t) in eos for t in a[0, S:])                           # fixed length: the EOS ids are never drawn
    assert torch.equal(call(1), a)                                           # reproducible under torch.manual_seed
    assert not torch.equal(call(2), a)                                       # another seed: 20 draws from 5 candidates each
    assert lr.sampling is None                                               # (set_sampling(None) in a finally)
    # an open-ended sampled call stops at the first EOS id; the same runner then serves a greedy lookup call
    stop_id = int(a[0, S + 4])

    def open_ended():
        torch.manual_seed(1)
        with torch.inference_mode():
            return model.generate(ids, **dict(kw, min_new_tokens=0, eos_token_id=stop_id))

    cut = open_ended()
    new = cut[0, S:]
    hits = (new == stop_id).nonzero()
    assert torch.equal(cut[:, :S], ids) and 1 <= new.numel() <= n
    assert (int(hits[0]) == new.numel() - 1) if hits.numel() else new.numel() == n
    assert torch.equal(open_ended(), cut) and lr.sampling is None
    with torch.inference_mode():
        greedy = model.generate(ids, prompt_lookup_num_tokens=3, do_sample=False, min_new_tokens=n, max_new_tokens=n, num_beams=1, pad_token_id=0)
    assert hf_fast._RUNNERS[model][("lookup", 3)] is lr and greedy.shape == (1, S + n) and lr.graph is not None
    hf_fast._RUNNERS.pop(model)
