"""GPU: prompt-lookup speculative decoding inside the captured token step.

The rows attention (amq_attn_decode_rows_f16) against successive batch-1 calls of amq_attn_decode_seq_f16; the verify-and-propose tail
(amq_decode_tail_lookup_f16) against tests/lookup_ref.py; the runner (QuantLlama(lookup=D)): drafts never change the output; against plain one-row
decoding; the runner's surface; the HF surface (convert_model_to_hip(model, lookup=True))."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev():
    return torch.device(DEV)


# ------------------------------------------------------------------------------------------------------------------ 1. the attention kernel
def _rows_state(ops, tab, max_seq, p, rows):
    cur, pos, err = ops.new_step_state(_dev(), batch=rows)
    positions = [p + j for j in range(rows)]
    pos.copy_(torch.tensor(positions, dtype=torch.int32))
    cur.copy_(tab.view(max_seq, 128)[torch.tensor([min(max(q, 0), max_seq - 1) for q in positions], device=_dev())])
    return cur, pos, err


def _oracle_rows(ops, tab, q, k, v, kc, vc, p, rows, max_seq, nh, nkv, n_splits):
    """`rows` successive batch-1 calls of amq_attn_decode_seq_f16, one per row, each appending its own cache row"""
    dev = _dev()
    kc_, vc_ = kc.clone(), vc.clone()
    out = torch.zeros(rows, nh * 128, dtype=torch.float16, device=dev)
    for j in range(rows):
        cur1, pos1, err1 = _rows_state(ops, tab, max_seq, p + j, 1)
        ops.attn_decode(q[j:j + 1].contiguous(), k[j:j + 1].contiguous(), v[j:j + 1].contiguous(), kc_, vc_, out[j:j + 1], pos1, nh, nkv, cur=cur1,
                        n_splits=n_splits)
        assert err1.tolist() == [0]
    return out, kc_, vc_


# (p, rows, max_seq, n_splits as ops takes it: 1 = one workgroup per (head, row), >= 2 the split kernel)
ROWS_CASES = [
    (0, 2, 384, 1), (0, 8, 384, 1), (37, 4, 384, 1), (200, 5, 384, 1), (376, 8, 384, 1), (382, 2, 384, 1),     # single workgroup; p = 0; p + rows = max_seq
    (0, 5, 2048, 8), (100, 4, 2048, 8), (250, 8, 2048, 8),                 # split, one active chunk (T <= 256); 250 + 8: rows 6, 7 open a second chunk
    (254, 4, 2048, 8), (700, 5, 2048, 8), (1500, 8, 2048, 8), (2040, 8, 2048, 8), (2046, 2, 2048, 6),          # several chunks; the end of the cache
]


@pytest.mark.parametrize("nh,nkv", [(4, 4), (4, 2), (32, 8)])
@pytest.mark.parametrize("p,rows,max_seq,n_splits", ROWS_CASES)
def test_attn_decode_rows_equals_successive_single_rows(nh, nkv, p, rows, max_seq, n_splits):
    from amq_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(1000 * p + 10 * rows + nh + nkv + max_seq)
    kc = torch.full((1, nkv, max_seq, 128), float("nan"), dtype=torch.float16, device=dev)     # rows >= p are NaN: never read from the cache
    vc = torch.full_like(kc, float("nan"))
    kc[0, :, :p] = torch.randn(nkv, p, 128, generator=g).half().to(dev)
    vc[0, :, :p] = torch.randn(nkv, p, 128, generator=g).half().to(dev)
    q = torch.randn(rows, nh * 128, generator=g).half().to(dev)
    k = torch.randn(rows, nkv * 128, generator=g).half().to(dev)
    v = torch.randn(rows, nkv * 128, generator=g).half().to(dev)
    tab = ops.rope_table(max_seq, 10000.0, dev)
    # the oracle in the same form; grouped-query models over a split cache would take the matrix-core kernel there (other arithmetic), so their oracle
    # is the single-workgroup form -- the bits the per-head split kernel reproduces with one active chunk
    gqa_split = nh != nkv and n_splits > 1
    ref, kc_r, vc_r = _oracle_rows(ops, tab, q, k, v, kc, vc, p, rows, max_seq, nh, nkv, 1 if gqa_split else n_splits)

    def run():
        kc_, vc_ = kc.clone(), vc.clone()
        out = torch.zeros(rows, nh * 128, dtype=torch.float16, device=dev)
        cur, pos, err = _rows_state(ops, tab, max_seq, p, rows)
        ops.attn_decode_rows(q, k, v, kc_, vc_, out, cur, pos, nh, nkv, n_splits=n_splits)
        assert err.tolist() == [0] * rows and pos.tolist() == [p + j for j in range(rows)]
        return out, kc_, vc_

    got, kc_g, vc_g = run()
    assert torch.isfinite(got.float()).all()
    assert torch.equal(kc_g[0, :, :p + rows], kc_r[0, :, :p + rows]) and torch.equal(vc_g[0, :, :p + rows], vc_r[0, :, :p + rows])
    assert torch.isnan(kc_g[0, :, p + rows:]).all() and torch.isnan(vc_g[0, :, p + rows:]).all()
    for j in range(rows):
        T = p + j + 1
        chunk = max(256, (-(-T // n_splits) + 31) // 32 * 32) if n_splits > 1 else T
        one_chunk = -(-T // chunk) == 1
        err = (got[j].float() - ref[j].float()).abs().max().item()
        print(f"rows attention nh={nh} nkv={nkv} p={p} row={j} splits={n_splits} one_chunk={one_chunk} max|diff|={err:.3e}")
        if one_chunk:
            assert torch.equal(got[j], ref[j]), (j, err)
        else:
            assert err <= 2e-3 * ref[j].float().abs().max().item() + 1e-3, (j, err)
    again, _, _ = run()
    assert torch.equal(again, got)
    assert all(int(t.abs().sum().item()) == 0 for t in ops._ATTN_TICKETS._cur.values())


@pytest.mark.parametrize("max_seq,n_splits", [(384, 1), (2048, 8)])
def test_attn_decode_rows_out_of_range_row_is_that_rows_no_op(max_seq, n_splits):
    from amq_amd import ops
    dev, nh, nkv, rows = _dev(), 4, 2, 4
    p = max_seq - 2                                   # rows 0, 1 fit; rows 2, 3 are at max_seq, max_seq + 1 (the tail saturates them at max_seq)
    g = torch.Generator().manual_seed(3)
    kc = torch.randn(1, nkv, max_seq, 128, generator=g).half().to(dev)
    vc = torch.randn(1, nkv, max_seq, 128, generator=g).half().to(dev)
    q = torch.randn(rows, nh * 128, generator=g).half().to(dev)
    k = torch.randn(rows, nkv * 128, generator=g).half().to(dev)
    v = torch.randn(rows, nkv * 128, generator=g).half().to(dev)
    tab = ops.rope_table(max_seq, 10000.0, dev)
    ref, kc_r, vc_r = _oracle_rows(ops, tab, q, k, v, kc, vc, p, 2, max_seq, nh, nkv, 1)
    cur, pos, err = _rows_state(ops, tab, max_seq, p, rows)
    pos[2:].fill_(max_seq)
    out = torch.full((rows, nh * 128), 7.0, dtype=torch.float16, device=dev)
    kc_, vc_ = kc.clone(), vc.clone()
    ops.attn_decode_rows(q, k, v, kc_, vc_, out, cur, pos, nh, nkv, n_splits=n_splits)
    assert err.tolist() == [0, 0, 1, 1]
    assert torch.equal(kc_, kc_r) and torch.equal(vc_, vc_r)
    assert bool((out[2:] == 7.0).all())
    for j in range(2):
        assert (out[j].float() - ref[j].float()).abs().max() <= 2e-3 * ref[j].float().abs().max() + 1e-3
    with pytest.raises(ops._lib.AmqError):
        ops.check_step_state(err)
    # a row whose row 0 would sit below position 0 is refused the same way
    cur, pos, err = _rows_state(ops, tab, max_seq, 0, rows)
    pos.copy_(torch.tensor([0, 0, 2, 3], dtype=torch.int32))           # row 1 claims position 0: its row 0 would be at -1
    ops.attn_decode_rows(q, k, v, kc.clone(), vc.clone(), out, cur, pos, nh, nkv, n_splits=n_splits)
    assert err.tolist() == [0, 1, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ 2. the tail kernel
VOCAB, HID, ROPE_ROWS = 64, 16, 48


def _tail_case(ops, D, history, drafts, argmaxes, ngram, external=False, suppress=(), ties=False, steps0=3, cap=ROPE_ROWS):
    dev, R = _dev(), D + 1
    g = torch.Generator().manual_seed(len(history) * 31 + D)
    embed = torch.randn(VOCAB, HID, generator=g).half().to(dev)
    tab = torch.randn(ROPE_ROWS, 128, generator=g).half().to(dev)
    logits = torch.zeros(R, VOCAB, dtype=torch.float16)
    for j, a in enumerate(argmaxes):
        logits[j, a] = 5.0
        if ties and a + 3 < VOCAB:
            logits[j, a + 3] = 5.0                   # a later equal maximum: the first one wins
        for s in suppress:
            logits[j, s] = 9.0                       # a suppressed id as the maximum of every row
    logits = logits.to(dev)
    state, hist = ops.new_lookup_state(dev, D, ngram, cap)
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
    sup = torch.tensor(list(suppress) + [-1] * (8 - len(suppress)), dtype=torch.int32, device=dev) if suppress else None
    ops.decode_tail_lookup(logits, embed, token, pos, x, state, hist, tab, cur, suppress=sup)
    torch.cuda.synchronize()
    n, new_hist, nxt = lookup_ref.step(history, drafts, argmaxes, D, ngram, external)
    st = state.tolist()
    assert st[ops.LOOKUP_ACCEPTED] == n and st[ops.LOOKUP_COUNT] == len(new_hist) and st[ops.LOOKUP_STEPS] == steps0 + 1 and st[ops.LOOKUP_TICKET] == 0
    assert hist[:len(new_hist)].tolist() == new_hist
    assert st[ops.LOOKUP_DRAFT + 1:ops.LOOKUP_DRAFT + 1 + D] == nxt, (st[ops.LOOKUP_DRAFT:ops.LOOKUP_DRAFT + 8], nxt)
    assert st[ops.LOOKUP_ARGMAX:ops.LOOKUP_ARGMAX + R] == list(argmaxes)
    toks = [argmaxes[n]] + [min(max(d, 0), VOCAB - 1) for d in nxt]
    assert token.tolist() == toks
    assert torch.equal(x, embed[torch.tensor(toks, device=dev)])
    newp = [min(p + n + 1 + j, ROPE_ROWS) for j in range(R)]
    assert pos.tolist() == newp
    assert torch.equal(cur, tab[torch.tensor([min(q, ROPE_ROWS - 1) for q in newp], device=dev)])
    assert err.tolist() == [0] * R
    return n


def test_tail_every_acceptance_count_and_the_proposal():
    from amq_amd import ops
    for D in (1, 3, 4, 7):
        hist = [3, 9, 4, 11, 3, 9, 4, 12, 20, 21][:6 + D % 3]
        am = [10 + j for j in range(D + 1)]
        for n in range(D + 1):                         # the first n drafts right, the next one wrong
            drafts = [am[i] if i < n else 63 for i in range(D)]
            assert _tail_case(ops, D, hist, drafts, am, 2) == n
        assert _tail_case(ops, D, hist, [-1] * D, am, 2) == 0
    # a -1 draft in the middle stops the acceptance although the drafts behind it are right
    assert _tail_case(ops, 4, [1, 2, 3], [10, -1, 12, 13], [10, 11, 12, 13, 14], 2) == 1
    # the proposal: most recent of two matches; a continuation shorter than D; g = 1 only; nothing; external mode
    assert _tail_case(ops, 2, [1, 2, 8, 8, 1, 2, 9, 9, 1], [-1, -1], [2, 0, 0], 2) == 0            # history ends 1, 2 -> [9, 9]
    assert _tail_case(ops, 4, [3, 4, 6, 3], [4, 6, 3, 4], [4, 6, 3, 4, 0], 3) == 4
    assert _tail_case(ops, 3, [5, 1, 7, 9, 2], [-1] * 3, [1, 0, 0, 0], 4) == 0
    assert _tail_case(ops, 3, [5, 6, 7], [-1] * 3, [8, 0, 0, 0], 2) == 0
    assert _tail_case(ops, 3, [1, 2, 1, 2, 1], [2, 1, 2], [2, 1, 2, 1], 2, external=True) == 3
    # a suppressed id as the maximum of every row; first-maximum ties
    assert _tail_case(ops, 3, [1, 2, 1, 2, 1], [2, 1, 5], [2, 1, 2, 1], 2, suppress=(40, 41)) == 2
    assert _tail_case(ops, 3, [1, 2, 1, 2, 1], [2, 1, 2], [2, 1, 2, 1], 2, ties=True) == 3
    # the end of the cache: positions saturate at rope_rows; a history that fills history_cap exactly
    full = [(7 * i) % 5 for i in range(ROPE_ROWS - 3)]
    assert _tail_case(ops, 2, full, [1, 1], [1, 1, 0], 2) == 2             # 45 + 3 tokens = history_cap; positions 47, 48, 48


def test_tail_random_histories():
    import random
    from amq_amd import ops
    rng = random.Random(7)
    for _ in range(40):
        D, g = rng.randint(1, 7), rng.randint(1, 4)
        hist = [rng.randrange(4) for _ in range(rng.randint(1, 30))]
        am = [rng.randrange(4) for _ in range(D + 1)]
        drafts = [rng.choice([am[i], am[i], rng.randrange(4), -1]) for i in range(D)]
        _tail_case(ops, D, hist, drafts, am, g)


# ------------------------------------------------------------------------------------------------------------------ 3. / 4. the runner
SUP = 5             # an id listed in suppress_ids: the arg-max never takes it, so a draft of it is never accepted


def _prompt(S, seg, seed, vocab=1024):
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(8, vocab, (seg,), generator=g)
    return s.repeat(-(-S // seg))[:S].to(_dev())


def _run(m, ids, n, mode, ref=None, use_graph=False):
    """prompt pass + verify steps until n tokens are out.  mode: "lookup" (the tail proposes), "never" (external drafts never accepted), "right"
    (external drafts taken from ``ref``: always right).  -> (tokens [n], {emitted index: logits of the row that computed it}, steps)"""
    S, D = ids.numel(), m.lookup
    m.reset()
    m.set_suppressed([SUP])
    m.set_lookup_mode(mode != "lookup")
    m.prefill(ids, use_graph=use_graph)
    rows = {0: m.logits.view(m.R, -1)[0].float().clone()}
    row0 = set()
    count, _ = m.lookup_sync()
    steps = 0
    while count - S < n:
        e = count - S
        if mode == "never":
            m.verify_step([SUP] * D, use_graph=use_graph)
        elif mode == "right":
            d = ref[e:e + D].tolist()
            m.verify_step(d + [-1] * (D - len(d)), use_graph=use_graph)
        else:
            m.decode_step(use_graph)
        steps += 1
        count, _ = m.lookup_sync()
        acc = int(m.lookup_state[5].item())
        assert count - S == e + acc + 1
        lg = m.logits.view(m.R, -1).float()
        for j in range(acc + 1):
            rows[e + j] = lg[j].clone()
        row0.add(e)
    m.check()
    return m.history[S:S + n].to(torch.int64).clone(), rows, row0, steps


RUNNERS = [    # (blocks, hidden, inter, heads, kv heads, D, max_seq)
    (2, 512, 1024, 4, 4, 1, 128),
    (2, 512, 1024, 4, 2, 4, 1024),          # grouped-query, R = 5, a cache long enough for the split kernel
    (1, 4096, 11008, 32, 32, 3, 128),       # 7B width, R = 4
    (1, 4096, 11008, 32, 32, 7, 128),       # ... R = 8: the two-phase down_proj
]


@pytest.mark.parametrize("nb,H,I,nh,nkv,D,max_seq", RUNNERS)
def test_drafts_do_not_change_the_output(nb, H, I, nh, nkv, D, max_seq):
    """the central property: whatever is proposed -- looked up, never right, always right -- the tokens are the same, and so are the logits of every
    emitted position that is row 0 of a step in two of the runs; always-right drafts take ceil((n - 1) / R) steps, never-right ones n - 1; graph
    replay == eager; then the same tokens through a plain one-row runner (check 4)"""
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = dict(arch._cfg(nb, H, I, nh, nkv, 1, vocab=1024))
    R, n, S = D + 1, 34, 40
    ids = _prompt(S, 10, seed=D + nb)
    m = QuantLlama(cfg, None, device=DEV, max_seq=max_seq, seed=4, lookup=D, ngram_max=2)
    tb, rows_b, row0_b, steps_b = _run(m, ids, n, "never")
    assert steps_b == n - 1 and sorted(row0_b) == list(range(1, n))
    tc, rows_c, row0_c, steps_c = _run(m, ids, n, "right", ref=tb)
    assert torch.equal(tc, tb), (tc.tolist(), tb.tolist())
    assert steps_c == math.ceil((n - 1) / R), (steps_c, n, R)
    ta, rows_a, row0_a, steps_a = _run(m, ids, n, "lookup")
    assert torch.equal(ta, tb)
    stats = m.lookup_stats()
    # (bookkeeping only -- near a tautology: a random-weight model does not copy its prompt, so nothing here says the proposals come true.  The
    #  "more than one token per step" check is test_lookup_proposals_are_accepted_on_a_model_that_repeats, on a model built to repeat.)
    assert stats["steps"] == steps_a <= n - 1 and (steps_a < steps_b) == (stats["mean_accepted"] > 0) and stats["tokens"] >= n - 1
    for run0, rows in ((row0_a, rows_a), (row0_c, rows_c)):
        for e in run0:
            if e < n:
                assert torch.equal(rows[e], rows_b[e]), (e, (rows[e] - rows_b[e]).abs().max().item())
    # graph replay == eager, bit for bit (tokens and the logits of every row-0 position)
    tg, rows_g, row0_g, steps_g = _run(m, ids, n, "right", ref=tb, use_graph=True)
    assert torch.equal(tg, tb) and steps_g == steps_c and all(torch.equal(rows_g[e], rows_c[e]) for e in rows_c)
    m.reset()
    m.set_lookup_mode(False)
    assert torch.equal(m.generate(ids, n), tb)
    m.check()
    # check 4: a plain batch-1 runner FED these tokens: logits within 1e-2 max|ref| at EVERY emitted position (rows 1 .. D of the always-right run
    # included), its own greedy choice agreeing on >= 0.8 of the steps
    m1 = QuantLlama(cfg, None, device=DEV, max_seq=max_seq, seed=4)
    m1.set_suppressed([SUP])
    m1.prefill(ids, use_graph=False)
    own, worst = [], 0.0
    for i in range(n):
        ref = m1.logits.float()
        for rows in (rows_b, rows_c):
            err = (rows[i] - ref).abs().max().item()
            worst = max(worst, err / ref.abs().max().item())
            assert err <= 1e-2 * ref.abs().max().item(), (i, err, ref.abs().max().item())
        own.append(int(m1.token.item()))
        if i + 1 < n:
            m1.set_token(tb[i:i + 1].contiguous())
            m1.decode_step(use_graph=False)
    print(f"lookup R={R} H={H}: worst |logits - plain| / max|plain| = {worst:.3e}")
    assert (torch.tensor(own, device=tb.device) == tb).float().mean().item() >= 0.8


def test_lookup_proposals_are_accepted_on_a_model_that_repeats():
    """a model built to continue every token t with sigma(t) (embedding rows far larger than what the blocks add, lm_head row sigma(t) = embed row
    t; sigma has cycles of 4): whatever the prompt, its greedy output is periodic, so the tail's own proposals come true: more than one token per
    step, fewer steps than tokens, and still the tokens of the never-accepted run"""
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
    m = QuantLlama(cfg, None, device=DEV, max_seq=128, seed=4, lookup=D, ngram_max=2, dense=dense)
    tb, _, _, steps_b = _run(m, ids, n, "never")
    exp = [int(sigma[int(ids[-1])])]
    for _ in range(n - 1):
        exp.append(int(sigma[exp[-1]]))
    assert tb.tolist() == exp                           # (the construction holds: the model continues with sigma)
    ta, _, _, steps_a = _run(m, ids, n, "lookup")
    stats = m.lookup_stats()
    assert torch.equal(ta, tb) and steps_b == n - 1
    assert steps_a < steps_b and stats["tokens"] / stats["steps"] > 1.0 and stats["mean_accepted"] > 0.0, stats
    assert steps_a <= 8 + math.ceil((n - 1 - 8) / (D + 1))      # once a period is in the history every draft is right


# ------------------------------------------------------------------------------------------------------------------ 5. the runner's surface
def test_runner_surface():
    from amq_amd import arch
    from amq_amd.llama import DenseLlama, QuantLlama
    cfg = dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=1024))
    D, S, n = 3, 20, 24
    ids = _prompt(S, 7, seed=9)
    m = QuantLlama(cfg, None, device=DEV, max_seq=64, seed=4, lookup=D)
    out = m.generate(ids, n)
    assert out.shape == (n,) and out.dtype == torch.int64
    g1 = m.graph
    assert g1 is not None
    m.reset()
    assert torch.equal(m.generate(ids, n), out)                              # reset, then the same tokens
    short = m.generate(ids, 9)
    assert torch.equal(short, out[:9]) and m.graph is g1                     # another length: the captured step serves it
    assert torch.equal(m.generate(ids, n, use_graph=False), out)
    m.check()
    # EOS: truncated at the first EOS id; min_new_tokens holds it back
    eos = int(out[6])
    first = int((out == eos).nonzero()[0])
    m.set_eos([eos])
    cut = m.generate(ids, n, stop_at_eos=True)
    assert torch.equal(cut, out[:first + 1])
    held = m.generate(ids, n, stop_at_eos=True, min_new_tokens=first + 3)
    assert held.numel() >= first + 3 and eos not in held[:first + 3].tolist()
    assert torch.equal(held[:first], out[:first])
    m.set_eos(())
    assert torch.equal(m.generate(ids, n), out)
    # a request past the cache
    with pytest.raises(ValueError):
        m.generate(ids, 64 - S - D + 1)
    m.generate(ids, 64 - S - D)
    m.check()
    # what a lookup runner refuses, each with its reason
    for kw in (dict(batch=2), dict(ragged=True), dict(engine=True), dict(lookup=8), dict(ngram_max=5)):
        with pytest.raises(ValueError):
            QuantLlama(cfg, None, device=DEV, max_seq=64, **{"lookup": D, **kw})
    with pytest.raises(ValueError):
        m.set_sampling(0.8)
    with pytest.raises(ValueError):
        m.prefill(ids, start_pos=4)
    with pytest.raises(ValueError):
        DenseLlama(cfg, device=DEV, max_seq=64, lookup=D)
    with pytest.raises(ValueError):
        QuantLlama(cfg, None, device=DEV, max_seq=64).verify_step([1, 2, 3])

    class Fused(QuantLlama):
        FUSE_QKV_ATTN = True
    with pytest.raises(ValueError):
        Fused(cfg, None, device=DEV, max_seq=64, lookup=D)


# ------------------------------------------------------------------------------------------------------------------ 6. the HF surface
NAMES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _swap_linears(model, bits_cycle=(4, 2, 3, 3, 2, 4, 3), seed=100):
    from amq_amd.hqq_format import random_hqq
    from amq_amd.patching import HQQWeightsModule
    i = 0
    for layer in model.model.layers:
        for parent in (layer.self_attn, layer.mlp):
            for name in NAMES:
                lin = getattr(parent, name, None)
                if lin is None:
                    continue
                n, k = lin.weight.shape
                h = random_hqq(n, k, bits_cycle[i % len(bits_cycle)], seed=seed + i)
                i += 1
                h.bias = None if lin.bias is None else lin.bias.data.detach().clone()
                setattr(parent, name, HQQWeightsModule(h.to(torch.device(DEV))))
    return model


def _tiny(family, layers=2):
    torch.manual_seed(0)
    if family == "llama":
        from transformers import LlamaConfig, LlamaForCausalLM
        cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=layers, num_attention_heads=2, num_key_value_heads=1,
                          vocab_size=1000, max_position_embeddings=256, rms_norm_eps=1e-5, attn_implementation="eager")
        m = LlamaForCausalLM(cfg)
    else:
        from transformers import Qwen2Config, Qwen2ForCausalLM
        cfg = Qwen2Config(hidden_size=896, intermediate_size=640, num_hidden_layers=layers, num_attention_heads=7, num_key_value_heads=1,
                          vocab_size=1000, max_position_embeddings=256, rms_norm_eps=1e-6, attn_implementation="eager", rope_theta=1000000.0,
                          tie_word_embeddings=False)
        m = Qwen2ForCausalLM(cfg)
        with torch.no_grad():
            for layer in m.model.layers:
                for nm in ("q_proj", "k_proj", "v_proj"):
                    getattr(layer.self_attn, nm).bias.normal_(0.0, 0.1)
    return m.to(torch.float16).to(DEV).eval()


def _same_new_tokens_or_a_tie(model, row, fast_new, slow_new, eos=None):
    """two fp16 implementations of one function decode greedily: equal tokens, or -- at the first step where they part -- a near-tie under HF's own
    logits for the common prefix (what follows a parted step is not comparable)"""
    diff = (fast_new != slow_new).nonzero()
    if len(diff) == 0:
        return
    t = int(diff[0])
    with torch.inference_mode():
        lg = model(torch.cat([row, slow_new[:t]])[None]).logits[0, -1].float()
        if eos is not None:
            lg[eos] = float("-inf")
    gap = float(lg.max() - lg[int(fast_new[t])])
    assert gap <= 4e-3 * float(lg[torch.isfinite(lg)].abs().max()), (t, gap, fast_new.tolist(), slow_new.tolist())


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_prompt_lookup_generate_on_the_converted_object(family):
    pytest.importorskip("transformers")
    from amq_amd import hf_fast
    from amq_amd.patching import prepare_for_inference
    model = _swap_linears(_tiny(family))
    prepare_for_inference(model, backend="hip")
    eos = model.generation_config.eos_token_id
    S, n = 18, 20
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, 1000, (6,), generator=g).repeat(3)[None].to(DEV)
    kw = dict(min_new_tokens=n, max_new_tokens=n, do_sample=False, num_beams=1, pad_token_id=0)
    # decided beforehand, from transformers itself: does its generate know the argument?  Where it does, HF's own calls below run unguarded (an error
    # in the fused modules under HF's assisted-decoding loop is a failure of this test); where it does not, HF refuses the unknown argument with a
    # ValueError, and exactly that is expected of the calls that fall through
    import transformers
    hf_takes_it = hasattr(transformers.GenerationConfig(), "prompt_lookup_num_tokens")

    def through_hf(k):
        with torch.inference_mode():
            if hf_takes_it:
                return model.generate(ids, prompt_lookup_num_tokens=k, **kw)
            with pytest.raises(ValueError):
                model.generate(ids, prompt_lookup_num_tokens=k, **kw)
        return None

    hf_lookup = through_hf(3)                           # HF's own prompt lookup on the unconverted modules
    hf_fast.convert_model_to_hip(model)
    with torch.inference_mode():
        plain = model.generate(ids, **kw)
    assert set(hf_fast._RUNNERS[model]) == {1}
    # without lookup=True the call falls through: no lookup runner is bound
    through_hf(3)
    assert set(hf_fast._RUNNERS[model]) == {1}
    hf_fast.convert_model_to_hip(model, lookup=True)
    with torch.inference_mode():
        fast = model.generate(ids, prompt_lookup_num_tokens=3, **kw)
        fast2 = model.generate(ids, prompt_lookup_num_tokens=3, max_matching_ngram_size=3, **kw)
    lr = hf_fast._RUNNERS[model][("lookup", 3)]        # one runner per k: g is a word of its device block
    assert lr.lookup == 3 and lr.ngram_max == 3 and int(lr.lookup_state[1].item()) == 3
    assert [k for k in hf_fast._RUNNERS[model] if isinstance(k, tuple)] == [("lookup", 3)]
    assert fast.shape == (1, S + n) and fast.dtype == ids.dtype and torch.equal(fast[:, :S], ids)
    _same_new_tokens_or_a_tie(model, ids[0], fast[0, S:], plain[0, S:], eos)
    _same_new_tokens_or_a_tie(model, ids[0], fast2[0, S:], plain[0, S:], eos)
    assert torch.equal(fast[0, S:S + 3], plain[0, S:S + 3])
    if hf_lookup is not None:
        _same_new_tokens_or_a_tie(model, ids[0], fast[0, S:], hf_lookup[0, S:], eos)
    # calls the predicate refuses go to HF's own generate and bind nothing
    before = set(hf_fast._RUNNERS[model])
    through_hf(9)
    assert set(hf_fast._RUNNERS[model]) == before
    # ... and so does a call whose draft rows would pass max_position_embeddings (256) although prompt + new tokens fit: HF serves it
    if hf_takes_it:
        room = 256 - S - 2                              # S + n = 254 fits; + 3 draft rows = 257 does not
        with torch.inference_mode():
            far = model.generate(ids, prompt_lookup_num_tokens=3, min_new_tokens=room, max_new_tokens=room, do_sample=False, num_beams=1, pad_token_id=0)
        assert far.shape == (1, 254) and set(hf_fast._RUNNERS[model]) == before
    hf_fast._RUNNERS.pop(model)
