"""GPU: batched decode over prompts of unequal length -- every sequence at a position of its own.

Kernels (amq_attn_decode_seq_f16, amq_decode_tail_seq_f16, amq_decode_tail_sample_seq_f16, amq_set_token_seq_f16) against the shared-position
entry points run on each sequence alone; the ragged runner (QuantLlama(ragged=True)) against batch-1 runs on the un-padded prompts and against the
plain batched runner; the HF surface (convert_model_to_hip(model, padded=True)) against HF's own generate with the same left-padding mask."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev():
    return torch.device(DEV)


def _rope_ref(t, pos):
    inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32, device=t.device) / 128.0))
    fr = torch.tensor([float(pos)], device=t.device)[:, None] * inv[None, :]
    emb = torch.cat([fr, fr], -1)
    cos, sin = emb.cos().half(), emb.sin().half()
    rot = torch.cat([-t[..., 64:], t[..., :64]], -1)
    return t * cos + rot * sin


def _seq_state(ops, tab, max_seq, positions):
    cur, pos, err = ops.new_step_state(_dev(), batch=len(positions))
    pos.copy_(torch.tensor(positions, dtype=torch.int32))
    cur.copy_(tab.view(max_seq, 128)[torch.tensor([min(max(p, 0), max_seq - 1) for p in positions], device=_dev())])
    return cur, pos, err


def _attn_inputs(positions, max_seq, nh, nkv, seed):
    """caches whose rows at and beyond each sequence's position are NaN: they must never contribute (the new token's row is written by the call)"""
    dev, B = _dev(), len(positions)
    g = torch.Generator().manual_seed(seed)
    kc = torch.full((B, nkv, max_seq, 128), float("nan"), dtype=torch.float16, device=dev)
    vc = torch.full_like(kc, float("nan"))
    for b, p in enumerate(positions):
        kc[b, :, :p] = torch.randn(nkv, p, 128, generator=g).half().to(dev)
        vc[b, :, :p] = torch.randn(nkv, p, 128, generator=g).half().to(dev)
    q = torch.randn(B, nh * 128, generator=g).half().to(dev)
    k = torch.randn(B, nkv * 128, generator=g).half().to(dev)
    v = torch.randn(B, nkv * 128, generator=g).half().to(dev)
    return kc, vc, q, k, v


ATTN_CASES = [
    ((5, 200, 383, 0), 384, 4, 4, 1),               # one workgroup per head (max_seq <= 512)
    ((17, 300, 0), 512, 8, 2, 1),                   # ... grouped heads sharing a kv head, three sequences
    ((100, 700, 1500, 2047), 2048, 8, 8, 8),        # split kernel: one sequence inside one chunk, others over several, the last cache row
    ((255, 256, 1023), 2048, 4, 4, 6),              # ... T = 256 / 257: the second chunk holds only the new token
    ((100, 700, 1500, 2047), 2048, 8, 2, 8),        # grouped-query kernel (nh / nkv = 4) and its combine launch
    ((0, 63, 64, 3000), 4096, 16, 4, 16),           # ... the first token of a sequence beside a long one
]


@pytest.mark.parametrize("positions,max_seq,nh,nkv,n_splits", ATTN_CASES)
def test_attn_decode_seq_equals_each_sequence_alone(positions, max_seq, nh, nkv, n_splits):
    """sequence b of amq_attn_decode_seq_f16 == the shared-position entry point on that sequence alone at pos[b], bit for bit (output, appended
    row, untouched rest of the cache); finite although every unused row is NaN; the eager fp32 formula; determinism; tickets left zero"""
    from amq_amd import ops
    dev, B = _dev(), len(positions)
    kc, vc, q, k, v = _attn_inputs(positions, max_seq, nh, nkv, seed=7 * sum(positions) + max_seq + nh)
    tab = ops.rope_table(max_seq, 10000.0, dev)

    def run_seq():
        kc_, vc_ = kc.clone(), vc.clone()
        out = torch.zeros(B, nh * 128, dtype=torch.float16, device=dev)
        cur, pos, err = _seq_state(ops, tab, max_seq, positions)
        ops.attn_decode(q, k, v, kc_, vc_, out, pos, nh, nkv, cur=cur, n_splits=n_splits)
        assert err.tolist() == [0] * B and pos.tolist() == list(positions)
        ops.check_step_state(err)
        return out, kc_, vc_

    got, kc_g, vc_g = run_seq()
    assert torch.isfinite(got.float()).all()
    for b, p in enumerate(positions):
        kc1, vc1 = kc[b:b + 1].clone(), vc[b:b + 1].clone()
        out1 = torch.zeros(1, nh * 128, dtype=torch.float16, device=dev)
        cur1, pos1, err1 = ops.new_step_state(dev)
        cur1.copy_(tab.view(max_seq, 128)[p]); pos1.fill_(p)
        ops.attn_decode(q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), kc1, vc1, out1, pos1, nh, nkv, cur=cur1,
                        n_splits=n_splits)
        assert int(err1.item()) == 0
        assert torch.equal(got[b], out1[0]), (b, p, (got[b].float() - out1[0].float()).abs().max().item())
        assert torch.equal(kc_g[b, :, :p + 1], kc1[0, :, :p + 1]) and torch.equal(vc_g[b, :, :p + 1], vc1[0, :, :p + 1])
        assert torch.isnan(kc_g[b, :, p + 1:]).all() and torch.isnan(vc_g[b, :, p + 1:]).all()      # nothing written behind the new row
        # the appended row: HF's rotation of the new key, the raw value
        assert torch.equal(kc_g[b, :, p], _rope_ref(k[b].view(nkv, 128), p)) and torch.equal(vc_g[b, :, p], v[b].view(nkv, 128))
        # eager fp32 formula over the sequence's own rows
        K = kc_g[b, :, :p + 1].repeat_interleave(nh // nkv, 0).float()
        V = vc_g[b, :, :p + 1].repeat_interleave(nh // nkv, 0).float()
        qr = _rope_ref(q[b].view(nh, 128), p).float()
        w = torch.einsum("hd,htd->ht", qr, K) * (128 ** -0.5)
        ref = torch.einsum("ht,htd->hd", torch.softmax(w, -1), V).reshape(-1)
        assert (got[b].float() - ref).abs().max() <= 4e-3 * ref.abs().max() + 1e-3, (b, p)
    again, kc_a, vc_a = run_seq()
    assert torch.equal(again, got)
    assert all(int(t.abs().sum().item()) == 0 for t in ops._ATTN_TICKETS._cur.values())


@pytest.mark.parametrize("pos,max_seq,nh,nkv,batch,n_splits", [(200, 384, 4, 4, 3, 1), (1500, 2048, 8, 8, 3, 8), (1500, 2048, 8, 2, 4, 8)])
def test_attn_decode_seq_with_equal_positions_is_the_shared_position_launch(pos, max_seq, nh, nkv, batch, n_splits):
    from amq_amd import ops
    dev = _dev()
    kc, vc, q, k, v = _attn_inputs([pos] * batch, max_seq, nh, nkv, seed=pos + nh)
    tab = ops.rope_table(max_seq, 10000.0, dev)
    outs = []
    for seq in (True, False):
        kc_, vc_ = kc.clone(), vc.clone()
        out = torch.zeros(batch, nh * 128, dtype=torch.float16, device=dev)
        if seq:
            cur, p, err = _seq_state(ops, tab, max_seq, [pos] * batch)
        else:
            cur, p, err = ops.new_step_state(dev)
            cur.copy_(tab.view(max_seq, 128)[pos]); p.fill_(pos)
        ops.attn_decode(q, k, v, kc_, vc_, out, p, nh, nkv, cur=cur, n_splits=n_splits)
        ops.check_step_state(err)
        outs.append((out, kc_[:, :, :pos + 1].clone(), vc_[:, :, :pos + 1].clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("max_seq,nh,nkv,n_splits", [(384, 4, 4, 1), (2048, 8, 8, 8), (2048, 8, 2, 8)])
def test_attn_decode_seq_out_of_range_position_is_that_sequences_no_op(max_seq, nh, nkv, n_splits):
    """an ordinary argument check: the state of ONE sequence says max_seq (what the tail's saturation leaves after the last row) -- its output and
    cache are untouched and its error word is raised; the others are served; check_step_state raises"""
    from amq_amd import _lib, ops
    dev = _dev()
    positions = [37, max_seq, 300]
    inside = [37, 0, 300]
    kc, vc, q, k, v = _attn_inputs(inside, max_seq, nh, nkv, seed=max_seq + nh)
    tab = ops.rope_table(max_seq, 10000.0, dev)
    kc_, vc_ = kc.clone(), vc.clone()
    out = torch.full((3, nh * 128), 7.0, dtype=torch.float16, device=dev)
    cur, pos, err = _seq_state(ops, tab, max_seq, positions)
    ops.attn_decode(q, k, v, kc_, vc_, out, pos, nh, nkv, cur=cur, n_splits=n_splits)
    assert err.tolist() == [0, 1, 0]
    assert bool((out[1] == 7.0).all()) and torch.isnan(kc_[1]).all() and torch.isnan(vc_[1]).all()
    for b in (0, 2):
        p = positions[b]
        kc1, vc1 = kc[b:b + 1].clone(), vc[b:b + 1].clone()
        out1 = torch.zeros(1, nh * 128, dtype=torch.float16, device=dev)
        cur1, pos1, _ = ops.new_step_state(dev)
        cur1.copy_(tab.view(max_seq, 128)[p]); pos1.fill_(p)
        ops.attn_decode(q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), kc1, vc1, out1, pos1, nh, nkv, cur=cur1,
                        n_splits=n_splits)
        assert torch.equal(out[b], out1[0]) and torch.equal(kc_[b, :, :p + 1], kc1[0, :, :p + 1])
    with pytest.raises(_lib.AmqError):
        ops.check_step_state(err)
    assert all(int(t.abs().sum().item()) == 0 for t in ops._ATTN_TICKETS._cur.values())


def test_tail_and_set_token_advance_every_sequence():
    """amq_decode_tail_seq_f16 / amq_set_token_seq_f16: per-row first-maximum arg-max, every pos[b] + 1, every rope_cur[b] = table[pos[b] + 1],
    saturation at rope_rows per sequence, the suppress list; the sampled tail's per-sequence form likewise"""
    from amq_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    vocab, hidden, B, rows = 1024, 256, 5, 50
    embed = torch.randn(vocab, hidden, generator=g).half().to(dev)
    logits = torch.randn(B, vocab, generator=g).half().to(dev)
    logits[2, 100] = 9.0; logits[2, 700] = 9.0                      # tie: the first one wins
    tab = ops.rope_table(rows, 10000.0, dev)
    table = tab.view(rows, 128)
    positions = [41, 0, 7, 48, 49]                                   # 48 -> 49 (the last row); 49 -> 50 = rope_rows: saturated, row 49 kept
    want_tok = torch.argmax(logits.float(), 1)
    assert int(want_tok[2]) == 100

    def fresh():
        cur, pos, err = _seq_state(ops, tab, rows, positions)
        return cur, pos, err, torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, hidden, dtype=torch.float16, device=dev)

    cur, pos, err, token, x = fresh()
    ops.decode_tail(logits, embed, token, pos, x, table=tab, cur=cur)
    assert torch.equal(token, want_tok) and pos.tolist() == [42, 1, 8, 49, 50] and err.tolist() == [0] * B
    assert torch.equal(x, embed[want_tok])
    assert torch.equal(cur, table[torch.tensor([42, 1, 8, 49, 49], device=dev)])
    ops.decode_tail(logits, embed, token, pos, x, table=tab, cur=cur)            # once more: the full sequence stays at rope_rows
    assert pos.tolist() == [43, 2, 9, 50, 50] and torch.equal(cur, table[torch.tensor([43, 2, 9, 49, 49], device=dev)])
    # the suppress list: the winners of rows 2 and 4 are never chosen
    cur, pos, err, token, x = fresh()
    sup = torch.full((8,), -1, dtype=torch.int32, device=dev)
    sup[0], sup[3] = 100, int(want_tok[4])
    masked = logits.float().clone()
    masked[:, 100] = float("-inf"); masked[:, int(want_tok[4])] = float("-inf")
    ops.decode_tail(logits, embed, token, pos, x, table=tab, cur=cur, suppress=sup)
    assert torch.equal(token, torch.argmax(masked, 1)) and int(token[2]) == 700 and pos.tolist() == [42, 1, 8, 49, 50]
    assert torch.equal(x, embed[token])
    # set_token: the rows of the positions as they are, positions untouched; one id broadcast, or one per sequence
    cur, pos, err, token, x = fresh()
    cur.zero_()
    ids = torch.tensor([5, 1023, 0, 77, 512], dtype=torch.int64, device=dev)
    ops.set_token(ids, embed, token, pos, x, table=tab, cur=cur)
    assert torch.equal(token, ids) and torch.equal(x, embed[ids]) and pos.tolist() == positions
    assert torch.equal(cur, table[torch.tensor(positions, device=dev)])
    ops.set_token(ids[3:4].contiguous(), embed, token, pos, x, table=tab, cur=cur)
    assert token.tolist() == [77] * B and torch.equal(x, embed[token])
    # the sampled tail with top_k = 1 and no draw = the greedy choice; same per-sequence bookkeeping
    cur, pos, err, token, x = fresh()
    state = ops.new_sampling_state(dev)
    ops.set_sampling_state(state, top_k=1, first_kept=True)
    ops.decode_tail_sample(logits, embed, token, pos, x, state, table=tab, cur=cur)
    assert torch.equal(token, want_tok) and pos.tolist() == [42, 1, 8, 49, 50] and torch.equal(x, embed[want_tok])
    assert torch.equal(cur, table[torch.tensor([42, 1, 8, 49, 49], device=dev)])
    # a step state that is not the views of one array of blocks is refused on the host
    with pytest.raises(ValueError):
        ops.decode_tail(logits, embed, token, pos, x, table=tab, cur=cur.contiguous())
    with pytest.raises(ValueError):
        ops.decode_tail(logits[:3].contiguous(), embed, token[:3].contiguous(), pos, x[:3].contiguous(), table=tab, cur=cur)


# ---------------------------------------------------------------------------------------------------------------- the runner
def _right_padded(lengths, S, seed, vocab=1024):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab, (len(lengths), S), generator=g)
    pad = ids.clone()
    for b, n in enumerate(lengths):
        pad[b, n:] = 0
    return pad.to(_dev())


def _ragged_run(mb, ids, lengths, steps, use_graph=False):
    """prompt pass + steps - 1 token steps of a ragged runner -> (tokens [B, steps], the logits of every step [steps, B, vocab])"""
    B = len(lengths)
    mb.prefill(ids, use_graph=use_graph, lengths=lengths)
    toks, logits = [mb.token.clone()], [mb.logits.float().view(B, -1).clone()]
    for _ in range(1, steps):
        mb.decode_step(use_graph)
        toks.append(mb.token.clone())
        logits.append(mb.logits.float().view(B, -1).clone())
    return torch.stack(toks, 1), torch.stack(logits)


def _against_each_alone(m1, ids, lengths, toks_b, logits_b):
    """Every sequence against its own batch-1 run on its un-padded prompt.  Two fp16 routes (8 rows per launch / one row) part at a near-tie of
    the two best logits, and what follows a parted step is a different sequence, not comparable: the batch-1 run is therefore FED the ragged
    run's tokens, so that every step compares the same function of the same inputs.  Logits within 1e-2 of the largest reference logit at EVERY
    step (not only the last); the batch-1 run's own greedy choice agrees with the ragged run's token on >= 0.8 of the steps."""
    steps = toks_b.shape[1]
    for b, n in enumerate(lengths):
        m1.reset()
        m1.prefill(ids[b, :n].contiguous(), use_graph=False)
        own = []
        for i in range(steps):
            ref = m1.logits.float()
            err = (logits_b[i, b] - ref).abs().max().item()
            assert err <= 1e-2 * ref.abs().max().item(), (b, n, i, err, ref.abs().max().item())
            own.append(int(m1.token.item()))
            if i + 1 < steps:
                m1.set_token(toks_b[b, i:i + 1].contiguous())
                m1.decode_step(use_graph=False)
        agree = (torch.tensor(own, device=toks_b.device) == toks_b[b]).float().mean().item()
        assert agree >= 0.8, (b, n, own, toks_b[b].tolist())                      # (a near-tie may flip a greedy choice)


@pytest.mark.parametrize("B,gqa", [(2, False), (4, True), (8, False)])
def test_ragged_decode_matches_single_sequence_runs(B, gqa):
    """QuantLlama(batch=B, ragged=True) over prompts of unequal length: every sequence gets what a batch-1 runner gives it alone on its un-padded
    prompt.  Enough steps that every position passes the longest prompt's length: the cache rows the pad rows of the prompt pass wrote are all
    overwritten and attended.  Graph replay == eager."""
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = dict(arch._cfg(2, 512, 1024, 4, 2 if gqa else 4, 1, vocab=1024))
    lengths = [24, 7, 16, 1, 23, 2, 11, 24][:B]
    S, steps = 24, 26
    assert min(lengths) + steps - 1 > S
    ids = _right_padded(lengths, S, seed=B)
    mb = QuantLlama(cfg, None, device=DEV, max_seq=64, seed=4, batch=B, ragged=True)
    out_b, steps_logits = _ragged_run(mb, ids, lengths, steps)
    logits_b = steps_logits[-1].clone()
    assert out_b.shape == (B, steps) and mb.pos.tolist() == [n + steps - 1 for n in lengths] and mb.host_pos == max(lengths) + steps - 1
    mb.check()
    _against_each_alone(QuantLlama(cfg, None, device=DEV, max_seq=64, seed=4), ids, lengths, out_b, steps_logits)
    mb.reset()
    assert torch.equal(mb.generate(ids, steps, use_graph=False, lengths=lengths), out_b)      # generate() is that loop
    # what stands in the pad columns does not matter
    junk = ids.clone()
    for b, n in enumerate(lengths):
        junk[b, n:] = 1023 - b
    mb.reset()
    assert torch.equal(mb.generate(junk, steps, use_graph=False, lengths=lengths), out_b)
    mb.reset()
    out_g = mb.generate(ids, steps, use_graph=True, lengths=torch.tensor(lengths))
    assert torch.equal(out_g, out_b) and torch.equal(mb.logits.float().view(B, -1), logits_b)
    # the captured prompt pass of this length serves other lengths
    other = [max(1, S - n) for n in lengths]
    mb.reset()
    eager = mb.generate(ids, 4, use_graph=False, lengths=other).clone()
    mb.reset()
    assert torch.equal(mb.generate(ids, 4, use_graph=True, lengths=other), eager)
    mb.check()
    with pytest.raises(ValueError):
        mb.prefill(ids, lengths=[0] + lengths[1:])
    with pytest.raises(ValueError):
        mb.prefill(ids, lengths=lengths, start_pos=4)
    with pytest.raises(ValueError):
        mb.generate(ids, 64 - max(lengths) + 1, lengths=lengths)          # the longest prompt + n does not fit the cache
    with pytest.raises(ValueError):
        mb.prefill_batch(ids)


@pytest.mark.parametrize("B", [2, 4])
def test_ragged_runner_with_equal_lengths_is_the_plain_batched_runner(B):
    from amq_amd import arch
    from amq_amd.llama import DenseLlama, QuantLlama
    cfg = dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=1024))
    ids = torch.randint(0, 1024, (B, 24), generator=torch.Generator().manual_seed(B)).to(_dev())
    steps = 6
    plain = QuantLlama(cfg, None, device=DEV, max_seq=48, seed=4, batch=B)
    rag = QuantLlama(cfg, None, device=DEV, max_seq=48, seed=4, batch=B, ragged=True)
    assert plain.pos.shape == (1,) and rag.pos.shape == (B,) and rag.rope_cur.shape == (B, 128) and not plain.ragged
    for use_graph in (False, True):
        plain.reset(); rag.reset()
        a = plain.generate(ids, steps, use_graph=use_graph)
        b = rag.generate(ids, steps, use_graph=use_graph, lengths=[24] * B)
        assert torch.equal(a, b) and torch.equal(plain.logits, rag.logits.view(B, -1))
        rag.reset()
        assert torch.equal(rag.generate(ids, steps, use_graph=use_graph), a)          # no lengths: every prompt fills its row
    rag.check(); plain.check()
    each = [3, 5] + [7] * (B - 2)
    rag.set_pos(each)
    assert rag.host_pos == max(each) and rag.pos.tolist() == each
    rag.set_pos(9)
    assert rag.pos.tolist() == [9] * B and rag.host_pos == 9
    with pytest.raises(ValueError):
        plain.prefill(ids, lengths=[24] * B)
    for kw in (dict(engine=True), ):
        with pytest.raises(ValueError):
            QuantLlama(cfg, None, device=DEV, max_seq=48, seed=4, batch=1, ragged=True, **kw)
    with pytest.raises(ValueError):
        DenseLlama(cfg, device=DEV, max_seq=48, batch=B, ragged=True)
    rag.fuse_qkv_attn = True
    with pytest.raises(ValueError):
        rag._step()
    rag.fuse_qkv_attn = False


def test_ragged_decode_long_cache():
    """a cache long enough for several workgroups per head and sequence (grouped-query heads: the matrix-core kernel and its combine launch), one
    sequence past the first chunk, one far inside it"""
    from amq_amd import arch, ops
    from amq_amd.llama import QuantLlama
    cfg = dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=1024))
    lengths, S, max_seq, steps = [300, 37, 210], 300, 640, 6
    assert ops.attn_decode_splits(max_seq) > 1
    ids = _right_padded(lengths, S, seed=5)
    mb = QuantLlama(cfg, None, device=DEV, max_seq=max_seq, seed=4, batch=3, ragged=True)
    out_b, steps_logits = _ragged_run(mb, ids, lengths, steps, use_graph=True)
    mb.check()
    _against_each_alone(QuantLlama(cfg, None, device=DEV, max_seq=max_seq, seed=4), ids, lengths, out_b, steps_logits)


def test_ragged_decode_long_cache_multi_head():
    """the same with one kv head per query head: the split kernel with the last-arriver combine, chunks from each sequence's own position"""
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = dict(arch._cfg(1, 512, 1024, 4, 4, 1, vocab=1024))
    lengths, S, max_seq, steps = [300, 37, 210], 300, 640, 6
    ids = _right_padded(lengths, S, seed=6)
    mb = QuantLlama(cfg, None, device=DEV, max_seq=max_seq, seed=4, batch=3, ragged=True)
    out_b, steps_logits = _ragged_run(mb, ids, lengths, steps, use_graph=True)
    mb.check()
    _against_each_alone(QuantLlama(cfg, None, device=DEV, max_seq=max_seq, seed=4), ids, lengths, out_b, steps_logits)


def test_ragged_decode_at_7b_width():
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = dict(arch._cfg(1, 4096, 11008, 32, 32, 1, vocab=1024))
    B, S, steps = 8, 16, 4
    lengths = [16, 3, 9, 1, 12, 16, 5, 8]
    ids = _right_padded(lengths, S, seed=B)
    mb = QuantLlama(cfg, None, device=DEV, max_seq=32, seed=4, batch=B, ragged=True)
    out_b, steps_logits = _ragged_run(mb, ids, lengths, steps)
    logits_b = steps_logits[-1].clone()
    _against_each_alone(QuantLlama(cfg, None, device=DEV, max_seq=32, seed=4), ids, lengths, out_b, steps_logits)
    mb.reset()
    out_g = mb.generate(ids, steps, use_graph=True, lengths=lengths)
    assert torch.equal(out_g, out_b) and torch.equal(mb.logits.float(), logits_b)
    mb.check()


def test_ragged_sampled_decoding_and_eos_stop():
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=1024))
    lengths, S, n = [20, 5, 13, 1], 20, 24
    ids = _right_padded(lengths, S, seed=9)
    m = QuantLlama(cfg, None, device=DEV, max_seq=64, seed=4, batch=4, ragged=True)
    greedy = m.generate(ids, n, lengths=lengths).clone()
    m.set_sampling(temperature=0.8, top_k=50, top_p=0.9, seed=5)
    a = m.generate(ids, n, lengths=lengths).clone()
    b = m.generate(ids, n, lengths=lengths).clone()
    assert torch.equal(a, b) and a.shape == (4, n)
    assert m.pos.tolist() == [v + n - 1 for v in lengths]
    m.set_sampling(temperature=0.7, top_k=50, top_p=0.9, seed=6)
    assert not torch.equal(m.generate(ids, n, lengths=lengths), a)
    m.set_sampling(temperature=1.0, top_k=1, top_p=1.0, seed=1)
    assert torch.equal(m.generate(ids, n, lengths=lengths), greedy)
    m.set_sampling(None)
    # EOS: a token of the greedy run that the fewest sequences emit; whoever emits it pads from there, the others go on
    g = greedy.cpu()
    cands = sorted(set(g[:, 1:n - 2].reshape(-1).tolist()), key=lambda t: (int((g == t).any(1).sum()), t))
    eos, pad = int(cands[0]), 1000
    hit = (g == eos)
    assert hit.any() and int(hit.any(1).sum()) < 4, "every sequence emits the chosen id: no sequence would continue"
    want = g.clone()
    for r in range(4):
        if hit[r].any():
            want[r, int(hit[r].int().argmax()) + 1:] = pad
    longest = max(int(hit[r].int().argmax()) + 1 if hit[r].any() else n for r in range(4))
    m.set_eos([eos], pad_id=pad)
    got = m.generate(ids, n, stop_at_eos=True, lengths=lengths).cpu()
    assert torch.equal(got, want[:, :longest])
    assert m.unfinished() == 4 - int(hit.any(1).sum())
    m.check()


# ---------------------------------------------------------------------------------------------------------------- the HF surface
NAMES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _swap_linears(model, bits_cycle=(4, 2, 3, 3, 2, 4, 3), seed=100):
    """every decoder linear -> an HQQ stand-in of its shape (random HQQ weights; the linear's own bias kept)"""
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
        from transformers import MistralConfig, MistralForCausalLM
        cfg = MistralConfig(hidden_size=512, intermediate_size=768, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=1,
                            vocab_size=1000, max_position_embeddings=256, rms_norm_eps=1e-5, attn_implementation="eager", sliding_window=None,
                            rope_theta=1000000.0, head_dim=128)
        m = MistralForCausalLM(cfg)
    return m.to(torch.float16).to(DEV).eval()


def _prepared(family):
    from amq_amd.patching import prepare_for_inference
    model = _swap_linears(_tiny(family))
    prepare_for_inference(model, backend="hip")
    return model


def _left_padded(lengths, S, seed, pad=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lengths), S), pad, dtype=torch.int64)
    mask = torch.zeros(len(lengths), S, dtype=torch.int64)
    for b, n in enumerate(lengths):
        ids[b, S - n:] = torch.randint(1, 1000, (n,), generator=g)
        mask[b, S - n:] = 1
    return ids.to(DEV), mask.to(DEV)


def _gen(model, ids, mask, n):
    return model.generate(ids, attention_mask=mask, min_new_tokens=n, max_new_tokens=n, do_sample=False, num_beams=1, pad_token_id=0)


def _same_new_tokens_or_a_tie(model, rows, fast_new, slow_new, eos=None):
    """rows: the un-padded prompts.  Two fp16 implementations of one function decode greedily: equal tokens, or -- at the first step where they part
    -- a near-tie under HF's own logits for the common prefix (what follows a parted step is not comparable)"""
    for b, row in enumerate(rows):
        diff = (fast_new[b] != slow_new[b]).nonzero()
        if len(diff) == 0:
            continue
        t = int(diff[0])
        with torch.inference_mode():
            lg = model(torch.cat([row, slow_new[b, :t]])[None]).logits[0, -1].float()      # (no start_pos: HF's own forward over the same modules)
            if eos is not None:
                lg[eos] = float("-inf")
        gap = float(lg.max() - lg[int(fast_new[b, t])])
        assert gap <= 4e-3 * float(lg[torch.isfinite(lg)].abs().max()), (b, t, gap, fast_new[b].tolist(), slow_new[b].tolist())


@pytest.mark.parametrize("family", ["llama", "mistral"])
def test_left_padded_generate_on_the_converted_object(family):
    """tokenizer(prompts, padding=True, padding_side="left") + model.generate(**enc) on a model converted with padded=True: HF's own generate over
    the same modules with the same mask (taken before the conversion); every row also against its prompt alone at batch 1"""
    pytest.importorskip("transformers")
    from amq_amd import hf_fast
    model = _prepared(family)
    eos = model.generation_config.eos_token_id
    lengths, S, n = [9, 4, 7], 9, 12
    ids, mask = _left_padded(lengths, S, seed=5)
    with torch.inference_mode():
        slow = _gen(model, ids, mask, n)
    # today's behaviour without the flag: HF's own generate, no runner
    hf_fast.convert_model_to_hip(model)
    with torch.inference_mode():
        unflagged = _gen(model, ids, mask, n)
    assert not hf_fast._RUNNERS.get(model) and unflagged.shape == slow.shape
    hf_fast.convert_model_to_hip(model, padded=True)
    ids_before, mask_before = ids.clone(), mask.clone()
    with torch.inference_mode():
        fast = _gen(model, ids, mask, n)
        fast2 = _gen(model, ids, mask, n)
    assert torch.equal(ids, ids_before) and torch.equal(mask, mask_before)
    assert fast.shape == (3, S + n) and fast.dtype == ids.dtype and torch.equal(fast[:, :S], ids)        # the caller's padded ids are the prefix
    assert torch.equal(fast, fast2)
    assert ("ragged", 3) in hf_fast._RUNNERS[model] and 3 not in hf_fast._RUNNERS[model]                 # (it really was the ragged runner)
    assert hf_fast._RUNNERS[model][("ragged", 3)].ragged
    rows = [ids[b, S - L:] for b, L in enumerate(lengths)]
    _same_new_tokens_or_a_tie(model, rows, fast[:, S:], slow[:, S:], eos)
    assert torch.equal(fast[:, S:S + 3], slow[:, S:S + 3])
    # every prompt alone, un-padded, at batch 1 through the same converted model
    for b, row in enumerate(rows):
        with torch.inference_mode():
            alone = _gen(model, row[None], torch.ones_like(row[None]), n)
        assert torch.equal(alone[0, :len(row)], row)
        _same_new_tokens_or_a_tie(model, [row], fast[b:b + 1, S:], alone[:, len(row):], eos)
        assert torch.equal(fast[b, S:S + 3], alone[0, len(row):len(row) + 3])
    # a full mask keeps going to the plain runner; masks the helper refuses go to HF and build nothing
    with torch.inference_mode():
        _gen(model, ids, torch.ones_like(mask), n)
    assert 3 in hf_fast._RUNNERS[model]
    hf_fast._RUNNERS.pop(model)
    hole = mask.clone(); hole[1, S - 2] = 0
    right = mask.flip(1)
    for bad in (hole, right):
        with torch.inference_mode():
            out = _gen(model, ids, bad, n)
        assert out.shape == (3, S + n) and not hf_fast._RUNNERS.get(model)
    with pytest.raises(ValueError):
        model(ids, attention_mask=mask, start_pos=0, use_cache=False)                                  # the forward surface keeps refusing padding
    # sampled / open-ended padded calls need sampling=True as well
    with torch.inference_mode():
        model.generate(ids, attention_mask=mask, max_new_tokens=6, do_sample=False, num_beams=1, pad_token_id=0)
    assert not hf_fast._RUNNERS.get(model)
    hf_fast.convert_model_to_hip(model, sampling=True, padded=True)
    with torch.inference_mode():
        torch.manual_seed(3)
        s1 = model.generate(ids, attention_mask=mask, min_new_tokens=8, max_new_tokens=8, do_sample=True, top_k=20, num_beams=1, pad_token_id=0)
        torch.manual_seed(3)
        s2 = model.generate(ids, attention_mask=mask, min_new_tokens=8, max_new_tokens=8, do_sample=True, top_k=20, num_beams=1, pad_token_id=0)
    assert torch.equal(s1, s2) and s1.shape == (3, S + 8) and torch.equal(s1[:, :S], ids) and ("ragged", 3) in hf_fast._RUNNERS[model]
    hf_fast.revert_model_to_hf(model)
    assert "_amq_padded" not in model.__dict__ and model not in hf_fast._RUNNERS
