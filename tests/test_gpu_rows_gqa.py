"""GPU: the matrix-core rows attention of grouped-query models (amq_attn_decode_rows_gqa_f16, ops.attn_decode_rows(grouped=True)).

1. / 2. Row j of a step at positions p .. p + R - 1 has the BITS of the single-token grouped kernel (ops.attn_decode with a per-sequence step state
   and the same n_splits) at position p + j, run R times in succession over a cache that then holds the step's earlier rows; so do the appended
   cache rows; nothing else is written.  This follows from the construction (same slicing, same orders, masked terms exact zeros): a difference is
   a bug, not a tolerance.  The caches are NaN from row p on: a row at or past p that reached an MFMA would show.
3. Against the eager fp32 formula and the per-head rows kernels, within the bounds tests/test_gpu_decode.py::test_attn_decode_gqa_kernel holds the
   single-token grouped kernel to.
4. Rows outside the cache.  5. The runner."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev():
    return torch.device(DEV)


def _rows_state(ops, tab, max_seq, p, rows):
    cur, pos, err = ops.new_step_state(_dev(), batch=rows)
    positions = [p + j for j in range(rows)]
    pos.copy_(torch.tensor(positions, dtype=torch.int32))
    cur.copy_(tab.view(-1, 128)[torch.tensor([min(max(q, 0), max_seq - 1) for q in positions], device=_dev())])
    return cur, pos, err


def _inputs(nh, nkv, p, rows, max_seq, seed=0):
    dev = _dev()
    g = torch.Generator().manual_seed(1000 * p + 10 * rows + nh + nkv + max_seq + seed)
    kc = torch.full((1, nkv, max_seq, 128), float("nan"), dtype=torch.float16, device=dev)     # rows >= p are NaN: never read from the cache
    vc = torch.full_like(kc, float("nan"))
    if p > 0:
        kc[0, :, :p] = torch.randn(nkv, p, 128, generator=g).half().to(dev)
        vc[0, :, :p] = torch.randn(nkv, p, 128, generator=g).half().to(dev)
    q = torch.randn(rows, nh * 128, generator=g).half().to(dev)
    k = torch.randn(rows, nkv * 128, generator=g).half().to(dev)
    v = torch.randn(rows, nkv * 128, generator=g).half().to(dev)
    return kc, vc, q, k, v


def _norms(seed=5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (1.0 + 0.1 * torch.randn(128, generator=g)).half().to(_dev()).contiguous()
    return dict(q_norm=mk(), k_norm=mk(), norm_eps=1e-6)


def _single_token_rows(ops, tab, q, k, v, kc, vc, p, rows, max_seq, nh, nkv, n_splits, **nk):
    """`rows` successive single-token calls of the grouped kernel (per-sequence step state of one sequence), each appending its own cache row.
    One chunk for everything (n_splits == 1) is not a launch ops.attn_decode gives the grouped kernel: the same chunk -- 2048 keys in 16 stages --
    is the first of two over a cache of twice the length, with the rows' positions inside it: one active chunk, written by the kernel itself."""
    dev = _dev()
    kc_, vc_, ns = kc.clone(), vc.clone(), n_splits
    if n_splits == 1:
        kc_ = torch.cat([kc_, torch.full_like(kc_, float("nan"))], 2).contiguous()
        vc_ = torch.cat([vc_, torch.full_like(vc_, float("nan"))], 2).contiguous()
        ns = 2
        assert p + rows <= max_seq and -(-(2 * max_seq) // 2) == max_seq
    out = torch.zeros(rows, nh * 128, dtype=torch.float16, device=dev)
    for j in range(rows):
        cur1, pos1, err1 = _rows_state(ops, tab, max_seq, p + j, 1)
        ops.attn_decode(q[j:j + 1].contiguous(), k[j:j + 1].contiguous(), v[j:j + 1].contiguous(), kc_, vc_, out[j:j + 1], pos1, nh, nkv, cur=cur1,
                        n_splits=ns, **nk)
        assert err1.tolist() == [0]
    return out, kc_[:, :, :max_seq], vc_[:, :, :max_seq]


def _rows_call(ops, tab, q, k, v, kc, vc, p, rows, max_seq, nh, nkv, n_splits, grouped=True, **nk):
    kc_, vc_ = kc.clone(), vc.clone()
    out = torch.zeros(rows, nh * 128, dtype=torch.float16, device=_dev())
    cur, pos, err = _rows_state(ops, tab, max_seq, p, rows)
    ops.attn_decode_rows(q, k, v, kc_, vc_, out, cur, pos, nh, nkv, n_splits=n_splits, grouped=grouped, **nk)
    assert err.tolist() == [0] * rows and pos.tolist() == [p + j for j in range(rows)]
    return out, kc_, vc_


def _same_bits(ops, nh, nkv, p, rows, max_seq, n_splits, twin=True, **nk):
    tab = ops.rope_table(max_seq, 10000.0, _dev())
    kc, vc, q, k, v = _inputs(nh, nkv, p, rows, max_seq)
    ns = n_splits or ops.attn_decode_splits(max_seq, nh, ops.attn_rows_gqa_blocks(rows, nh, nkv), nkv)      # 0: the launch's own policy
    ref, kc_r, vc_r = _single_token_rows(ops, tab, q, k, v, kc, vc, p, rows, max_seq, nh, nkv, ns, **nk)
    assert torch.isfinite(ref.float()).all()
    args = (ops, tab, q, k, v, kc, vc, p, rows, max_seq, nh, nkv)
    got, kc_g, vc_g = _rows_call(*args, n_splits, **nk)
    chunk = 128 * -(-(-(-max_seq // ns)) // 128)
    for j in range(rows):
        d = (got[j].float() - ref[j].float()).abs().max().item()
        print(f"rows gqa {nh}/{nkv} p={p} R={rows} max_seq={max_seq} splits={ns} row {j}: active chunks {-(-(p + j + 1) // chunk)} max|diff| {d:.3e}")
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, ref)
    assert torch.equal(kc_g[0, :, p:p + rows], kc_r[0, :, p:p + rows]) and torch.equal(vc_g[0, :, p:p + rows], vc_r[0, :, p:p + rows])
    assert torch.equal(kc_g[0, :, :p], kc[0, :, :p]) and torch.equal(vc_g[0, :, :p], vc[0, :, :p])
    assert torch.isnan(kc_g[0, :, p + rows:]).all() and torch.isnan(vc_g[0, :, p + rows:]).all()
    again, kc_a, vc_a = _rows_call(*args, n_splits, **nk)
    assert torch.equal(again, got) and torch.equal(kc_a[0, :, :p + rows], kc_g[0, :, :p + rows]) and torch.equal(vc_a[0, :, :p + rows], vc_g[0, :, :p + rows])
    if n_splits == 0:
        assert torch.equal(_rows_call(*args, ns, **nk)[0], got)
    if twin:
        from amq_amd import _lib
        with _lib.routed_to(_lib.open_twin()):
            safe, kc_s, vc_s = _rows_call(*args, n_splits, **nk)
        assert torch.equal(safe, got) and torch.equal(kc_s[0, :, :p + rows], kc_g[0, :, :p + rows]) and torch.equal(vc_s[0, :, :p + rows], vc_g[0, :, :p + rows])
    return got, kc_g, vc_g, (tab, kc, vc, q, k, v)


HEADS = [(4, 2), (32, 8), (28, 4), (16, 1), (6, 3)]
# (p, rows, max_seq, n_splits)
CASES = [
    (0, 2, 2048, 8), (0, 8, 2048, 8),           # the first token: nothing cached, the DMA clamp lands on a NaN row
    (60, 8, 2048, 8),                           # the new rows cross a tile boundary (64)
    (124, 8, 2048, 8),                          # ... a stage boundary (128)
    (250, 8, 2048, 8), (255, 2, 2048, 8), (256, 4, 2048, 8),       # ... a chunk boundary (256): rows whose numbers of active chunks differ
    (120, 8, 2048, 16),                         # chunks of 128
    (700, 5, 2048, 8),
    (2040, 8, 2048, 8),                         # p + R = max_seq
    (3000, 4, 4096, 4),                         # eight stages per workgroup
    (5000, 3, 5120, 40),                        # more than 32 active chunks in the combine
    (8000, 8, 8192, 0),
    (100, 4, 2048, 1),                          # one chunk for everything
]


@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("p,rows,max_seq,n_splits", CASES)
def test_rows_have_the_bits_of_the_single_token_kernel(nh, nkv, p, rows, max_seq, n_splits):
    from amq_amd import ops
    _same_bits(ops, nh, nkv, p, rows, max_seq, n_splits)


def test_rows_have_the_bits_of_the_single_token_kernel_long_cache():
    from amq_amd import ops
    _same_bits(ops, 8, 2, 30000, 4, 32768, 0)


@pytest.mark.parametrize("nh,nkv", [(32, 8), (28, 4)])
@pytest.mark.parametrize("p,rows,max_seq,n_splits", [(0, 8, 2048, 8), (124, 8, 2048, 8), (250, 8, 2048, 8), (8000, 8, 8192, 0)])
def test_rows_have_the_bits_of_the_single_token_kernel_qkn(nh, nkv, p, rows, max_seq, n_splits):
    from amq_amd import ops
    _same_bits(ops, nh, nkv, p, rows, max_seq, n_splits, **_norms())


def _rope_rows(t, cs):
    """HF's fp16 rotation of t [rows, heads, 128] with the step-state rows cs [rows, 128] = 64 (cos, sin) pairs each"""
    c = cs.view(-1, 64, 2)
    cos, sin = torch.cat([c[..., 0], c[..., 0]], -1)[:, None], torch.cat([c[..., 1], c[..., 1]], -1)[:, None]
    rot = torch.cat([-t[..., 64:], t[..., :64]], -1)
    return t * cos + rot * sin


@pytest.mark.parametrize("nh,nkv,p,rows,max_seq,n_splits", [(32, 8, 250, 8, 2048, 8), (28, 4, 700, 5, 2048, 8), (6, 3, 0, 8, 2048, 8), (16, 1, 3000, 4, 4096, 4),
                                                           (4, 2, 8000, 8, 8192, 0)])
def test_rows_against_the_eager_formula_and_the_per_head_kernels(nh, nkv, p, rows, max_seq, n_splits):
    from amq_amd import ops
    G = nh // nkv
    got, kc_g, vc_g, (tab, kc, vc, q, k, v) = _same_bits(ops, nh, nkv, p, rows, max_seq, n_splits, twin=False)
    cs = tab.view(max_seq, 128)[p:p + rows]
    # the appended rows: HF's rotation of the new keys, the raw values
    assert torch.equal(kc_g[0, :, p:p + rows].transpose(0, 1), _rope_rows(k.view(rows, nkv, 128), cs))
    assert torch.equal(vc_g[0, :, p:p + rows].transpose(0, 1), v.view(rows, nkv, 128))
    qr = _rope_rows(q.view(rows, nh, 128), cs).float()
    K, V = kc_g[0].repeat_interleave(G, 0).float(), vc_g[0].repeat_interleave(G, 0).float()        # [nh, max_seq, 128]
    per_head, _, _ = _rows_call(ops, tab, q, k, v, kc, vc, p, rows, max_seq, nh, nkv, 0, grouped=False)
    for j in range(rows):
        T = p + j + 1
        w = torch.einsum("hd,htd->ht", qr[j], K[:, :T]) * (128 ** -0.5)
        ref = torch.einsum("ht,htd->hd", torch.softmax(w, -1), V[:, :T]).reshape(-1)
        e1 = (got[j].float() - ref).abs().max().item()
        e2 = (got[j].float() - per_head[j].float()).abs().max().item()
        print(f"rows gqa {nh}/{nkv} p={p} row {j}: |got - eager| {e1:.3e} (max|ref| {ref.abs().max().item():.3e}), |got - per-head rows| {e2:.3e}")
        assert e1 <= 4e-3 * ref.abs().max().item() + 1e-3
        assert e2 <= 2e-3 * per_head[j].float().abs().max().item() + 1e-3


@pytest.mark.parametrize("nh,nkv,max_seq,n_splits", [(4, 2, 2048, 8), (28, 4, 2048, 1)])
def test_rows_outside_the_cache_are_no_ops(nh, nkv, max_seq, n_splits):
    from amq_amd import ops
    dev, rows = _dev(), 4
    p = max_seq - 2                                   # rows 0, 1 fit; rows 2, 3 would be at max_seq, max_seq + 1 (the tail saturates them at max_seq)
    tab = ops.rope_table(max_seq, 10000.0, dev)
    kc, vc, q, k, v = _inputs(nh, nkv, p, rows, max_seq)
    ref, kc_r, vc_r = _rows_call(ops, tab, q[:2].contiguous(), k[:2].contiguous(), v[:2].contiguous(), kc, vc, p, 2, max_seq, nh, nkv, n_splits)
    for sat in (False, True):
        cur, pos, err = _rows_state(ops, tab, max_seq, p, rows)
        if sat:
            pos[2:].fill_(max_seq)
        out = torch.full((rows, nh * 128), 7.0, dtype=torch.float16, device=dev)
        kc_, vc_ = kc.clone(), vc.clone()
        ops.attn_decode_rows(q, k, v, kc_, vc_, out, cur, pos, nh, nkv, n_splits=n_splits, grouped=True)
        assert err.tolist() == [0, 0, 1, 1]
        assert torch.equal(kc_[0, :, :p + 2], kc_r[0, :, :p + 2]) and torch.equal(vc_[0, :, :p + 2], vc_r[0, :, :p + 2])      # nothing appended past the cache
        assert bool((out[2:] == 7.0).all()) and torch.equal(out[:2], ref)
        with pytest.raises(ops._lib.AmqError):
            ops.check_step_state(err)
    # row 0 below zero: every row of the step is a no-op (row j would append cache row p + j of a sequence that has no row p), as in the per-head kernels
    kc0, vc0 = torch.randn(1, nkv, max_seq, 128).half().to(dev), torch.randn(1, nkv, max_seq, 128).half().to(dev)
    for grouped in (True, False):
        cur, pos, err = _rows_state(ops, tab, max_seq, -1, rows)
        out = torch.full((rows, nh * 128), 7.0, dtype=torch.float16, device=dev)
        kc_, vc_ = kc0.clone(), vc0.clone()
        ops.attn_decode_rows(q, k, v, kc_, vc_, out, cur, pos, nh, nkv, n_splits=n_splits, grouped=grouped)
        assert err.tolist() == [1, 1, 1, 1], (grouped, err.tolist())
        assert bool((out == 7.0).all()) and torch.equal(kc_, kc0) and torch.equal(vc_, vc0)


# ------------------------------------------------------------------------------------------------------------------ 5. the runner
SUP = 5             # an id listed in suppress_ids: the arg-max never takes it, so a draft of it is never accepted


def _prompt(S, seg, seed, vocab=1024):
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(8, vocab, (seg,), generator=g)
    return s.repeat(-(-S // seg))[:S].to(_dev())


def _run(m, ids, n, mode, ref=None, use_graph=False):
    """prompt pass + verify steps until n tokens are out (tests/test_gpu_lookup.py: _run).  mode: "lookup" (the tail proposes), "never" (external
    drafts never accepted), "right" (external drafts taken from ``ref``).  -> (tokens [n], {emitted index: its row's logits}, row-0 indices, steps)"""
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


def test_runner_takes_the_grouped_rows_attention(monkeypatch):
    from amq_amd import arch, ops
    from amq_amd.llama import QuantLlama
    if QuantLlama.ROWS_GQA_FROM is None:                # (a measured negative leaves the route off: the runner part is then about the switch)
        monkeypatch.setattr(QuantLlama, "ROWS_GQA_FROM", 2048)
    cfg = dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=1024))
    D, n, S, max_seq = 4, 24, 300, 2048
    R = D + 1
    ids = _prompt(S, 10, seed=3)
    seen = []
    inner = ops.attn_decode_rows

    def recorder(*args, **kwargs):
        seen.append(kwargs.get("grouped", False))
        return inner(*args, **kwargs)
    monkeypatch.setattr(ops, "attn_decode_rows", recorder)
    m = QuantLlama(cfg, None, device=DEV, max_seq=max_seq, seed=4, lookup=D, ngram_max=2)
    tb, rows_b, row0_b, steps_b = _run(m, ids, n, "never")
    assert seen and all(g is True for g in seen)
    assert steps_b == n - 1 and sorted(row0_b) == list(range(1, n))
    tc, rows_c, row0_c, steps_c = _run(m, ids, n, "right", ref=tb)
    assert torch.equal(tc, tb), (tc.tolist(), tb.tolist())
    assert steps_c == math.ceil((n - 1) / R), (steps_c, n, R)
    ta, rows_a, row0_a, steps_a = _run(m, ids, n, "lookup")
    assert torch.equal(ta, tb)
    for run0, rows in ((row0_a, rows_a), (row0_c, rows_c)):
        for e in run0:
            if e < n:
                assert torch.equal(rows[e], rows_b[e]), (e, (rows[e] - rows_b[e]).abs().max().item())
    # graph replay == eager, bit for bit
    tg, rows_g, row0_g, steps_g = _run(m, ids, n, "right", ref=tb, use_graph=True)
    assert torch.equal(tg, tb) and steps_g == steps_c and all(torch.equal(rows_g[e], rows_c[e]) for e in rows_c)
    # a plain one-row runner FED these tokens: logits within 1e-2 max|ref| at every emitted position, its own greedy choice agreeing on >= 0.8
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
    print(f"grouped rows runner R={R}: worst |logits - plain| / max|plain| = {worst:.3e}")
    assert (torch.tensor(own, device=tb.device) == tb).float().mean().item() >= 0.8
    # the switch: a threshold above this cache length leaves the per-head kernels in place
    del seen[:]
    monkeypatch.setattr(QuantLlama, "ROWS_GQA_FROM", 4096)
    m2 = QuantLlama(cfg, None, device=DEV, max_seq=max_seq, seed=4, lookup=D, ngram_max=2)
    _run(m2, ids, 6, "never")
    assert seen and all(g is False for g in seen)
