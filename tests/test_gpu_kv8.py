"""GPU: the 8-bit KV cache -- amq_kv8_store_f16 and amq_attn_decode_kv8_f16 against tests/kv8_ref.py (the storage format bit for
bit; the attention on exact integer scores within the derived bound, on random inputs against fp64), the position guard, the runner with
kv_bits=8 and the public surface."""
import numpy as np
import pytest
import torch

import attndomain_ref as A
import kv8_ref

pytestmark = pytest.mark.gpu

HEADS = [(4, 4), (8, 2), (8, 1)]
LONG = 4 * kv8_ref.CHUNK_MIN                     # a cache of 4 of the policy's smallest chunks
SHORT_POS = (0, 1, 31, 32, 63)
LONG_POS = (kv8_ref.CHUNK_MIN - 1, kv8_ref.CHUNK_MIN, kv8_ref.CHUNK_MIN + 1, 2 * kv8_ref.CHUNK_MIN, LONG - 1)
SHAPES = [(64, 1)] + [(LONG, ns) for ns in (1, 2, 4)]         # (max_seq, n_splits)


def _dev():
    return torch.device("cuda:0")


def _guarded(shape, dtype, dev, fill):
    """a tensor with a guard band behind it in the same allocation -> (tensor view, band view)"""
    n = int(np.prod(shape))
    flat = torch.empty(n + 4096, dtype=dtype, device=dev)
    flat[n:] = 55
    t = flat[:n].view(*shape)
    t.fill_(fill)
    return t, flat[n:]


def _caches(B, nkv, max_seq, dev, code_fill=0, scale_fill=0.0):
    (kc8, g0), (vc8, g1) = (_guarded((B, nkv, max_seq, 128), torch.int8, dev, code_fill) for _ in range(2))
    (ks, g2), (vs, g3) = (_guarded((B, nkv, max_seq), torch.float32, dev, scale_fill) for _ in range(2))
    return (kc8, ks, vc8, vs), (g0, g1, g2, g3)


def _bands_intact(bands):
    return all(bool((g == 55).all()) for g in bands)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype is torch.float32 else t


def _identity_table(max_seq, dev):
    tab = torch.zeros(max_seq, 64, 2, dtype=torch.float16, device=dev)
    tab[..., 0] = 1.0                                  # cos 1, sin 0: the rotation is the identity
    return tab


# ------------------------------------------------------------------------------------------------------------------ 1. store
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("B", [1, 3])
def test_store_is_the_restatement_bit_for_bit(nh, nkv, B):
    from amq_amd import ops
    dev, max_seq = _dev(), 64
    for S in (1, 5, 40):
        for pos0 in (0, 7):
            g = torch.Generator().manual_seed(1000 * S + pos0 + nkv)
            k = torch.randn(B * S, nkv, 128, generator=g)
            v = torch.randn(B * S, nkv, 128, generator=g) * 3.0
            single = B * S * nkv == 1                                        # one k row only: zero at pos0 0, subnormal at pos0 7
            if not single or pos0 == 0:
                k[0, 0] = 0.0                                                # a zero row
            if not single or pos0 == 7:
                k[-1, nkv - 1] *= 2.0 ** -20                                 # a row of fp16 subnormals
            v[-1, nkv - 1] *= 65504.0 / v[-1, nkv - 1].abs().max()           # a row that reaches the largest fp16
            k, v = k.half(), v.half()
            assert float(v[-1, nkv - 1].abs().max()) == 65504.0
            assert single and pos0 == 0 or 0 < float(k[-1, nkv - 1].abs().max()) < 2.0 ** -14
            (kc8, ks, vc8, vs), bands = _caches(B, nkv, max_seq, dev, code_fill=-77, scale_fill=-3.0)
            ops.kv8_store(k.reshape(B * S, -1).to(dev), v.reshape(B * S, -1).to(dev), kc8, ks, vc8, vs, pos0, nkv)
            torch.cuda.synchronize()
            for src, c8, sc in ((k, kc8, ks), (v, vc8, vs)):
                rc, rs = kv8_ref.quantize(src.view(B, S, nkv, 128).transpose(1, 2).contiguous())      # [B, nkv, S, 128]
                assert torch.equal(c8[:, :, pos0:pos0 + S].cpu(), rc), (S, pos0)
                assert torch.equal(_bits(sc[:, :, pos0:pos0 + S].cpu()), _bits(rs)), (S, pos0)
                rest = torch.ones(max_seq, dtype=torch.bool)
                rest[pos0:pos0 + S] = False
                assert bool((c8[:, :, rest.to(dev)] == -77).all()) and bool((sc[:, :, rest.to(dev)] == -3.0).all())
            assert _bands_intact(bands)


def test_store_nonfinite_row_gets_a_nan_scale():
    from amq_amd import ops
    dev = _dev()
    k = torch.randn(4, 2 * 128).half()
    v = torch.randn(4, 2 * 128).half()
    k[1, 5] = float("inf"); v[2, 200] = float("nan"); k[3, 130] = float("-inf")
    kc8, ks, vc8, vs = ops.kv8_alloc(1, 2, 8, dev)
    ops.kv8_store(k.to(dev), v.to(dev), kc8, ks, vc8, vs, 2, 2)
    for src, c8, sc in ((k, kc8, ks), (v, vc8, vs)):
        rc, rs = kv8_ref.quantize(src.view(1, 4, 2, 128).transpose(1, 2).contiguous())
        assert torch.equal(c8[:, :, 2:6].cpu(), rc)
        assert torch.equal(torch.isnan(sc[:, :, 2:6].cpu()), torch.isnan(rs)) and torch.equal(sc[:, :, 2:6].cpu().nan_to_num(7.0), rs.nan_to_num(7.0))
    assert bool(torch.isnan(ks[0, 0, 3])) and bool(torch.isnan(vs[0, 1, 4])) and bool(torch.isnan(ks[0, 1, 5]))
    assert bool(torch.isnan(ops.kv8_dequantize(kc8, ks)[0, 0, 3]).all())


# ------------------------------------------------------------------------------------------------------------------ 2. append
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("B", [1, 3])
def test_append_is_the_store(nh, nkv, B):
    """the row attn_decode_kv8 appends is byte-identical (codes and scale) to kv8_store of rope_rows' output for the same k / v; only that row
    changes -- the counterpart of test_rope_cache_matches_decode_append"""
    from amq_amd import ops
    dev, max_seq = _dev(), 64
    tab = ops.rope_table(max_seq, 10000.0, dev)
    for pos in (0, 1, 31, 63):
        g = torch.Generator().manual_seed(17 * pos + nh)
        q = torch.randn(B, nh * 128, generator=g).half().to(dev)
        k = torch.randn(B, nkv * 128, generator=g).half().to(dev)
        v = torch.randn(B, nkv * 128, generator=g).half().to(dev)
        (kc8, ks, vc8, vs), bands = _caches(B, nkv, max_seq, dev, code_fill=3, scale_fill=0.25)
        before = [t.clone() for t in (kc8, ks, vc8, vs)]
        out = torch.zeros(B, nh * 128, dtype=torch.float16, device=dev)
        cur, pos_state, err = ops.new_step_state(dev)
        cur.copy_(tab.view(max_seq, 128)[pos]); pos_state.fill_(pos)
        ops.attn_decode_kv8(q, k, v, kc8, ks, vc8, vs, out, pos_state, nh, nkv, cur=cur)
        assert int(err.item()) == 0
        want = ops.kv8_alloc(B, nkv, max_seq, dev)
        qr, kr = q.clone(), k.clone()
        ops.rope_rows(qr, kr, tab, 1, nh, nkv, pos0=pos)
        ops.kv8_store(kr, v, *want, pos, nkv)
        for got, w, b4 in zip((kc8, ks, vc8, vs), want, before):
            assert torch.equal(_bits(got[:, :, pos]), _bits(w[:, :, pos])), pos
            keep = torch.ones(max_seq, dtype=torch.bool, device=dev)
            keep[pos] = False
            assert torch.equal(_bits(got[:, :, keep]), _bits(b4[:, :, keep])), pos
        assert _bands_intact(bands)
        # ... and the host-position / table form appends the same bytes
        (kc8b, ksb, vc8b, vsb), _ = _caches(B, nkv, max_seq, dev, code_fill=3, scale_fill=0.25)
        out2 = torch.zeros_like(out)
        ops.attn_decode_kv8(q, k, v, kc8b, ksb, vc8b, vsb, out2, pos, nh, nkv, table=tab)
        assert torch.equal(kc8b, kc8) and torch.equal(_bits(ksb), _bits(ks)) and torch.equal(vc8b, vc8) and torch.equal(out2, out)


# ------------------------------------------------------------------------------------------------------------------ 3. exact scores
def _exact_launch(ops, dev, q, K, V, pos, max_seq, n_splits, tab):
    """K / V [B, nkv, pos + 1, 128] integer rows (row pos: the new token) -> out [B, nh, 128] float64 and its raw fp16 bits"""
    B, nh = q.shape[:2]
    nkv = K.shape[1]
    kc8 = torch.full((B, nkv, max_seq, 128), 77, dtype=torch.int8)
    vc8 = torch.full((B, nkv, max_seq, 128), 77, dtype=torch.int8)
    ks = torch.full((B, nkv, max_seq), float("nan"))                  # rows past the context: never read, or the output is NaN
    vs = torch.full((B, nkv, max_seq), float("nan"))
    if pos:
        for X, c8, sc in ((K, kc8, ks), (V, vc8, vs)):
            c, s = kv8_ref.quantize(torch.from_numpy(np.ascontiguousarray(X[:, :, :pos])))
            assert (s == 1.0).all()
            c8[:, :, :pos], sc[:, :, :pos] = c, s
    kc8, ks, vc8, vs = (t.to(dev) for t in (kc8, ks, vc8, vs))
    out = torch.full((B, nh * 128), 9.0, dtype=torch.float16, device=dev)
    qd = torch.from_numpy(q).reshape(B, -1).to(dev)
    kd = torch.from_numpy(np.ascontiguousarray(K[:, :, pos])).reshape(B, -1).to(dev)
    vd = torch.from_numpy(np.ascontiguousarray(V[:, :, pos])).reshape(B, -1).to(dev)
    ops.attn_decode_kv8(qd, kd, vd, kc8, ks, vc8, vs, out, pos, nh, nkv, table=tab, n_splits=n_splits)
    # the appended row holds the integers themselves
    assert torch.equal(kc8[:, :, pos].cpu().double(), torch.from_numpy(K[:, :, pos].astype(np.float64))) and bool((ks[:, :, pos] == 1.0).all())
    o = out.cpu().view(B, nh, 128)
    return o.double().numpy(), o.view(torch.int16).numpy()


@pytest.mark.parametrize("max_seq,n_splits", SHAPES)
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("B", [1, 3])
def test_exact_scores_within_the_derived_bound(max_seq, n_splits, nh, nkv, B):
    from amq_amd import ops
    dev = _dev()
    tab = _identity_table(max_seq, dev)
    chunk = ops.attn_decode_kv8_chunk(max_seq, n_splits)
    assert max_seq == 64 or chunk * n_splits == max_seq
    worst = 0.0
    for pos in (SHORT_POS if max_seq == 64 else LONG_POS):
        sk = sorted(set(A.seams("split", pos, chunk)) | {t for c in range(0, pos + 1, kv8_ref.CHUNK_MIN) for t in (c - 1, c) if 0 <= t <= pos})
        for profile in kv8_ref.EXACT_PROFILES:
            rounds = A.spotlight_rounds(len(sk), B, nh, nkv) if profile == "spotlight" else 1
            for rnd in range(rounds):
                q, K, V, raw = kv8_ref.exact_case(profile, B, nh, nkv, pos, sk, rnd)          # preconditions asserted inside (check_exact)
                r = kv8_ref.reference(raw * A.SCALE, V.astype(np.float64))
                got, bits = _exact_launch(ops, dev, q, K, V, pos, max_seq, n_splits, tab)
                err = np.abs(got - r.ref)
                worst = max(worst, float((err / r.bound).max()))
                assert (err <= r.bound).all(), (profile, pos, rnd, float((err / r.bound).max()))
                assert (bits[r.ref == 0] == 0).all(), (profile, pos, rnd)                       # no reference mass: +0
    print(f"kv8 exact scores max_seq={max_seq} splits={n_splits} heads=({nh},{nkv}) B={B}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ 4. random inputs
def _random_setup(B, nh, nkv, pos, max_seq, dev, seed):
    g = torch.Generator().manual_seed(seed)
    kc8 = torch.randint(-127, 128, (B, nkv, max_seq, 128), generator=g, dtype=torch.int8)
    vc8 = torch.randint(-127, 128, (B, nkv, max_seq, 128), generator=g, dtype=torch.int8)
    ks = torch.rand(B, nkv, max_seq, generator=g) * 0.03 + 0.005
    vs = torch.rand(B, nkv, max_seq, generator=g) * 0.03 + 0.005
    ks[:, :, pos + 1:] = float("nan"); vs[:, :, pos + 1:] = float("nan")       # rows that must never contribute
    q = torch.randn(B, nh * 128, generator=g).half()
    k = torch.randn(B, nkv * 128, generator=g).half()
    v = torch.randn(B, nkv * 128, generator=g).half()
    return [t.to(dev) for t in (q, k, v, kc8, ks, vc8, vs)]


@pytest.mark.parametrize("max_seq", [64, LONG])
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("B", [1, 3])
def test_random_inputs_against_fp64(max_seq, nh, nkv, B):
    from amq_amd import ops
    dev = _dev()
    tab = ops.rope_table(max_seq, 10000.0, dev)
    for pos in (SHORT_POS if max_seq == 64 else LONG_POS):
        q, k, v, kc8, ks, vc8, vs = _random_setup(B, nh, nkv, pos, max_seq, dev, 31 * pos + nh + B)

        def run(ns, sl=slice(None)):
            c = [t[sl].clone() for t in (kc8, ks, vc8, vs)]
            out = torch.zeros(q[sl].shape[0], nh * 128, dtype=torch.float16, device=dev)
            ops.attn_decode_kv8(q[sl].contiguous(), k[sl].contiguous(), v[sl].contiguous(), *c, out, pos, nh, nkv, table=tab, n_splits=ns)
            return out, c

        one, c1 = run(1)
        qr, kr = q.clone(), k.clone()
        ops.rope_rows(qr, kr, tab, 1, nh, nkv, pos0=pos)                     # the fp16-rotated q
        Kd = kv8_ref.dequantize(c1[0][:, :, :pos + 1], c1[1][:, :, :pos + 1])
        Vd = kv8_ref.dequantize(c1[2][:, :, :pos + 1], c1[3][:, :, :pos + 1])
        ref = kv8_ref.attention64(qr.cpu().view(B, nh, 128).double().numpy(), Kd, Vd).reshape(B, -1)
        mx = np.abs(ref).max()
        for ns in ((1,) if max_seq == 64 else (1, 2, 4)):
            got, c = run(ns)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(c, c1))                    # appended once, the same row
            e = np.abs(got.cpu().double().numpy() - ref).max()
            print(f"kv8 random max_seq={max_seq} pos={pos} splits={ns} heads=({nh},{nkv}) B={B}: max err {e:.3e} of max |ref| {mx:.3e}")
            assert e <= 4e-3 * mx + 1e-3, (pos, ns)
            assert (got.float() - one.float()).abs().max() <= 2e-3 * one.float().abs().max() + 1e-3, (pos, ns)
            again, _ = run(ns)
            assert torch.equal(again, got), (pos, ns)                                             # two runs: equal bits
            for b in range(B):
                alone, _ = run(ns, slice(b, b + 1))
                assert torch.equal(alone[0], got[b]), (pos, ns, b)                                # a batch row = the single-sequence launch
        auto, _ = run(0)
        assert (auto.float() - one.float()).abs().max() <= 2e-3 * one.float().abs().max() + 1e-3
    assert all(int(t.abs().sum().item()) == 0 for t in ops._ATTN_TICKETS._cur.values())           # tickets left zero


# ------------------------------------------------------------------------------------------------------------------ 5. position guard
@pytest.mark.parametrize("bad_pos", ["max_seq", -1])
@pytest.mark.parametrize("n_splits", [1, 3])
def test_position_guard(bad_pos, n_splits):
    from amq_amd import ops, _lib
    dev, nh, nkv, max_seq = _dev(), 8, 2, 1024
    bad = max_seq if bad_pos == "max_seq" else -1
    (kc8, ks, vc8, vs), bands = _caches(2, nkv, max_seq, dev, code_fill=5, scale_fill=0.5)
    before = [t.clone() for t in (kc8, ks, vc8, vs)]
    q = torch.randn(2, nh * 128).half().to(dev); k = torch.randn(2, nkv * 128).half().to(dev); v = torch.randn(2, nkv * 128).half().to(dev)
    out = torch.full((2, nh * 128), 7.0, dtype=torch.float16, device=dev)
    cur, pos_state, err = ops.new_step_state(dev)
    pos_state.fill_(bad)
    ops.attn_decode_kv8(q, k, v, kc8, ks, vc8, vs, out, pos_state, nh, nkv, cur=cur, n_splits=n_splits)
    torch.cuda.synchronize()
    assert int(err.item()) == 1 and bool((out == 7.0).all())
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((kc8, ks, vc8, vs), before)) and _bands_intact(bands)
    with pytest.raises(_lib.AmqError):
        ops.check_step_state(err)
    assert all(int(t.abs().sum().item()) == 0 for t in ops._ATTN_TICKETS._cur.values())
    with pytest.raises(ValueError):
        ops.attn_decode_kv8(q, k, v, kc8, ks, vc8, vs, out, bad, nh, nkv)                         # the host-position form: refused on the host
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------ 6. the runner
def _tiny_cfg(nkv):
    from amq_amd import arch
    return dict(arch._cfg(2, 512, 1024, 4, nkv, 1, vocab=1024))


def _arch_bits(cfg):
    rng = np.random.default_rng(0)
    return {name: [int(b) for b in rng.choice([2, 3, 4], size=2)] for name in cfg["linear"]}


def _step_model(m):
    """tests/kv8_ref.py's stepwise reference over a runner's weights, dequantized by the bit-exact dequantize kernel"""
    from amq_amd import ops
    blocks = []
    for blk in m.blocks:
        d = {name: ops.dequantize(blk[name].qn, blk[name].mn, blk[name].bits, blk[name].mode, blk[name].N, blk[name].K) for name in m.cfg["linear"]}
        d["ln1"], d["ln2"] = blk["ln1"], blk["ln2"]
        blocks.append(d)
    return kv8_ref.StepModel(m.embed, m.norm, m.lm_head, blocks, m.nh, m.nkv, eps=m.eps, theta=m.theta)


def _run(m, ids, steps, graph_from):
    """prompt pass + steps -> [steps + 1] logits rows (clones) and the tokens fed"""
    m.reset()
    out, toks = [m.prefill(ids, use_graph=graph_from == 0).clone()], []
    for step in range(steps):
        toks.append(m.token.clone())
        m.decode_step(use_graph=step >= graph_from)
        out.append(m.logits.clone())
    m.check()
    return out, toks


@pytest.mark.parametrize("nkv", [4, 2])
def test_runner_matches_the_stepwise_reference(nkv):
    from amq_amd.llama import QuantLlama
    cfg = _tiny_cfg(nkv)
    al = _arch_bits(cfg)
    m = QuantLlama(cfg, al, device="cuda:0", max_seq=64, seed=3, kv_bits=8)
    ids = torch.randint(0, 1024, (12,), generator=torch.Generator().manual_seed(5)).to(_dev())
    got, toks = _run(m, ids, 6, graph_from=2)                        # eager launches first, then hipGraph replays
    ref = _step_model(m)
    want = [ref.prompt(ids)] + [ref.step(t) for t in toks]           # fed the runner's own tokens
    scale = want[0].float().abs().max()
    for i, (g, w) in enumerate(zip(got, want)):
        e = float((g.view(-1).float() - w.float()).abs().max() / scale)
        print(f"kv8 runner nkv={nkv} row {i}: max |dlogit| / max |ref| = {e:.2e}")
        assert e <= 2e-2, i
    assert int(m.pos.item()) == 12 + 6
    # the caches: int8 + fp32, 132 / 256 of the fp16 runner's bytes; the prompt pass is the fp16 runner's bit for bit
    m16 = QuantLlama(cfg, al, device="cuda:0", max_seq=64, seed=3)
    assert torch.equal(m16.prefill(ids, use_graph=False), got[0])
    b8 = sum(m.blocks[0][k].numel() * m.blocks[0][k].element_size() for k in ("kc8", "ks", "vc8", "vs"))
    b16 = sum(m16.blocks[0][k].numel() * m16.blocks[0][k].element_size() for k in ("kc", "vc"))
    assert m.blocks[0]["kc8"].dtype is torch.int8 and m.blocks[0]["ks"].dtype is torch.float32 and "kc" not in m.blocks[0]
    assert b8 * 256 == b16 * 132
    assert m.total_bytes_per_token(40) - m.linear_bytes_per_token() - m.lm_head.numel() * 2 == 2 * m.nb * nkv * 132 * 40
    # graph replay == eager, bit for bit, at every step
    eager, _ = _run(m, ids, 6, graph_from=99)
    graph, _ = _run(m, ids, 6, graph_from=0)
    assert all(torch.equal(a, b) for a, b in zip(eager, graph)) and all(torch.equal(a, b) for a, b in zip(eager, got))


def test_runner_batch_rows_equal_single_runs():
    from amq_amd.llama import QuantLlama
    cfg = _tiny_cfg(2)
    ids = torch.randint(0, 1024, (3, 24), generator=torch.Generator().manual_seed(3)).to(_dev())
    mb = QuantLlama(cfg, None, device="cuda:0", max_seq=48, seed=4, batch=3, kv_bits=8)
    out_b = mb.generate(ids, 6, use_graph=False).clone()
    logits_b = mb.logits.float().clone()
    m1 = QuantLlama(cfg, None, device="cuda:0", max_seq=48, seed=4, kv_bits=8)
    for b in range(3):
        m1.reset()
        out_1 = m1.generate(ids[b], 6, use_graph=False)
        ref = m1.logits.float()
        assert (logits_b[b] - ref).abs().max() <= 1e-2 * ref.abs().max()
        assert (out_1 == out_b[b]).float().mean().item() >= 0.8
    mb.reset()
    out_g = mb.generate(ids, 6, use_graph=True)
    assert torch.equal(out_g, out_b) and torch.equal(mb.logits.float(), logits_b)
    mb.check()


def test_runner_long_cache_takes_the_split_path():
    from amq_amd import ops
    from amq_amd.llama import QuantLlama
    cfg = _tiny_cfg(2)
    max_seq, S = 1024, 2 * kv8_ref.CHUNK_MIN + 8
    ns = ops.attn_decode_kv8_splits(max_seq, 4, 1, 2)
    assert ns > 1 and S >= 2 * ops.attn_decode_kv8_chunk(max_seq, ns)              # the step's position lies in the third chunk
    m = QuantLlama(cfg, _arch_bits(cfg), device="cuda:0", max_seq=max_seq, seed=3, kv_bits=8)
    ids = torch.randint(0, 1024, (S,), generator=torch.Generator().manual_seed(6)).to(_dev())
    got, toks = _run(m, ids, 4, graph_from=1)
    ref = _step_model(m)
    want = [ref.prompt(ids)] + [ref.step(t) for t in toks]
    scale = want[0].float().abs().max()
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g.view(-1).float() - w.float()).abs().max() <= 2e-2 * scale, i
    eager, _ = _run(m, ids, 4, graph_from=99)
    assert all(torch.equal(a, b) for a, b in zip(eager, got))
    assert all(int(t.abs().sum().item()) == 0 for t in ops._ATTN_TICKETS._cur.values())


def test_runner_staged_step_on_an_owq_model():
    """the staged (OWQ) step issues the same 8-bit attention launch: a runner over the OWQ tiny model tests/test_gpu_owq_runner.py builds"""
    pytest.importorskip("transformers")
    from test_gpu_owq_runner import modules_of, owq_model
    from amq_amd.llama import QuantLlama
    _, ours, _, _ = owq_model(2)
    r = QuantLlama.from_hf(ours, max_seq=64, kv_bits=8)
    assert r.plan.staged and "kc8" in r.blocks[0]
    ids = torch.randint(0, 1000, (12,), generator=torch.Generator().manual_seed(8)).to(_dev())
    got, toks = _run(r, ids, 6, graph_from=2)
    blocks = []
    for b, layer in enumerate(ours.model.layers):
        d = {name: m.dequantize().half() for bb, name, m in modules_of(ours) if bb == b}
        d["ln1"], d["ln2"] = layer.input_layernorm.weight, layer.post_attention_layernorm.weight
        blocks.append(d)
    cfg = ours.config
    ref = kv8_ref.StepModel(ours.model.embed_tokens.weight, ours.model.norm.weight, ours.lm_head.weight, blocks, cfg.num_attention_heads,
                            cfg.num_key_value_heads, eps=cfg.rms_norm_eps, theta=float(getattr(cfg, "rope_theta", 10000.0)))
    with torch.no_grad():                                            # (the HF parameters ask for gradients)
        want = [ref.prompt(ids)] + [ref.step(t) for t in toks]
    scale = want[0].float().abs().max()
    for i, (g, w) in enumerate(zip(got, want)):
        e = float((g.view(-1).float() - w.float()).abs().max() / scale)
        print(f"kv8 owq runner row {i}: max |dlogit| / max |ref| = {e:.2e}")
        assert e <= 2e-2, i
    r16 = QuantLlama.from_hf(ours, max_seq=64)
    assert torch.equal(r16.prefill(ids, use_graph=False), got[0])


# ------------------------------------------------------------------------------------------------------------------ 7. the surface
def test_refusals_say_why():
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = _tiny_cfg(2)
    for kw in (dict(kv_bits=4), dict(kv_bits=8, ragged=True, batch=2), dict(kv_bits=8, lookup=3), dict(kv_bits=8, engine=True)):
        with pytest.raises(ValueError, match="kv_bits"):
            QuantLlama(cfg, None, device="cuda:0", max_seq=64, **kw)
    with pytest.raises(ValueError, match="kv_bits=8.*q / k norm"):
        QuantLlama(dict(cfg, qk_norm=True), None, device="cuda:0", max_seq=64, kv_bits=8)

    class Fused(QuantLlama):
        FUSE_QKV_ATTN = True
    with pytest.raises(ValueError, match="kv_bits=8.*fused"):
        Fused(cfg, None, device="cuda:0", max_seq=64, kv_bits=8)
    m = QuantLlama(cfg, None, device="cuda:0", max_seq=64, kv_bits=8)
    ids = torch.randint(0, 1024, (8,), generator=torch.Generator().manual_seed(1)).to(_dev())
    m.prefill(ids)
    with pytest.raises(ValueError, match="kv_bits=8.*position 0"):
        m.prefill(ids, start_pos=8)                                  # a chunked prompt
    with pytest.raises(ValueError, match="kv_bits=8"):
        m._prefill_unfused(ids)                                      # the SDPA comparison leg


def test_hf_surface():
    pytest.importorskip("transformers")
    from test_gpu_hf_fast import _hf_generate, _prepared
    from amq_amd import hf_fast
    from amq_amd.llama import QuantLlama
    model, ref = _prepared("llama")
    for kw in (dict(kv_bits=8, lookup=True), dict(kv_bits=8, padded=True), dict(kv_bits=7)):
        with pytest.raises(ValueError, match="kv_bits"):
            hf_fast.convert_model_to_hip(model, **kw)
    hf_fast.convert_model_to_hip(model, kv_bits=8)
    try:
        ids = torch.randint(0, 1000, (1, 20), generator=torch.Generator().manual_seed(2)).to(_dev())
        with torch.inference_mode():
            fast = _hf_generate(model, ids, 10)
            r = hf_fast._RUNNERS[model][1]
            assert r.kv_bits == 8 and r.blocks[0]["kc8"].dtype is torch.int8
            direct = QuantLlama.from_hf(model, max_seq=r.max_seq, kv_bits=8)
            eos = model.generation_config.eos_token_id
            direct.set_suppressed([] if eos is None else eos if isinstance(eos, (list, tuple)) else [eos])       # fixed-length calls never emit EOS
            assert torch.equal(fast[0, 20:], direct.generate(ids[0], 10).view(-1).to(fast.dtype))        # token for token
            # prompt-pass logits against HF's own forward over the oracle's weights: the bar of tests/test_gpu_hf_fast.py
            lg = model(ids, start_pos=0, use_cache=False).logits
            want = ref(ids).logits.float()
            assert (lg - want).abs().max() <= 6e-3 * want.abs().max()
            # a one-row step at the runner's position is served; a many-row call behind cached rows raises
            step = model(fast[:, 20:21], start_pos=20, use_cache=False)
            assert step.logits.shape == (1, 1, 1000) and step["start_pos"] == 21
            with pytest.raises(ValueError, match="kv_bits=8"):
                model(ids[:, :4], start_pos=21, use_cache=False)
            # sampled generate is served too
            hf_fast.convert_model_to_hip(model, sampling=True, kv_bits=8)
            torch.manual_seed(3)
            s1 = model.generate(ids, min_new_tokens=8, max_new_tokens=8, do_sample=True, top_k=20, attention_mask=torch.ones_like(ids), pad_token_id=0)
            torch.manual_seed(3)
            s2 = model.generate(ids, min_new_tokens=8, max_new_tokens=8, do_sample=True, top_k=20, attention_mask=torch.ones_like(ids), pad_token_id=0)
            assert torch.equal(s1, s2) and s1.shape == (1, 28)
    finally:
        hf_fast.revert_model_to_hf(model)


def test_hf_surface_runner_growth_carries_codes_and_scales():
    """a sequence that outgrows its runner's cache (256 -> 512 rows: the model of max_position_embeddings 512 the hf_fast tests build): the rebuilt
    runner carries codes and scales over, and the tokens are those of a runner built large enough at once.  (Below 256 keys both runners' attention
    launches have one active chunk: the same arithmetic, so the tokens are equal, not merely close.)"""
    pytest.importorskip("transformers")
    from test_gpu_hf_fast import _hf_generate, _prepared
    from amq_amd import hf_fast
    from amq_amd.llama import QuantLlama
    model, _ = _prepared("llama3.1")
    hf_fast.convert_model_to_hip(model, kv_bits=8)
    try:
        ids = torch.randint(0, 1000, (1, 120), generator=torch.Generator().manual_seed(4)).to(_dev())
        with torch.inference_mode():
            first = _hf_generate(model, ids, 10)                      # 130 positions: a runner of 256
            r0 = hf_fast._RUNNERS[model][1]
            assert r0.max_seq == 256 and r0.host_pos == 129
            tok, grown = first[:, -1:].clone(), []
            for p in range(129, 129 + 6):                             # one-row steps: the first asks for 2 x 130 positions -> rebuilt at 512
                o = model(tok, start_pos=p, use_cache=False)
                tok = o.logits[:, -1].argmax(-1).view(1, 1)
                grown.append(int(tok))
            r1 = hf_fast._RUNNERS[model][1]
            assert r1 is not r0 and r1.max_seq == 512 and r1.kv_bits == 8 and r1.host_pos == 135
            for nb, ob in zip(r1.blocks, r0.blocks):
                for key in ("kc8", "ks", "vc8", "vs"):
                    assert torch.equal(_bits(nb[key][:, :, :129]), _bits(ob[key][:, :, :129]))
            big = QuantLlama.from_hf(model, max_seq=512, kv_bits=8)
            eos = model.generation_config.eos_token_id
            big.set_suppressed([] if eos is None else eos if isinstance(eos, (list, tuple)) else [eos])
            whole = big.generate(ids[0], 10).view(-1)
            assert torch.equal(whole, first[0, 120:].to(whole.dtype))
            big.set_suppressed(())
            more = []
            for _ in range(6):
                big.decode_step()
                more.append(int(big.token))
            assert more == grown
    finally:
        hf_fast.revert_model_to_hf(model)
