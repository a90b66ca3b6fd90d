"""Qwen3's per-head q / k RMSNorm inside the rotating kernels (the amq_*_qkn_f16 entry points) and the runner over a tiny Qwen3ForCausalLM.

Kernel level, through ``ops``: every rotating kernel against the CPU restatements of tests/qknorm_ref.py (fp64 for outputs, fp16 for the appended key
row) and against each other bit for bit -- the row a prompt pass writes, the row a decode step appends (per-head, split, grouped-query kernel) and
the row a ``rows`` workgroup rotates for itself are the same bits.  Model level: QuantLlama.from_hf / convert_model_to_hip over a 2-layer Qwen3
(hidden 256, q width 512) against HF's own eager forward over the same swapped modules."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qknorm_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6


def _dev():
    return torch.device(DEV)


def _gammas(g):
    """weights drawn as 1 + 0.2 randn, so that a missing gamma shows"""
    return ((1 + 0.2 * torch.randn(128, generator=g)).half().to(_dev()), (1 + 0.2 * torch.randn(128, generator=g)).half().to(_dev()))


def _ulps(a, b):
    """|a - b| in fp16 ulps of the larger magnitude (normal range)"""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    mag = torch.maximum(a.abs(), b.abs()).clamp_min(2.0 ** -14)
    return ((a - b).abs() / 2.0 ** (torch.floor(torch.log2(mag)) - 10)).max().item()


def _state1(ops, tab, max_seq, pos):
    """the one-block step state at ``pos``"""
    cur, posd, err = ops.new_step_state(_dev())
    cur.copy_(tab.view(max_seq, 128)[pos])
    posd.fill_(pos)
    return cur, posd, err


def _state(ops, tab, max_seq, positions):
    cur, pos, err = ops.new_step_state(_dev(), batch=len(positions))
    pos.copy_(torch.tensor(positions, dtype=torch.int32))
    cur.copy_(tab.view(max_seq, 128)[torch.tensor(positions, device=_dev())])
    return cur, pos, err


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("nh,nkv", [(2, 2), (4, 1)])
def test_per_head_kernel_against_the_restatements(nh, nkv):
    """tokens fed one by one into an empty cache of 64 rows; at positions 0, 1, 37: the output against the fp64 restatement of the whole chain
    (rtol 1e-2, atol 3e-3: tests/test_gpu_decode.py's bar for this comparison), the appended key row against the fp16 restatement within 2 fp16
    ulps (the fp32 sum order may move fp16(x * rstd) by one ulp before gamma and the rotation), every element; the value row bit for bit.
    Both position sources (table, step state) give the same bits."""
    from amq_amd import ops
    dev, max_seq = _dev(), 64
    g = torch.Generator().manual_seed(11 * nh + nkv)
    gq, gk = _gammas(g)
    tab = ops.rope_table(max_seq, 10000.0, dev)
    kc = torch.zeros(1, nkv, max_seq, 128, dtype=torch.float16, device=dev)
    vc = torch.zeros_like(kc)
    out = torch.zeros(1, nh * 128, dtype=torch.float16, device=dev)
    K64, V64 = [], []
    for pos in range(38):
        q = torch.randn(1, nh * 128, generator=g).half().to(dev)
        k = torch.randn(1, nkv * 128, generator=g).half().to(dev) * (0.5 + pos % 3)        # (the norm removes the scale)
        v = torch.randn(1, nkv * 128, generator=g).half().to(dev)
        cos, sin = ref.table_cos_sin(tab.view(max_seq, 128)[pos])
        if pos % 2:
            cur, posd, err = _state1(ops, tab, max_seq, pos)
            ops.attn_decode(q, k, v, kc, vc, out, posd, nh, nkv, cur=cur, q_norm=gq, k_norm=gk, norm_eps=EPS)
            assert err.tolist() == [0]
        else:
            ops.attn_decode(q, k, v, kc, vc, out, pos, nh, nkv, table=tab, q_norm=gq, k_norm=gk, norm_eps=EPS)
        K64.append(ref.norm_rope_f64(k.view(nkv, 128), gk, EPS, cos, sin))
        V64.append(v.view(nkv, 128).cpu().double())
        if pos in (0, 1, 37):
            k16 = ref.norm_rope_f16(k.view(nkv, 128), gk, EPS, cos, sin)
            u = _ulps(kc[0, :, pos], k16)
            q64 = ref.norm_rope_f64(q.view(nh, 128), gq, EPS, cos, sin)
            want = ref.attention_f64(q64, torch.stack(K64, 1).repeat_interleave(nh // nkv, 0), torch.stack(V64, 1).repeat_interleave(nh // nkv, 0))
            got = out[0].cpu().double().view(nh, 128)
            print(f"per-head nh={nh} nkv={nkv} pos={pos}: key row {u:.2f} ulp, max|out - f64| = {(got - want).abs().max().item():.3e}")
            assert u <= 2.0
            assert torch.equal(vc[0, :, pos], v.view(nkv, 128))
            assert torch.allclose(got, want, rtol=1e-2, atol=3e-3)
            # without the weights the same call gives something else: the norm is not a no-op of this test
            kc2, vc2, out2 = kc.clone(), vc.clone(), torch.zeros_like(out)
            ops.attn_decode(q, k, v, kc2, vc2, out2, pos, nh, nkv, table=tab)
            assert not torch.equal(kc2[0, :, pos], kc[0, :, pos])


@pytest.mark.parametrize("nh,nkv", [(4, 1), (2, 2)])
def test_split_kernel(nh, nkv):
    """max_seq 1024, position 600: the per-head split kernel (n_splits forced per query head through a multi-head copy for the grouped shape) against
    fp64 at 4e-3 max + 1e-3; with one active chunk bit-identical to the single-workgroup kernel"""
    from amq_amd import ops
    dev, max_seq, pos = _dev(), 1024, 600
    g = torch.Generator().manual_seed(5 + nh)
    gq, gk = _gammas(g)
    tab = ops.rope_table(max_seq, 10000.0, dev)
    # every query head its own copy of its kv head: the per-head split kernel also for the grouped shape (the grouped kernel has its own test)
    kc = torch.zeros(1, nh, max_seq, 128, dtype=torch.float16, device=dev)
    vc = torch.zeros_like(kc)
    rows = torch.randn(2, nkv, pos, 128, generator=g).half().to(dev)
    kc[0, :, :pos] = rows[0].repeat_interleave(nh // nkv, 0)
    vc[0, :, :pos] = rows[1].repeat_interleave(nh // nkv, 0)
    kc[:, :, pos + 1:] = float("nan"); vc[:, :, pos + 1:] = float("nan")
    q = torch.randn(1, nh * 128, generator=g).half().to(dev)
    k1 = torch.randn(1, nkv, 128, generator=g).half().to(dev)
    v1 = torch.randn(1, nkv, 128, generator=g).half().to(dev)
    k = k1.repeat_interleave(nh // nkv, 1).reshape(1, -1).contiguous()
    v = v1.repeat_interleave(nh // nkv, 1).reshape(1, -1).contiguous()

    def run(ns, p=pos):
        kc_, vc_ = kc.clone(), vc.clone()
        out = torch.zeros(1, nh * 128, dtype=torch.float16, device=dev)
        c, pd, e = _state1(ops, tab, max_seq, p)
        ops.attn_decode(q, k, v, kc_, vc_, out, pd, nh, nh, cur=c, n_splits=ns, q_norm=gq, k_norm=gk, norm_eps=EPS)
        assert e.tolist() == [0]
        return out, kc_

    one, kc1 = run(1)
    got, kc2 = run(3)                                     # three active chunks of 256 keys
    assert torch.equal(kc2[0, :, :pos + 1], kc1[0, :, :pos + 1])
    cos, sin = ref.table_cos_sin(tab.view(max_seq, 128)[pos])
    K = torch.cat([kc[0, :, :pos].cpu().double(), ref.norm_rope_f64(k.view(nh, 128), gk, EPS, cos, sin)[:, None]], 1)
    V = torch.cat([vc[0, :, :pos].cpu().double(), v.view(nh, 128).cpu().double()[:, None]], 1)
    want = ref.attention_f64(ref.norm_rope_f64(q.view(nh, 128), gq, EPS, cos, sin), K, V).reshape(-1)
    for name, o in (("single", one), ("split", got)):
        err = (o[0].cpu().double() - want).abs().max().item()
        print(f"split nh={nh} nkv={nkv} {name}: max|out - f64| = {err:.3e} (bar {4e-3 * want.abs().max().item() + 1e-3:.3e})")
        assert err <= 4e-3 * want.abs().max().item() + 1e-3
    assert _ulps(kc2[0, :, pos], ref.norm_rope_f16(k.view(nh, 128), gk, EPS, cos, sin)) <= 2.0
    if nh != nkv:
        # the grouped shape as ops routes it over a long cache (one kv head, the matrix-core kernel): the same bar against fp64, the same cache row
        kcg, vcg = kc[:, ::nh // nkv].contiguous(), vc[:, ::nh // nkv].contiguous()
        outg = torch.zeros(1, nh * 128, dtype=torch.float16, device=dev)
        c, pd, e = _state1(ops, tab, max_seq, pos)
        ops.attn_decode(q, k1.reshape(1, -1).contiguous(), v1.reshape(1, -1).contiguous(), kcg, vcg, outg, pd, nh, nkv, cur=c, n_splits=3, q_norm=gq,
                        k_norm=gk, norm_eps=EPS)
        assert e.tolist() == [0]
        err = (outg[0].cpu().double() - want).abs().max().item()
        print(f"split nh={nh} nkv={nkv} grouped route: max|out - f64| = {err:.3e}")
        assert err <= 4e-3 * want.abs().max().item() + 1e-3
        assert torch.equal(kcg[0, :, pos], kc2[0, ::nh // nkv, pos])
    # one active chunk (T <= 256): the single-workgroup kernel's bits
    a, ka = run(1, 200)
    b, kb = run(3, 200)
    assert torch.equal(a, b) and torch.equal(ka[0, :, 200], kb[0, :, 200])


@pytest.mark.parametrize("nh,nkv", [(8, 2), (7, 1)])
@pytest.mark.parametrize("pos", [530, 1000])
def test_gqa_matrix_core_kernel(nh, nkv, pos):
    """the grouped-query kernel (queries normalised and rotated in MFMA-fragment registers) against fp64 at the same bar; the cache row it writes
    is the per-head kernel's bit for bit"""
    from amq_amd import ops
    dev, max_seq = _dev(), 1024
    g = torch.Generator().manual_seed(pos + nh)
    gq, gk = _gammas(g)
    tab = ops.rope_table(max_seq, 10000.0, dev)
    kc = torch.zeros(2, nkv, max_seq, 128, dtype=torch.float16, device=dev)
    vc = torch.zeros_like(kc)
    kc[:, :, :pos] = torch.randn(2, nkv, pos, 128, generator=g).half().to(dev)
    vc[:, :, :pos] = torch.randn(2, nkv, pos, 128, generator=g).half().to(dev)
    kc[:, :, pos + 1:] = float("nan"); vc[:, :, pos + 1:] = float("nan")
    q = torch.randn(2, nh * 128, generator=g).half().to(dev)
    k = torch.randn(2, nkv * 128, generator=g).half().to(dev)
    v = torch.randn(2, nkv * 128, generator=g).half().to(dev)
    n_splits = ops.attn_decode_splits(max_seq, nh, 2, nkv)
    assert n_splits >= 2                                   # the grouped route (amq_kernels.h: attn_decode_takes_gqa)

    def run(ns):
        kc_, vc_ = kc.clone(), vc.clone()
        out = torch.zeros(2, nh * 128, dtype=torch.float16, device=dev)
        c, pd, e = ops.new_step_state(dev)
        c.copy_(tab.view(max_seq, 128)[pos]); pd.fill_(pos)
        ops.attn_decode(q, k, v, kc_, vc_, out, pd, nh, nkv, cur=c, n_splits=ns, q_norm=gq, k_norm=gk, norm_eps=EPS)
        assert int(e.item()) == 0
        return out, kc_, vc_

    got, kc_g, vc_g = run(n_splits)
    one, kc_1, vc_1 = run(1)                              # one workgroup per query head
    assert torch.equal(kc_g[:, :, :pos + 1], kc_1[:, :, :pos + 1]) and torch.equal(vc_g[:, :, :pos + 1], vc_1[:, :, :pos + 1])
    assert torch.isnan(kc_g[:, :, pos + 1:]).all()
    cos, sin = ref.table_cos_sin(tab.view(max_seq, 128)[pos])
    for b in range(2):
        K = torch.cat([kc[b, :, :pos].cpu().double(), ref.norm_rope_f64(k[b].view(nkv, 128), gk, EPS, cos, sin)[:, None]], 1)
        V = torch.cat([vc[b, :, :pos].cpu().double(), v[b].view(nkv, 128).cpu().double()[:, None]], 1)
        want = ref.attention_f64(ref.norm_rope_f64(q[b].view(nh, 128), gq, EPS, cos, sin), K.repeat_interleave(nh // nkv, 0),
                                 V.repeat_interleave(nh // nkv, 0)).reshape(-1)
        err = (got[b].cpu().double() - want).abs().max().item()
        print(f"gqa nh={nh} nkv={nkv} pos={pos} b={b}: max|out - f64| = {err:.3e} (bar {4e-3 * want.abs().max().item() + 1e-3:.3e})")
        assert err <= 4e-3 * want.abs().max().item() + 1e-3


@pytest.mark.parametrize("p,max_seq,n_splits,nh,nkv", [(20, 64, 1, 4, 2), (600, 1024, 3, 4, 4)])
def test_rows_form_equals_successive_single_rows(p, max_seq, n_splits, nh, nkv):
    """R = 3 rows at p = 20 (single form) / p = 600 (split form, three active chunks): row j is the per-sequence kernel at p + j over a cache that
    already holds the rows, bit for bit, and the appended rows are the same bits -- tests/test_gpu_lookup.py's property, with the norm.  (The split
    case is multi-head: a grouped shape's per-sequence split call takes the matrix-core kernel, which is other arithmetic.)"""
    from amq_amd import ops
    dev, R = _dev(), 3
    g = torch.Generator().manual_seed(p)
    gq, gk = _gammas(g)
    tab = ops.rope_table(max_seq, 10000.0, dev)
    kc = torch.full((1, nkv, max_seq, 128), float("nan"), dtype=torch.float16, device=dev)
    vc = torch.full_like(kc, float("nan"))
    kc[0, :, :p] = torch.randn(nkv, p, 128, generator=g).half().to(dev)
    vc[0, :, :p] = torch.randn(nkv, p, 128, generator=g).half().to(dev)
    q = torch.randn(R, nh * 128, generator=g).half().to(dev)
    k = torch.randn(R, nkv * 128, generator=g).half().to(dev)
    v = torch.randn(R, nkv * 128, generator=g).half().to(dev)
    kw = dict(q_norm=gq, k_norm=gk, norm_eps=EPS)
    # the oracle: R successive one-row calls of the per-sequence form with the same split, each appending its row
    kc_r, vc_r = kc.clone(), vc.clone()
    want = torch.zeros(R, nh * 128, dtype=torch.float16, device=dev)
    for j in range(R):
        c1, p1, e1 = _state(ops, tab, max_seq, [p + j])
        ops.attn_decode(q[j:j + 1].contiguous(), k[j:j + 1].contiguous(), v[j:j + 1].contiguous(), kc_r, vc_r, want[j:j + 1], p1, nh, nkv, cur=c1,
                        n_splits=n_splits, **kw)
        assert e1.tolist() == [0]
    kc_g, vc_g = kc.clone(), vc.clone()
    got = torch.zeros(R, nh * 128, dtype=torch.float16, device=dev)
    cur, pos, err = _state(ops, tab, max_seq, [p + j for j in range(R)])
    ops.attn_decode_rows(q, k, v, kc_g, vc_g, got, cur, pos, nh, nkv, n_splits=n_splits, **kw)
    assert err.tolist() == [0] * R
    assert torch.equal(kc_g[0, :, :p + R], kc_r[0, :, :p + R]) and torch.equal(vc_g[0, :, :p + R], vc_r[0, :, :p + R])
    assert torch.isnan(kc_g[0, :, p + R:]).all()
    for j in range(R):
        print(f"rows p={p} row={j} splits={n_splits}: max|diff| = {(got[j].float() - want[j].float()).abs().max().item():.3e}")
        assert torch.equal(got[j], want[j]), j


@pytest.mark.parametrize("pos0", [0, 9])
def test_prompt_kernels_write_what_decode_steps_append(pos0):
    """rope_cache / rope_rows on S = 5 rows of 2 sequences: q rows and cache rows are the bits S decode steps rotate and append"""
    from amq_amd import ops
    dev, nh, nkv, S, B, max_seq = _dev(), 4, 2, 5, 2, 32
    g = torch.Generator().manual_seed(40 + pos0)
    gq, gk = _gammas(g)
    kw = dict(q_norm=gq, k_norm=gk, norm_eps=EPS)
    tab = ops.rope_table(max_seq, 10000.0, dev)
    q = torch.randn(B * S, nh * 128, generator=g).half().to(dev)
    k = torch.randn(B * S, nkv * 128, generator=g).half().to(dev)
    v = torch.randn(B * S, nkv * 128, generator=g).half().to(dev)
    kc = torch.zeros(B, nkv, max_seq, 128, dtype=torch.float16, device=dev)
    vc = torch.zeros_like(kc)
    kc[:, :, :pos0] = torch.randn(B, nkv, pos0, 128, generator=g).half().to(dev)
    vc[:, :, :pos0] = torch.randn(B, nkv, pos0, 128, generator=g).half().to(dev)
    # S decode steps per sequence (batch 2, one shared position per step)
    kc_d, vc_d = kc.clone(), vc.clone()
    out = torch.zeros(B, nh * 128, dtype=torch.float16, device=dev)
    for s in range(S):
        rows = torch.tensor([b * S + s for b in range(B)], device=dev)
        ops.attn_decode(q[rows].contiguous(), k[rows].contiguous(), v[rows].contiguous(), kc_d, vc_d, out, pos0 + s, nh, nkv, table=tab, **kw)
    # the prompt pass
    q_c, kc_p, vc_p = q.clone(), kc.clone(), vc.clone()
    ops.rope_cache(q_c, k, v, kc_p, vc_p, tab, pos0, nh, nkv, **kw)
    assert torch.equal(kc_p, kc_d) and torch.equal(vc_p, vc_d)
    # one sequence, 3-D caches: the same rows
    q_1, kc_1, vc_1 = q[:S].clone(), kc[0].clone(), vc[0].clone()
    ops.rope_cache(q_1, k[:S].contiguous(), v[:S].contiguous(), kc_1, vc_1, tab, pos0, nh, nkv, **kw)
    assert torch.equal(kc_1, kc_d[0]) and torch.equal(q_1, q_c[:S])
    # rope_rows: q and k in place, the same bits
    q_r, k_r = q.clone(), k.clone()
    ops.rope_rows(q_r, k_r, tab, S, nh, nkv, pos0=pos0, **kw)
    assert torch.equal(q_r, q_c)
    assert torch.equal(k_r.view(B, S, nkv, 128).transpose(1, 2), kc_d[:, :, pos0:pos0 + S])
    # ... and q is the fp16 restatement within 2 ulps (what the decode kernels rotate is not observable: their outputs are checked above)
    for r in (0, S - 1, B * S - 1):
        cos, sin = ref.table_cos_sin(tab.view(max_seq, 128)[pos0 + r % S])
        assert _ulps(q_c[r].view(nh, 128), ref.norm_rope_f16(q[r].view(nh, 128), gq, EPS, cos, sin)) <= 2.0
    # without the weights: the kernels as they were
    q_n, k_n = q.clone(), k.clone()
    ops.rope_rows(q_n, k_n, tab, S, nh, nkv, pos0=pos0)
    assert not torch.equal(q_n, q_r)


def test_wrappers_refuse_bad_norms():
    from amq_amd import ops
    dev = _dev()
    g = torch.ones(128, dtype=torch.float16, device=dev)
    q = torch.zeros(1, 256, dtype=torch.float16, device=dev)
    kc = torch.zeros(1, 2, 16, 128, dtype=torch.float16, device=dev)
    with pytest.raises(ValueError, match="go together"):
        ops.attn_decode(q, q, q, kc, kc.clone(), q.clone(), 0, 2, 2, q_norm=g)
    with pytest.raises(ValueError, match="128 elements"):
        ops.attn_decode(q, q, q, kc, kc.clone(), q.clone(), 0, 2, 2, q_norm=g, k_norm=torch.ones(64, dtype=torch.float16, device=dev))
    with pytest.raises(ValueError, match="must be in GPU memory"):
        ops.rope_rows(q.clone(), q.clone(), ops.rope_table(16, 10000.0, dev), 1, 2, 2, q_norm=g.cpu(), k_norm=g)


# ------------------------------------------------------------------------------------------------------------------ the model
NAMES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _swap_linears(model, bits_cycle=(4, 2, 3, 3, 2, 4, 3), seed=100):
    """every decoder linear -> an HQQ stand-in of its shape (random HQQ weights)"""
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
                h.bias = None
                setattr(parent, name, HQQWeightsModule(h.to(torch.device(DEV))))
    return model


def _prepared(tie):
    """tests/test_gpu_hf_fast.py::_prepared for a tiny Qwen3: 2 layers, hidden 256, 4 / 2 heads of 128 (q width 512), norm weights 1 + 0.2 randn"""
    transformers = pytest.importorskip("transformers")
    from amq_amd.patching import prepare_for_inference
    torch.manual_seed(0)
    cfg = transformers.Qwen3Config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                   head_dim=128, vocab_size=1000, max_position_embeddings=1024, rms_norm_eps=1e-6, attn_implementation="eager",
                                   tie_word_embeddings=tie)
    m = transformers.Qwen3ForCausalLM(cfg)
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.q_norm.weight.copy_(1 + 0.2 * torch.randn(128))
            layer.self_attn.k_norm.weight.copy_(1 + 0.2 * torch.randn(128))
    m = _swap_linears(m.to(torch.float16).to(DEV).eval())
    prepare_for_inference(m, backend="hip")
    return m


@pytest.fixture(scope="module", params=[True, False], ids=["tied", "untied"])
def model(request):
    return _prepared(request.param)


@pytest.fixture(scope="module")
def untied():
    return _prepared(False)


def _hf_generate(model, ids, n):
    return model.generate(ids, min_new_tokens=n, max_new_tokens=n, do_sample=False, num_beams=1, attention_mask=torch.ones_like(ids), pad_token_id=0)


def _assert_same_tokens_or_a_tie(model, fast, slow, n_prompt):
    """tests/test_gpu_hf_fast.py's rule: equal tokens, or -- at the first step where they part -- a near-tie (gap <= 4e-3 max|logit|) under HF's own
    logits for the common prefix; what follows a parted step is not comparable"""
    if torch.equal(fast, slow):
        return
    for b in range(fast.shape[0]):
        diff = (fast[b] != slow[b]).nonzero()
        if len(diff) == 0:
            continue
        t = int(diff[0])
        assert t >= n_prompt
        with torch.inference_mode():
            lg = model(slow[b:b + 1, :t]).logits[0, -1].float()
        gap = float(lg.max() - lg[int(fast[b, t])])
        assert gap <= 4e-3 * float(lg.abs().max()), (b, t, gap, fast[b, n_prompt:].tolist(), slow[b, n_prompt:].tolist())


def test_from_hf_matches_hf_eager_forward(model):
    """a 9-token prompt + 8 greedy steps: logits within 2e-2 * scale of HF's own eager forward over the same swapped modules (teacher-forced with the
    runner's tokens); graph replay == the eager walk bit for bit.  (The parent commit: ValueError 'per-head q / k norms are not part of the
    runner's block'.)"""
    from amq_amd.llama import QuantLlama
    ids = torch.randint(5, 1000, (9,), generator=torch.Generator().manual_seed(1)).to(DEV)
    r = QuantLlama.from_hf(model, max_seq=64)
    assert r.qk_norm and r.qd == 512 and r.H == 256 and r.engine is None and not r.can_fuse_qkv_attn
    assert r.blocks[0]["qn"].data_ptr() == model.model.layers[0].self_attn.q_norm.weight.data_ptr()       # the module's own tensor
    assert (r.lm_head.data_ptr() == r.embed.data_ptr()) == bool(model.config.tie_word_embeddings)
    runs = {}
    for use_graph in (False, True):
        r.reset()
        lg = [r.prefill(ids, use_graph=use_graph).float().clone()]
        toks = [int(r.token.item())]
        for _ in range(8):
            r.decode_step(use_graph)
            lg.append(r.logits.float().clone())
            toks.append(int(r.token.item()))
        r.check()
        runs[use_graph] = (torch.stack(lg), toks)
    assert runs[True][1] == runs[False][1] and torch.equal(runs[True][0], runs[False][0])
    lg, toks = runs[False]
    seq = torch.cat([ids, torch.tensor(toks[:-1], device=DEV)])[None]
    with torch.inference_mode():
        want = model(seq).logits[0, 8:].float()
    scale = float(want.abs().max())
    err = float((lg - want).abs().max())
    print(f"from_hf tie={model.config.tie_word_embeddings}: max|logits - HF| = {err:.3e} (bar {2e-2 * scale:.3e})")
    assert err <= 2e-2 * scale


@pytest.mark.parametrize("B", [1, 2])
def test_converted_model_generates_hf_tokens(model, B):
    from amq_amd.hf_fast import convert_model_to_hip, revert_model_to_hf
    ids = torch.randint(5, 1000, (B, 9), generator=torch.Generator().manual_seed(2 + B)).to(DEV)
    slow = _hf_generate(model, ids, 8)
    convert_model_to_hip(model, sampling=True, padded=True, lookup=True)
    try:
        fast = _hf_generate(model, ids, 8)
    finally:
        revert_model_to_hf(model)
    assert fast.shape == slow.shape and torch.equal(fast[:, :12], slow[:, :12]), (fast[:, 9:].tolist(), slow[:, 9:].tolist())
    _assert_same_tokens_or_a_tie(model, fast, slow, 9)


def test_ragged_rows_equal_their_single_runs(untied):
    from amq_amd.llama import QuantLlama
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(5, 1000, (L,), generator=g).to(DEV) for L in (5, 9)]
    ids = torch.zeros(2, 9, dtype=torch.int64, device=DEV)
    for b, p in enumerate(prompts):
        ids[b, :p.numel()] = p
    r2 = QuantLlama.from_hf(untied, max_seq=64, batch=2, ragged=True)
    got = r2.generate(ids, 6, lengths=[5, 9])
    r2.check()
    r1 = QuantLlama.from_hf(untied, max_seq=64)
    for b, p in enumerate(prompts):
        assert torch.equal(got[b], r1.generate(p, 6)), b


def test_lookup_drafts_do_not_change_the_output(untied):
    """never-right, always-right and looked-up drafts give the same tokens and the same row-0 logits (tests/test_gpu_lookup.py's statement), over
    normed cache rows: what a ROWS workgroup rotates for itself is what the row's own workgroup appends"""
    from amq_amd.llama import QuantLlama
    D, n, S, SUP = 3, 10, 12, 3
    ids = torch.randint(8, 1000, (6,), generator=torch.Generator().manual_seed(9)).repeat(2).to(DEV)
    m = QuantLlama.from_hf(untied, max_seq=64, lookup=D)

    def run(mode, refs=None, use_graph=False):
        m.reset()
        m.set_suppressed([SUP])
        m.set_lookup_mode(mode != "lookup")
        m.prefill(ids, use_graph=use_graph)
        rows0 = {0: m.logits.view(m.R, -1)[0].float().clone()}
        count, _ = m.lookup_sync()
        while count - S < n:
            e = count - S
            if mode == "never":
                m.verify_step([SUP] * D, use_graph=use_graph)
            elif mode == "right":
                d = refs[e:e + D].tolist()
                m.verify_step(d + [-1] * (D - len(d)), use_graph=use_graph)
            else:
                m.decode_step(use_graph)
            count, _ = m.lookup_sync()
            rows0[e] = m.logits.view(m.R, -1)[0].float().clone()
        m.check()
        return m.history[S:S + n].to(torch.int64).clone(), rows0

    never, rows_n = run("never")
    right, rows_r = run("right", never)
    looked, rows_l = run("lookup")
    graph, rows_g = run("right", never, use_graph=True)
    assert torch.equal(right, never) and torch.equal(looked, never) and torch.equal(graph, never)
    assert len(rows_r) < len(rows_n)                      # always-right drafts take fewer steps
    for rows in (rows_r, rows_l, rows_g):
        for e, lg in rows.items():
            assert torch.equal(lg, rows_n[e]), e
    # ... and they are the plain one-row runner's greedy tokens, or part at a near-tie of its own logits
    m1 = QuantLlama.from_hf(untied, max_seq=64)
    m1.set_suppressed([SUP])
    m1.prefill(ids, use_graph=False)
    for i in range(n):
        lg = m1.logits.float()
        if int(m1.token.item()) != int(never[i]):
            lg[SUP] = float("-inf")
            assert float(lg.max() - lg[int(never[i])]) <= 4e-3 * float(lg[torch.isfinite(lg)].abs().max()), i
            break
        if i + 1 < n:
            m1.decode_step(False)


def test_sampling_is_reproducible_graph_and_eager(untied):
    from amq_amd.llama import QuantLlama
    ids = torch.randint(5, 1000, (9,), generator=torch.Generator().manual_seed(4)).to(DEV)
    r = QuantLlama.from_hf(untied, max_seq=64)
    r.set_sampling(0.9, 40, 0.95, seed=1234)
    a = r.generate(ids, 8, use_graph=False)
    b = r.generate(ids, 8, use_graph=True)
    c = r.generate(ids, 8, use_graph=True)
    r.set_sampling(0.9, 40, 0.95, seed=99)
    d = r.generate(ids, 8, use_graph=True)
    r.check()
    assert torch.equal(a, b) and torch.equal(b, c) and a.shape == (8,)
    assert not torch.equal(a, d)                          # (another seed, other draws: the seed is what fixes them)


def test_long_cache_chunked_prompt_then_steps(untied):
    """max_seq 1024, a 600-token prompt fed in two chunks, then 4 steps: logits against one whole-prompt pass at 1e-2 * scale -- the chunked prompt
    pass and the long-cache decode route (4 / 2 heads: the grouped-query kernel) over normed cache rows"""
    from amq_amd import ops
    from amq_amd.llama import QuantLlama
    ids = torch.randint(5, 1000, (600,), generator=torch.Generator().manual_seed(6)).to(DEV)
    r = QuantLlama.from_hf(untied, max_seq=1024)
    assert ops.attn_decode_splits(1024, r.nh, 1, r.nkv) > 1
    whole = [r.prefill(ids, use_graph=False).float().clone()]
    toks = [r.token.clone()]
    for _ in range(4):
        r.decode_step(False)
        whole.append(r.logits.float().clone())
        toks.append(r.token.clone())
    r.check()
    r.reset()
    r.prefill(ids[:352], use_graph=False)
    got = [r.prefill(ids[352:], use_graph=False, start_pos=352).float().clone()]
    for i in range(4):
        r.set_token(toks[i])                              # (the whole-prompt run's tokens: the same sequence in both runs)
        r.decode_step(False)
        got.append(r.logits.float().clone())
    r.check()
    for i, (a, b) in enumerate(zip(got, whole)):
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        print(f"long cache step {i}: max|chunked - whole| = {err:.3e} (bar {1e-2 * scale:.3e})")
        assert err <= 1e-2 * scale, i


def test_a_qk_norm_step_is_still_five_launches_per_block():
    """the recorded ops calls of one eager step of a qk_norm runner (tests/test_gpu_step_plan.py's way): per block the five launches of every other
    model, the attention launch carrying the norm weights -- no launch in front of attention; the A/B step forms refuse the model"""
    from amq_amd import arch, ops
    from amq_amd.llama import QuantLlama
    m = QuantLlama(arch.MODEL_CONFIGS["tiny-qwen3-test"], max_seq=32, device=DEV)
    assert m.qk_norm and m.qd == 512 and m.H == 256
    m.prefill(torch.randint(0, 999, (4,), generator=torch.Generator().manual_seed(1)), use_graph=False)
    names = ("gemv_grouped", "gemv_grouped_sums", "gemv", "rmsnorm", "silu_mul", "attn_decode", "attn_decode_rows", "rope_rows", "rope_cache", "gemm",
             "linear", "gemv_f16w", "decode_tail", "decode_tail_sample", "decode_tail_lookup", "set_token")
    calls, saved = [], {n: getattr(ops, n) for n in names}
    try:
        for n in names:
            def wrapped(*a, _n=n, _f=saved[n], **k):
                calls.append((_n, k))
                return _f(*a, **k)
            setattr(ops, n, wrapped)
        m._step()
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
    torch.cuda.synchronize()
    m.check()
    launched = [n for n, _ in calls]
    block = ["gemv_grouped", "attn_decode", "gemv_grouped", "gemv_grouped", "gemv_grouped"]
    assert launched == block * 2 + ["gemv_f16w", "decode_tail"], launched
    for n, k in calls:
        if n == "attn_decode":
            assert k["q_norm"].shape == (128,) and k["k_norm"].shape == (128,) and k["norm_eps"] == 1e-6
    with pytest.raises(ValueError, match="per-head q / k norm"):
        QuantLlama(arch.MODEL_CONFIGS["tiny-qwen3-test"], max_seq=32, device=DEV, engine=True)
