"""Sampled decoding and EOS stop on the GPU: the kernel (amq_sample_f16) against the fp64 restatement of its rules (tests/sampling_ref.py), the
runner's sampled graph beside its greedy one, and the opt-in HF surface (convert_model_to_hip(model, sampling=True))."""
import numpy as np
import pytest
import torch

import sampling_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAND = 1e-4     # fp32-sum bound of the issue ((256 + 18) * 2^-24 = 1.6e-5 of the mass, x 6); the kernel's fixed-point sums sit far inside it


def _state(temperature=1.0, top_k=0, top_p=1.0, seed=0, **kw):
    from amq_amd import ops
    return ops.set_sampling_state(ops.new_sampling_state(torch.device(DEV)), temperature, top_k, top_p, seed, **kw)


def _rows(vocab, scale, rows, seed):
    return np.stack([ref.logits_row(vocab, scale, seed + r) for r in range(rows)])


@pytest.mark.parametrize("vocab", ref.VOCABS)
def test_kept_set(vocab):
    """the kept mask: exact for top-k alone (integer work on fp16 keys); with top-p every token whose mass of strictly larger logits is below
    top_p - BAND is kept, every one above top_p + BAND dropped, and tie classes are kept or dropped whole"""
    from amq_amd import ops
    for si, scale in enumerate(ref.SCALES):
        for rows in (1, 3, 8):
            lg = _rows(vocab, scale, rows, seed=7 * vocab + 100 * si + rows)
            suppress = (int(lg[0].argmax()), 5, vocab - 1) if rows == 3 else ()        # (the largest logit of row 0 among them)
            sup = torch.tensor(list(suppress) + [-1] * (8 - len(suppress)), dtype=torch.int32, device=DEV) if suppress else None
            dl = torch.from_numpy(lg).to(DEV)
            for temperature, top_k, top_p in ref.GRID:
                kept = torch.zeros(rows, vocab, dtype=torch.uint8, device=DEV)
                tok = ops.sample(dl, _state(temperature, top_k, top_p, seed=3), kept_out=kept, suppress=sup)
                kept, tok = kept.cpu().numpy().astype(bool), tok.cpu().numpy()
                for r in range(rows):
                    want, want_k, d = ref.kept_set(lg[r], temperature, top_k, top_p, suppress)
                    case = (vocab, scale, rows, r, temperature, top_k, top_p)
                    assert kept[r, tok[r]], case
                    assert not kept[r, list(suppress)].any(), case
                    if top_p >= 1.0:
                        assert np.array_equal(kept[r], want), case
                        continue
                    assert not (kept[r] & ~want_k).any(), case                          # nothing top-k dropped comes back
                    assert kept[r][want_k & (d < top_p - BAND)].all(), case
                    assert not kept[r][want_k & (d > top_p + BAND)].any(), case
                    vals = lg[r].astype(np.float32)
                    cand = want_k
                    lo_kept = vals[kept[r]].min()
                    assert np.array_equal(kept[r][cand], vals[cand] >= lo_kept), case       # a threshold on the logit: whole tie classes


@pytest.mark.parametrize("vocab", ref.VOCABS)
def test_draw_with_given_u(vocab):
    """u supplied: the token's fp64 cumulative interval (ascending token index, over the kernel's own mask) contains u within BAND"""
    from amq_amd import ops
    n = 1024
    g = np.random.default_rng(vocab)
    u = g.random(n).astype(np.float32)
    u[0], u[1], u[2] = 0.0, 1.0 - 2.0 ** -24, 0.5
    du = torch.from_numpy(u).to(DEV)
    for si, scale in enumerate(ref.SCALES):
        lg = ref.logits_row(vocab, scale, seed=31 * vocab + si)
        one = torch.from_numpy(lg).to(DEV)
        many = one[None].expand(n, vocab).contiguous()
        for temperature, top_k, top_p in ref.GRID:
            st = _state(temperature, top_k, top_p)
            kept = torch.zeros(1, vocab, dtype=torch.uint8, device=DEV)
            ops.sample(one, st, kept_out=kept)
            tok = ops.sample(many, st, u=du).cpu().numpy()
            kept = kept.cpu().numpy()[0].astype(bool)
            c, p = ref.cdf(lg, temperature, kept)
            case = (vocab, scale, temperature, top_k, top_p)
            assert kept[tok].all(), case
            hi, lo = c[tok], c[tok] - p[tok]
            bad = ~((lo - BAND <= u) & (u < hi + BAND))
            assert not bad.any(), (case, tok[bad][:4], u[bad][:4], lo[bad][:4], hi[bad][:4])
            # u = 0: the first kept token the kernel can draw at all (a weight below 2^-40 of the largest rounds to zero in its fixed point)
            rel = np.where(kept, p / p.max(), 0.0)
            assert np.flatnonzero(rel >= 2.0 ** -41)[0] <= tok[0] <= np.flatnonzero(rel >= 2.0 ** -39)[0], case


def test_distribution_and_streams():
    """generated u: 200,000 draws (2000 sequences x 100 draw counters, the kernel advancing the counter itself) of one 1000-token row, top_k = 50"""
    from amq_amd import ops
    vocab, rows, draws = 1000, 2000, 100
    lg = ref.logits_row(vocab, 3.0, seed=99)
    many = torch.from_numpy(lg).to(DEV)[None].expand(rows, vocab).contiguous()
    want, _, _ = ref.kept_set(lg, 0.9, 50, 1.0)
    _, p = ref.cdf(lg, 0.9, want)

    def stream(seed):
        st = _state(0.9, 50, 1.0, seed=seed)
        out = torch.stack([ops.sample(many, st, flags=ops.SAMPLE_ADVANCE).clone() for _ in range(draws)])
        assert int(st[6].item()) == draws                                               # the draw counter moved once per launch
        return out.cpu().numpy()

    a, a2, b = stream(1234), stream(1234), stream(1235)
    assert np.array_equal(a, a2) and not np.array_equal(a, b)
    n = a.size
    freq = np.bincount(a.reshape(-1), minlength=vocab) / n
    assert not freq[~want].any()
    kept = np.flatnonzero(want)
    print("max |freq - p| / sigma:", float((np.abs(freq - p)[kept] / np.sqrt(p[kept] * (1 - p[kept]) / n)).max()))
    assert np.all(np.abs(freq - p)[kept] <= 5.0 * np.sqrt(p[kept] * (1 - p[kept]) / n) + 1.0 / n)
    # the generator is the documented function of (seed, draw counter, sequence index): spot-check draws whose u is clear of an interval end
    c, _ = ref.cdf(lg, 0.9, want)
    for d, s in ((0, 0), (0, 1), (1, 0), (7, 1999), (99, 5)):
        u = ref.uniform(1234, d, s)
        t = ref.draw(lg, 0.9, want, u)
        if min(abs(u - c[t]), abs(u - (c[t] - p[t]))) > BAND:
            assert a[d, s] == t, (d, s, u)


# ------------------------------------------------------------------ runner
NAMES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _tiny_prepared(layers=2):
    """the tiny Llama of tests/test_gpu_hf_fast.py (head_dim 128, vocab 1000) with HQQ stand-ins for its linears, prepared for the HIP backend"""
    transformers = pytest.importorskip("transformers")
    from amq_amd.hqq_format import random_hqq
    from amq_amd.patching import HQQWeightsModule, prepare_for_inference
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=layers, num_attention_heads=2, num_key_value_heads=1,
                                   vocab_size=1000, max_position_embeddings=256, rms_norm_eps=1e-5, attn_implementation="eager")
    model = transformers.LlamaForCausalLM(cfg).to(torch.float16).to(DEV).eval()
    i = 0
    for layer in model.model.layers:
        for parent in (layer.self_attn, layer.mlp):
            for name in NAMES:
                lin = getattr(parent, name, None)
                if lin is None:
                    continue
                n, k = lin.weight.shape
                h = random_hqq(n, k, (4, 2, 3, 3, 2, 4, 3)[i % 7], seed=100 + i)
                i += 1
                h.bias = None
                setattr(parent, name, HQQWeightsModule(h.to(torch.device(DEV))))
    prepare_for_inference(model, backend="hip")
    return model


def _ids(B, S=12, seed=5):
    return torch.randint(3, 1000, (B, S), generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("B", (1, 3))
def test_runner_seeded_graph_and_eager(B):
    from amq_amd.llama import QuantLlama
    model = _tiny_prepared()
    r = QuantLlama.from_hf(model, max_seq=128, batch=B)
    ids = _ids(B) if B > 1 else _ids(1)[0]
    n = 24
    greedy = r.generate(ids, n).clone()
    g0 = r.graph
    assert g0 is not None and r.sample_graph is None
    r.set_sampling(temperature=1.0, top_k=0, top_p=0.95, seed=11)
    a = r.generate(ids, n).clone()
    gs = r.sample_graph
    assert gs is not None and r.graph is g0
    assert torch.equal(a, r.generate(ids, n))                                           # run vs re-run
    assert torch.equal(a, r.generate(ids, n, use_graph=False))                          # graph vs eager
    r.set_sampling(temperature=1.0, top_k=0, top_p=0.95, seed=12)
    assert not torch.equal(a, r.generate(ids, n))
    assert not torch.equal(a, greedy)
    # parameters changed between replays take effect, in the same graph: top_k = 1 -> every token's logit is its step's maximum
    r.set_sampling(temperature=0.7, top_k=1, top_p=1.0, seed=12)
    for use_graph in (True, False):
        r.prefill(ids)
        for _ in range(n):
            lg = r.logits.view(B, -1).float()
            assert torch.equal(lg.gather(1, r.token.view(B, 1))[:, 0], lg.max(dim=1).values)
            r.decode_step(use_graph)
    assert r.sample_graph is gs and r.graph is g0
    # back to greedy: the tokens of a fresh greedy runner, the graph captured before sampling was ever on
    r.set_sampling(None)
    assert torch.equal(r.generate(ids, n), greedy) and r.graph is g0
    fresh = QuantLlama.from_hf(model, max_seq=128, batch=B)
    assert torch.equal(fresh.generate(ids, n), greedy)


def test_runner_eos_stop():
    from amq_amd.llama import QuantLlama
    model = _tiny_prepared()
    n = 40
    r = QuantLlama.from_hf(model, max_seq=128, batch=1)
    ids = _ids(1)[0]
    r.set_sampling(temperature=1.0, top_k=0, top_p=1.0, seed=21)
    full = r.generate(ids, n).clone().tolist()
    j = next(j for j in range(3, n) if full[j] not in full[:j])
    r.set_eos((full[j],), pad_id=0)
    assert r.generate(ids, n).tolist() == full                                          # without stop_at_eos: today's fixed length
    cut = r.generate(ids, n, stop_at_eos=True)
    assert cut.tolist() == full[:j + 1]
    assert r.unfinished() == 0

    r2 = QuantLlama.from_hf(model, max_seq=128, batch=2)
    ids2 = _ids(2)
    r2.set_sampling(temperature=1.0, top_k=0, top_p=1.0, seed=22)
    full2 = r2.generate(ids2, n).clone()
    row0, row1 = full2[0].tolist(), full2[1].tolist()
    j = next(j for j in range(3, n - 2) if row0[j] not in row0[:j] and row0[j] not in row1)
    r2.set_eos((row0[j],), pad_id=7)
    cut2 = r2.generate(ids2, n, stop_at_eos=True)
    assert cut2.shape == (2, n)
    assert cut2[0].tolist() == row0[:j + 1] + [7] * (n - j - 1)
    assert cut2[1].tolist() == row1
    assert r2.unfinished() == 1
    # greedy with EOS stop: the greedy tokens up to and including the first EOS
    r.set_sampling(None)
    r.set_eos((), 0)
    g = r.generate(ids, n).tolist()
    j = next(j for j in range(2, n) if g[j] not in g[:j])
    r.set_eos((g[j],), pad_id=0)
    assert r.generate(ids, n, stop_at_eos=True).tolist() == g[:j + 1]
    assert r.generate(ids, n, stop_at_eos=True, min_new_tokens=j + 2).tolist()[:j] == g[:j]


# ------------------------------------------------------------------ HF surface
def test_hf_surface_sampling_opt_in():
    from amq_amd import hf_fast
    model = _tiny_prepared()
    ids = _ids(2, S=10, seed=9)
    mask = torch.ones_like(ids)
    hf_fast.convert_model_to_hip(model)                                                 # default: both calls are HF's
    torch.manual_seed(0)
    model.generate(ids, do_sample=True, top_k=5, max_new_tokens=6, attention_mask=mask, pad_token_id=0)
    model.generate(ids, do_sample=False, max_new_tokens=6, attention_mask=mask, pad_token_id=0, eos_token_id=2)
    assert model not in hf_fast._RUNNERS
    hf_fast.convert_model_to_hip(model, sampling=True)
    torch.manual_seed(0)
    a = model.generate(ids, do_sample=True, top_k=5, max_new_tokens=20, attention_mask=mask, pad_token_id=0)
    assert model in hf_fast._RUNNERS and a.shape == (2, 30) and torch.equal(a[:, :10], ids)
    torch.manual_seed(0)
    assert torch.equal(a, model.generate(ids, do_sample=True, top_k=5, max_new_tokens=20, attention_mask=mask, pad_token_id=0))
    torch.manual_seed(1)
    assert not torch.equal(a, model.generate(ids, do_sample=True, top_k=5, max_new_tokens=20, attention_mask=mask, pad_token_id=0))
    # every new token is within HF's own top 5 for its prefix (HF's forward over the same modules, teacher-forced), near-ties allowed
    with torch.inference_mode():
        lg = model(a).logits.float()                                                    # (no start_pos: HF's own forward)
    for b in range(2):
        for t in range(10, 30):
            row = lg[b, t - 1]
            fifth = torch.topk(row, 5).values[-1]
            assert float(row[a[b, t]]) >= float(fifth) - 4e-3 * float(row.abs().max()), (b, t)

    # open-ended greedy: HF's own result on the unconverted model, up to the first near-tie, including where it stops
    hf_fast.revert_model_to_hf(model)
    base = model.generate(ids[:1], do_sample=False, max_new_tokens=12, attention_mask=mask[:1], pad_token_id=0)
    e = int(base[0, 10 + 5])                                                            # a token HF emits at step 5 (or earlier) becomes the EOS id
    slow = model.generate(ids[:1], do_sample=False, max_new_tokens=12, attention_mask=mask[:1], pad_token_id=0, eos_token_id=e)
    hf_fast.convert_model_to_hip(model, sampling=True)
    fast = model.generate(ids[:1], do_sample=False, max_new_tokens=12, attention_mask=mask[:1], pad_token_id=0, eos_token_id=e)
    if fast.shape == slow.shape and torch.equal(fast, slow):
        return
    m = min(fast.shape[1], slow.shape[1])
    diff = (fast[0, :m] != slow[0, :m]).nonzero()
    assert len(diff) > 0, (fast.tolist(), slow.tolist())                                # same tokens: same length
    t = int(diff[0])
    with torch.inference_mode():
        row = model(slow[:, :t]).logits[0, -1].float()
    assert float(row.max() - row[int(fast[0, t])]) <= 4e-3 * float(row.abs().max()), (t, fast.tolist(), slow.tolist())
