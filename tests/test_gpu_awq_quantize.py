"""ops.awq_clip / ops.awq_quantize -- AWQ's clip search on the matrix cores and its round-to-nearest as HIP kernels (csrc/amq_awq.hip, DESIGN.md
3.11) -- against the torch restatement of their arithmetic (tests/awq_search_ref.py): bounds, chosen steps, every step's error sum, codes, scale,
zero and the dense output BIT FOR BIT (every operation is a basic IEEE fp32 operation or an fmaf in a fixed order, so no tolerance is granted), on
the reference's fixtures (tests/golden/awqclip_*.npz) and on shapes beyond them; and through every layer above them up to a calibrated, packed HF
model that generates.  What the device gives is printed and written to profiles/awq_quantize.json ("parity")."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import awq_search_ref as ref
from quantize_common import assert_codes, assert_format_a, same_bits
from test_awq_quantize_cpu import CASES, IDS, fixture, restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "awq_quantize.json")
OBSERVED = {}
_SEEDED = {}


def seeded(N, K, group, bits, T):
    """(W, X fp16, a column scale, the restated clip search) of a shape beyond the fixtures, from a seeded generator; computed once"""
    key = (N, K, group, bits, T)
    if key not in _SEEDED:
        g = torch.Generator().manual_seed(N * 13 + K + group + bits + T)
        W = (torch.randn(N, K, generator=g) * 0.02).half()
        W[::5, ::11] *= 4.0
        X = torch.randn(T, K, generator=g)
        X[:, ::37] *= 10.0
        X = X.half()
        c = (0.25 + 3.0 * torch.rand(K, generator=g)).float()
        _SEEDED[key] = (W, X, c, ref.clip(W, X, bits, group, deploy=True))
    return _SEEDED[key]


def clip_identical(W, X, bits, group, want):
    """the device's clip search equals the restatement's, bit for bit; returns (hi, lo) on the device"""
    from amq_amd import ops
    N, K = W.shape
    hi, lo, info = ops.awq_clip(W.to(DEV), X.to(DEV), bits, group, return_info=True)
    assert info.nonfinite == 0 and tuple(info.err.shape) == (N, K // group, 10) and info.best.dtype == torch.int32
    err = info.err.cpu()
    assert same_bits(err, want["err"]), f"err: {int((err.view(torch.int32) != want['err'].view(torch.int32)).sum())} of {err.numel()} sums differ"
    assert torch.equal(info.best.cpu(), want["best"]), "best"
    assert same_bits(hi.cpu(), want["hi"]) and same_bits(lo.cpu(), want["lo"]), "bounds"
    return hi, lo


def quantize_identical(W, bits, group, hi, lo, col_scale=None):
    """the device's packed layer and dense output equal the restatement's, bit for bit"""
    from amq_amd import ops
    N, K = W.shape
    want = ref.quantize(W, bits, group, col_scale=col_scale, hi=None if hi is None else hi.cpu(), lo=None if lo is None else lo.cpu(), deploy=True)
    cs = None if col_scale is None else col_scale.to(DEV)
    h = ops.awq_quantize(W.to(DEV), bits, group, col_scale=cs, hi=hi, lo=lo)
    assert_format_a(h, bits, group, (N, K))
    assert_codes(h, want["q"])
    assert same_bits(h.scale.cpu(), want["scale"]) and same_bits(h.zero.cpu(), want["zero"]), "scale / zero"
    W_hat = ops.dequantize_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, N, K, group).cpu()
    assert torch.equal(W_hat.float(), want["W_hat"]), "the packed layer dequantizes to another weight than the search saw"
    dense = ops.awq_quantize(W.to(DEV), bits, group, col_scale=cs, hi=hi, lo=lo, dense=True)
    assert dense.dtype == torch.float16 and torch.equal(dense.cpu().float(), want["dense"]), "dense"


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_fixtures_bit_for_bit(name, bits):
    f = fixture(name)
    group = int(f["group"])
    hi, lo = clip_identical(f["W"], f["Xs"], bits, group, restated(name, bits, True))
    quantize_identical(f["W"], bits, group, hi, lo)
    quantize_identical(f["W"], bits, group, None, None, col_scale=torch.linspace(0.5, 2.0, f["W"].shape[1]))


# one tile of everything; N not a multiple of 32 and T padded; groups of 32; several workgroups and the real T; eleven groups per row, T = 67
BEYOND = [(16, 128, 128, 4, 16), (48, 256, 64, 3, 40), (80, 512, 32, 2, 130), (272, 384, 128, 3, 512), (64, 1408, 128, 4, 67)]


@pytest.mark.parametrize("N,K,group,bits,T", BEYOND)
def test_shapes_beyond_the_fixtures_bit_for_bit(N, K, group, bits, T):
    W, X, c, want = seeded(N, K, group, bits, T)
    hi, lo = clip_identical(W, X, bits, group, want)
    quantize_identical(W, bits, group, hi, lo)
    quantize_identical(W, bits, group, None, None, col_scale=c)


def test_run_to_run_and_the_conservative_twin_give_the_same_bits():
    from amq_amd import _lib, ops
    W, X, c, _ = seeded(272, 384, 128, 3, 512)
    Wd, Xd, cd = W.to(DEV), X.to(DEV), c.to(DEV)

    def both():
        hi, lo, info = ops.awq_clip(Wd, Xd, 3, 128, return_info=True)
        h = ops.awq_quantize(Wd, 3, 128, col_scale=cd, hi=hi, lo=lo)
        return hi, lo, info.best, info.err, h.W_q, h.scale, h.zero, ops.awq_quantize(Wd, 3, 128, col_scale=cd, dense=True)

    first, again = both(), both()
    with _lib.routed_to(_lib.open_twin()):
        twin = both()
    for other in (again, twin):
        assert all(torch.equal(a, b) for a, b in zip(first, other))


def test_both_entry_points_replay_from_a_captured_graph():
    from amq_amd import ops
    N, K, group, bits, T = 48, 256, 64, 3, 40
    W1, X1, c, _ = seeded(N, K, group, bits, T)
    W1, X1, c = W1.to(DEV), X1.to(DEV), c.to(DEV)
    W2, X2 = (W1.flip(0) * 1.5).half(), X1.flip(1).contiguous()
    eager = []
    for w, x in ((W1, X1), (W2, X2)):
        hi, lo, info = ops.awq_clip(w, x, bits, group, return_info=True)
        h = ops.awq_quantize(w, bits, group, col_scale=c, hi=hi, lo=lo)
        eager.append((hi.clone(), lo.clone(), info.best.clone(), info.err.clone(), h.W_q, h.scale, h.zero))
    Wbuf, Xbuf = W1.clone(), X1.clone()
    hi, lo, best, err, cinfo, _ = ops.awq_clip_buffers(N, K, T, bits, group, Wbuf.device)
    W_q, scale, zero, _, qinfo, _ = ops.awq_quantize_buffers(N, K, bits, group, Wbuf.device)
    cwork = torch.empty((ref.workspace_bytes(N, K, T, group) + 3) // 4, dtype=torch.int32, device=DEV)
    qwork = torch.empty((ref.quantize_workspace_bytes(N, K, group) + 3) // 4, dtype=torch.int32, device=DEV)

    def launch():
        ops.awq_clip_launch(Wbuf, Xbuf, bits, group, hi, lo, best, err, cinfo, cwork)
        ops.awq_quantize_launch(Wbuf, bits, group, c, hi, lo, W_q, scale, zero, None, qinfo, qwork)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for (w, x), want in (((W2, X2), eager[1]), ((W1, X1), eager[0])):
        Wbuf.copy_(w)
        Xbuf.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((hi, lo, best, err, W_q, scale, zero), want))
        assert int(cinfo.cpu()[0]) == 0 and int(qinfo.cpu()[0]) == 0


def test_wider_dtypes_are_cast_at_the_boundary():
    from amq_amd import ops
    W, X, _, _ = seeded(48, 256, 64, 3, 40)
    Xd = X.to(DEV)
    hi, lo = ops.awq_clip(W.to(DEV), Xd, 3, 64)
    hi32, lo32 = ops.awq_clip(W.to(DEV).float(), Xd.float(), 3, 64)            # W and X hold fp16 values, so the same result
    assert torch.equal(hi, hi32) and torch.equal(lo, lo32)
    base = ops.awq_quantize(W.to(DEV), 3, 64, hi=hi, lo=lo)
    wide = ops.awq_quantize(W.to(DEV).float(), 3, 64, hi=hi, lo=lo)
    assert torch.equal(wide.W_q, base.W_q) and torch.equal(wide.scale, base.scale) and torch.equal(wide.zero, base.zero)
    b16 = ops.awq_quantize(W.to(torch.bfloat16).to(DEV), 3, 64)
    same = ops.awq_quantize(W.to(torch.bfloat16).to(torch.float16).to(DEV), 3, 64)
    assert torch.equal(b16.W_q, same.W_q) and torch.equal(b16.scale, same.scale) and torch.equal(b16.zero, same.zero)


def test_refusals_in_order():
    """every refusal of the two entry points once, in the header's order; a refused call returns before any launch"""
    from amq_amd import _lib, ops
    N, K, group, bits, T = 48, 256, 64, 3, 40
    W, X, c, _ = seeded(N, K, group, bits, T)
    Wd, Xd, cd = W.to(DEV), X.to(DEV), c.to(DEV)
    hi, lo, best, err, info, work = ops.awq_clip_buffers(N, K, T, bits, group, Wd.device)
    W_q, scale, zero, _, qinfo, qwork = ops.awq_quantize_buffers(N, K, bits, group, Wd.device)
    odd = torch.empty(N * K + 8, dtype=torch.float16, device=DEV)[1:1 + N * K].view(N, K)        # 2-byte aligned only
    wide = torch.empty(N, 2 * K, dtype=torch.float16, device=DEV)

    def clip(match, W=Wd, X=Xd, bits=bits, group=group, hi=hi, work=work):
        with pytest.raises(_lib.AmqError, match=match):
            ops.awq_clip_launch(W, X, bits, group, hi, lo, best, err, info, work)

    clip("null", hi=None)
    clip("aligned", W=odd)
    clip("bits", bits=5)
    clip("groups of", group=96)
    clip("N %", W=Wd[:40])                                       # (N = 40; the buffers are larger than it needs)
    clip("K %", W=wide[:, :192].contiguous(), X=Xd[:, :192].contiguous())
    with pytest.raises(_lib.AmqError, match="T=0"):              # (the launch form takes T from X: the C entry point directly)
        _lib.check(_lib.load().amq_awq_clip_f16(_lib.ptr(Wd), _lib.ptr(Xd), N, K, 0, bits, group, _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(best),
                                                _lib.ptr(err), _lib.ptr(info), _lib.ptr(work), work.numel() * 4, _lib.current_stream()))
    clip("workspace too small", work=work[:1])

    def quant(match, W=Wd, bits=bits, group=group, hi=hi, lo=lo, W_q=W_q, dense=None, work=qwork):
        with pytest.raises(_lib.AmqError, match=match):
            ops.awq_quantize_launch(W, bits, group, cd, hi, lo, W_q, scale, zero, dense, qinfo, work)

    quant("null", lo=None)
    quant("null", W_q=None)                                      # scale and zero without W_q
    quant("aligned", W=odd)
    quant("bits", bits=1)
    quant("groups of", group=256)
    quant("N %", W=Wd[:40])
    quant("K %", W=wide[:, :192].contiguous())
    quant("workspace too small", work=qwork[:4])
    # the convenience forms refuse in Python what they can, and read the info block
    with pytest.raises(ValueError, match="32, 64 and 128"):
        ops.awq_clip(Wd, Xd, bits, 256)
    with pytest.raises(ValueError, match="bits"):
        ops.awq_quantize(Wd, 5, group)
    with pytest.raises(ValueError, match="GPU"):
        ops.awq_clip(W, X, bits, group)
    with pytest.raises(ValueError, match="together"):
        ops.awq_quantize(Wd, bits, group, hi=hi)
    with pytest.raises(ValueError, match="row"):
        ops.awq_clip(Wd, Xd[:0], bits, group)
    bad = Wd.clone()
    bad[17, 130] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        ops.awq_quantize(bad, bits, group, name="q_proj")
    with pytest.raises(ValueError, match="not finite"):
        ops.awq_clip(bad, Xd, bits, group)
    bad = Wd.clone()
    bad[3, 7] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        ops.awq_quantize(bad, bits, group, dense=True)


def _calibrated(n_kv_heads):
    from test_gpu_hf import _tiny_llama
    from amq_amd.arch import LINEARS
    from amq_amd.patching import quantize_model_awq
    from amq_amd.quant_linear import HIPQuantLinear
    dense = _tiny_llama(n_kv_heads)
    cycle = (4, 2, 3, 3, 2, 4, 3)
    bits = {name: [cycle[(i + b) % 7] for b in range(2)] for i, name in enumerate(LINEARS)}       # a mixed per-linear assignment
    g = torch.Generator().manual_seed(5)
    prompts = torch.randint(0, 1000, (8, 8), generator=g).to(DEV)
    with torch.no_grad():
        text = dense.generate(prompts, min_new_tokens=56, max_new_tokens=56, do_sample=False, num_beams=1)      # 8 windows of 64 tokens
    samples = [text[i:i + 1].cpu() for i in range(8)]
    ours, report = quantize_model_awq(copy.deepcopy(dense), {"linear": bits}, samples)
    assert len(report) == 14
    for b, layer in enumerate(ours.model.layers):
        for full in LINEARS:
            parent, attr = full.split(".")
            mod = getattr(getattr(layer, parent), attr)
            r = report[(b, full)]
            assert isinstance(mod, HIPQuantLinear) and mod.bits == bits[full][b] == r["bits"], (b, full)
            assert set(r) == {"bits", "ratio", "search_loss", "clip_steps", "loss", "rtn_loss"}
            assert r["loss"] == r["loss"] and r["rtn_loss"] == r["rtn_loss"]
            if attr in ("q_proj", "k_proj"):
                assert r["clip_steps"] is None
            else:
                assert len(r["clip_steps"]) == 10 and sum(r["clip_steps"]) == mod.outfeatures * mod.infeatures // 128
            if attr == "o_proj" and n_kv_heads == 1:
                assert r["ratio"] is None and r["search_loss"] is None            # v_proj is not o_proj's shape: auto_scale.py:185
            else:
                assert len(r["search_loss"]) == 20 and r["search_loss"][int(round(r["ratio"] * 20))] <= r["search_loss"][0]
    key = "tiny_llama_mha" if n_kv_heads == 2 else "tiny_llama_gqa"
    OBSERVED[key] = {f"{b}.{n}": {k: v[k] for k in ("bits", "ratio", "clip_steps", "loss", "rtn_loss")} for (b, n), v in report.items()}
    print(key, {f"{b}.{n}": round(v["loss"] / v["rtn_loss"], 3) for (b, n), v in report.items()})
    return dense, ours, bits, prompts, text


def test_quantize_model_awq_packs_and_generates():
    pytest.importorskip("transformers")
    from amq_amd import evaluate
    from amq_amd.arch import LINEARS
    from amq_amd.hqq_format import quantize_rtn
    from amq_amd.patching import HQQWeightsModule, prepare_for_inference, quantize_model_awq
    dense, ours, bits, prompts, text = _calibrated(2)
    assert isinstance(ours.lm_head, torch.nn.Linear)
    with pytest.raises(TypeError):
        quantize_model_awq(ours, 4, [text[:1].cpu()])                                              # already quantized
    with pytest.raises(ValueError):
        quantize_model_awq(copy.deepcopy(dense), 4, [text[0].cpu()])                               # not [1, seqlen]
    prepare_for_inference(ours, backend="hip")
    with torch.no_grad():
        out = ours.generate(prompts[:2], min_new_tokens=6, max_new_tokens=6, do_sample=False, num_beams=1)
    assert out.shape == (2, 14)
    rtn = copy.deepcopy(dense)
    for b, layer in enumerate(rtn.model.layers):
        for full in LINEARS:
            parent, attr = full.split(".")
            lin = getattr(getattr(layer, parent), attr)
            setattr(getattr(layer, parent), attr, HQQWeightsModule(quantize_rtn(lin.weight.detach(), bits[full][b], 128)))
    prepare_for_inference(rtn, backend="hip")
    windows = [text[:4].cpu(), text[4:].cpu()]
    ppl_dense = float(np.exp(np.mean([torch.nn.functional.cross_entropy(dense(w.to(DEV)).logits[:, :-1].float().reshape(-1, 1000),
                                                                        w[:, 1:].reshape(-1).to(DEV)).item() for w in windows])))
    # recorded, not asserted: on a random tiny model the ordering is not guaranteed (eval_ppl: per-token perplexity to the 4th power, B = 4)
    OBSERVED["tiny_llama_ppl"] = {"dense": ppl_dense, "awq_quantize": evaluate.eval_ppl(ours, None, windows, seqlen=64),
                                  "quantize_rtn": evaluate.eval_ppl(rtn, None, windows, seqlen=64)}
    print("perplexity:", OBSERVED["tiny_llama_ppl"])


def test_quantize_model_awq_under_gqa_skips_the_v_to_o_search():
    pytest.importorskip("transformers")
    from amq_amd.patching import prepare_for_inference
    _, ours, _, prompts, _ = _calibrated(1)
    prepare_for_inference(ours, backend="hip")
    with torch.no_grad():
        out = ours.generate(prompts[:2], min_new_tokens=6, max_new_tokens=6, do_sample=False, num_beams=1)
    assert out.shape == (2, 14)


def _block_with_inputs(n_kv_heads):
    """a tiny model with hot channels planted in block 0's input norm, that block's inputs [4, 64, 256] and keyword arguments, and the inputs of
    its linears"""
    from test_gpu_hf import _tiny_llama
    model = _tiny_llama(n_kv_heads)
    layer = model.model.layers[0]
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        layer.input_layernorm.weight[torch.randperm(256, generator=g)[:6]] *= 12.0
    xs, kwargs = [], {}

    def catch(m, a, kw):
        xs.append((a[0] if a else kw["hidden_states"]).detach())
        kwargs.update({k: v for k, v in kw.items() if k != "hidden_states"})

    handle = layer.register_forward_pre_hook(catch, with_kwargs=True)
    feats = {}
    at = {"self_attn.q_proj": layer.self_attn.q_proj, "self_attn.o_proj": layer.self_attn.o_proj, "mlp.gate_proj": layer.mlp.gate_proj,
          "mlp.down_proj": layer.mlp.down_proj}
    hs = [m.register_forward_hook(lambda m, i, o, n=n: feats.setdefault(n, []).append(i[0].detach().clone())) for n, m in at.items()]
    with torch.no_grad():
        for window in torch.randint(0, 1000, (4, 1, 64), generator=g):          # one window per pass: the keyword arguments are a window's
            model(window.to(DEV), use_cache=False)
    handle.remove()
    for h in hs:
        h.remove()
    return layer, xs, kwargs, {n: torch.cat(v, dim=0) for n, v in feats.items()}


@pytest.mark.parametrize("n_kv_heads", [2, 1], ids=["mha", "gqa"])
def test_the_searched_scales_fold_away(n_kv_heads):
    """applying the searched scales WITHOUT quantizing leaves the block's output within fp16 rounding of the original: max abs difference <= 2e-3 of
    the output's max abs (fp16's 2^-10 step with headroom).  Under GQA there are three searches and o_proj's input is untouched."""
    pytest.importorskip("transformers")
    from amq_amd.patching import _awq_apply_scale, _awq_searches
    layer, xs, kw, feats = _block_with_inputs(n_kv_heads)

    def run(block):
        outs = [block(x, **kw) for x in xs]
        return torch.cat([(o[0] if isinstance(o, (tuple, list)) else o).float() for o in outs])

    with torch.no_grad():
        want = run(layer)
        scaled = copy.deepcopy(layer)
        attn_kw = {k: v for k, v in kw.items() if k != "use_cache"}
        found = _awq_searches(scaled, feats, attn_kw, {"linear": {n: [3] for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj",
                                                                                   "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                                                                                   "mlp.down_proj")}}, 0, 128)
        assert len(found) == (4 if n_kv_heads == 2 else 3)
        assert any(float(s.max() / s.min()) > 1.5 for _, _, _, s, _, _ in found), "no search moved off ratio 0: nothing to fold"
        o_in = feats["self_attn.o_proj"].clone()
        _awq_apply_scale(scaled, found, feats)
        assert torch.equal(feats["self_attn.o_proj"], o_in) == (n_kv_heads == 1)
        got = run(scaled)
    worst = float((got - want).abs().max() / want.abs().max())
    OBSERVED[f"scale_fold_{'mha' if n_kv_heads == 2 else 'gqa'}"] = worst
    print(f"folded scales: max abs difference / max abs output {worst:.3g}")
    assert worst <= 2e-3


def test_zz_observed_parity_is_recorded():
    """last in the file: what the device gave in the tests above goes to profiles/awq_quantize.json under "parity" (the timings of
    tools/awq_bench.py live beside it)"""
    if not OBSERVED:                        # (run alone: nothing to record)
        return
    try:
        doc = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        doc["parity"] = {"device": torch.cuda.get_device_name(0), "cases": OBSERVED}
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError as e:                    # a read-only checkout: the assertions above are what counts
        print("not recorded:", e)
