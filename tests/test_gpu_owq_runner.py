"""OWQ models in the decode runner and in scoring (DESIGN.md 3.12 "In the runner").

1. The stage kernel (csrc/amq_owq_step.hip, ops.owq_stage) is held BIT FOR BIT to the composition of the entry points it stands in front of:
   ops.rmsnorm / ops.silu_mul, ops.owq_gather, ops.owq_outlier_add -- rows, activations, residual forms, parts, guard bands, non-finite inputs,
   determinism, graph replay, and the refusals in their documented order.
2. The runner over a calibrated tiny Llama (QuantLlama.from_hf over HIPOWQLinear modules): against an fp64 forward over the dequantized weights
   with HF's forward over the modules as the yardstick, graph replay, batches, ragged batches, prompt lookup, the HF surface, the two metrics.
What the device gives is printed and written to profiles/owq_decode.json ("parity"; the timings of tools/owq_decode_bench.py live beside it)."""
import copy
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import evalmetrics_ref as mref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "owq_decode.json")
OBSERVED = {}
GUARD = 64              # poisoned fp16 elements on either side of every output
POISON = 0x7BFF         # (65504: a value no result here takes)


def bits_of(t):
    return t.contiguous().view(torch.int16)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits_of(a), bits_of(b))


# ------------------------------------------------------------------------------------------------------------------ 1. the stage kernel
def owq_part(K, n_out, N, seed):
    """a layer's deployment side with random contents: perm [Kp] (a random choice of K - n_out columns in random order, -1 padding), out_ids
    ascending, W_out [N, n_out]; n_out == 0: a plain sibling"""
    from amq_amd import ops
    if n_out == 0:
        return dict(K=K, n_out=0, N=N)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randperm(K, generator=g)
    Kp = ops.owq_packed_columns(K, n_out)
    perm = torch.full((Kp,), -1, dtype=torch.int32)
    perm[:K - n_out] = ids[:K - n_out].to(torch.int32)
    out_ids = torch.sort(ids[K - n_out:])[0].to(torch.int32)
    W_out = (torch.randn(N, n_out, generator=g) * 0.05).half()
    return dict(K=K, n_out=n_out, N=N, Kp=Kp, perm=perm.to(DEV), out_ids=out_ids.to(DEV), W_out=W_out.to(DEV))


# (K, [(n_out, N)]): the issue's layers -- (256, 4) with 4 padding columns, (384, 130) with 2, (512, 2), a plain part -- as 1, 2 and 3 parts of
# different N and n_out in one launch; N = 16 / 80 / 272 are no multiples of the 256 outputs a workgroup owns; n_out = 130 / 66 cross the tile of 64
CASES = {
    "k256_one": (256, [(4, 16)]),
    "k384_two": (384, [(130, 80), (4, 272)]),
    "k512_three": (512, [(2, 272), (66, 16), (0, 0)]),
    "k256_three": (256, [(4, 80), (0, 0), (130, 272)]),
}
ACTS = ("none", "rmsnorm", "silu_mul")


def guarded(n):
    """n fp16 elements between two poisoned bands -> (the whole buffer, the view)"""
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.int16, device=DEV).view(torch.float16)
    return buf, buf[GUARD:GUARD + n]


def bands_intact(buf, n):
    raw = buf.view(torch.int16)
    return bool((raw[:GUARD] == POISON).all()) and bool((raw[GUARD + n:] == POISON).all())


def inputs(R, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(R, K, generator=g) * 1.5).half().to(DEV)
    x2 = torch.randn(R, K, generator=g).half().to(DEV)
    gamma = (1.0 + 0.1 * torch.randn(K, generator=g)).half().to(DEV)
    return x, x2, gamma


def activation(act, x, x2, gamma, eps):
    from amq_amd import ops
    if act == "rmsnorm":
        return ops.rmsnorm(x, gamma, eps)
    if act == "silu_mul":
        return ops.silu_mul(x, x2)
    return x


def stage(act, x, x2, gamma, eps, parts):
    from amq_amd import ops
    code = {"none": ops.OWQ_ACT_NONE, "rmsnorm": ops.OWQ_ACT_RMSNORM, "silu_mul": ops.OWQ_ACT_SILU_MUL}[act]
    ops.owq_stage(x, parts, act=code, gamma=gamma, eps=eps, x2=x2)


def run_case(layers, R, act, residual, seed, x=None):
    """one stage launch into guarded outputs and the composition of the existing ops -> [(xg, xg_want, y, y_want)] per part (y None: plain)"""
    from amq_amd import ops
    K = layers[0]["K"]
    x0, x2, gamma = inputs(R, K, seed)
    x = x0 if x is None else x
    eps = 1e-5
    a = activation(act, x, x2, gamma, eps)
    g = torch.Generator().manual_seed(seed + 1)
    parts, held = [], []
    for l in layers:
        if l["n_out"] == 0:
            xb, xg = guarded(R * K)
            parts.append(dict(xg=xg.view(R, K)))
            held.append((l, xb, xg.view(R, K), None, None, None))
            continue
        xb, xg = guarded(R * l["Kp"])
        yb, y = guarded(R * l["N"])
        y = y.view(R, l["N"])
        res0 = torch.randn(R, l["N"], generator=g).half().to(DEV)
        if residual == "alias":
            y.copy_(res0)
            res = y
        else:
            res = res0.clone() if residual == "separate" else None
        parts.append(dict(perm=l["perm"], out_ids=l["out_ids"], W_out=l["W_out"], xg=xg.view(R, l["Kp"]), y=y, residual=res))
        held.append((l, xb, xg.view(R, l["Kp"]), yb, y, res0))
    stage(act, x, x2, gamma, eps, parts)
    torch.cuda.synchronize()
    out = []
    for l, xb, xg, yb, y, res0 in held:
        assert bands_intact(xb, xg.numel()), "xg's guard bands were written"
        if l["n_out"] == 0:
            out.append((xg, a, None, None))
            continue
        assert bands_intact(yb, y.numel()), "y's guard bands were written"
        want = torch.zeros_like(y) if residual == "none" else res0.clone()
        ops.owq_outlier_add(a, l["out_ids"], l["W_out"], want)
        out.append((xg, ops.owq_gather(a, l["perm"]), y, want))
    return out


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_stage_is_the_composition_of_the_existing_ops_bit_for_bit(case, act):
    K, spec = CASES[case]
    layers = [owq_part(K, n_out, N, seed=17 * i + K) for i, (n_out, N) in enumerate(spec)]
    for R in (1, 2, 5, 8):
        for residual in ("none", "separate", "alias"):
            for i, (xg, xg_want, y, y_want) in enumerate(run_case(layers, R, act, residual, seed=R)):
                assert same(xg, xg_want), (case, act, R, residual, i, "xg")
                if y is not None:
                    assert same(y, y_want), (case, act, R, residual, i, "y", float((y.float() - y_want.float()).abs().max()))
                    assert bool(torch.isfinite(y).all())
    # the padding columns are 0 and a workgroup's tail outputs were formed (not left as poison)
    l = layers[0]
    if l["n_out"]:
        xg = run_case(layers, 2, act, "none", seed=3)[0][0]
        assert bool((xg[:, l["perm"] < 0] == 0).all())


@pytest.mark.parametrize("act", ["none", "silu_mul"])
def test_stage_non_finite_inputs(act):
    """an inf in a column of x that no packed column reads (an outlier column: only the padding stands where it would have been) leaves xg finite,
    and it propagates through the outlier product exactly as the existing op's does"""
    K = 384
    l = owq_part(K, 130, 80, seed=5)
    x, _, _ = inputs(5, K, seed=9)
    x = x.clone()
    col = int(l["out_ids"][7])
    x[1, col] = float("inf")
    x[3, col] = float("-inf")
    (xg, xg_want, y, y_want), = run_case([l], 5, act, "separate", seed=9, x=x)
    assert bool(torch.isfinite(xg).all()) and same(xg, xg_want) and bool((xg[:, l["perm"] < 0] == 0).all())
    assert same(y, y_want)
    assert not bool(torch.isfinite(y[1]).all()) and not bool(torch.isfinite(y[3]).all()) and bool(torch.isfinite(y[[0, 2, 4]]).all())


def test_stage_is_deterministic_and_replays_from_a_graph():
    from amq_amd import ops
    from amq_amd.llama import capture_graph, _prime_graph_state
    K, R, eps = 512, 5, 1e-5
    layers = [owq_part(K, 66, 272, seed=1), owq_part(K, 2, 80, seed=2), owq_part(K, 0, 0, seed=3)]
    x, x2, gamma = inputs(R, K, seed=4)
    res = torch.randn(R, 272, generator=torch.Generator().manual_seed(6)).half().to(DEV)

    def buffers():
        return [dict(perm=l["perm"], out_ids=l["out_ids"], W_out=l["W_out"], xg=torch.zeros(R, l["Kp"], dtype=torch.float16, device=DEV),
                     y=torch.zeros(R, l["N"], dtype=torch.float16, device=DEV), residual=res if l["N"] == 272 else None) if l["n_out"]
                else dict(xg=torch.zeros(R, K, dtype=torch.float16, device=DEV)) for l in layers]

    def outputs(parts):
        return [t.clone() for p in parts for t in ([p["xg"], p["y"]] if "y" in p else [p["xg"]])]

    for act in ACTS:
        first = buffers()
        stage(act, x, x2, gamma, eps, first)
        want = outputs(first)
        again = buffers()
        stage(act, x, x2, gamma, eps, again)
        assert all(same(a, b) for a, b in zip(outputs(again), want)), act
        dev = torch.device(DEV)
        _prime_graph_state(dev)
        held = buffers()
        graph = capture_graph(dev, lambda: stage(act, x, x2, gamma, eps, held))
        for p in held:
            for k in ("xg", "y"):
                if k in p:
                    p[k].fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(same(a, b) for a, b in zip(outputs(held), want)), act
        # other rows through the same graph: the launch reads x where it lies
        x.copy_(inputs(R, K, seed=8)[0])
        fresh = buffers()
        stage(act, x, x2, gamma, eps, fresh)
        graph.replay()
        torch.cuda.synchronize()
        assert all(same(a, b) for a, b in zip(outputs(held), outputs(fresh))), act
        x.copy_(inputs(R, K, seed=4)[0])
    assert ops.OWQ_STAGE_ROWS == 8


def test_stage_refusals_in_their_documented_order():
    """include/amq_hip.h amq_owq_stage_f16: null / misaligned activations, unknown act, n_parts, R, K, then part by part null pointers, alignment,
    n_out, Kp, N -- validation only, nothing is launched (the pointers are never dereferenced)"""
    from amq_amd import _lib, ops
    lib = _lib.load()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)

    def part(**kw):
        f = dict(perm=one, out_ids=one, W_out=one, xg=one, y=one, residual=None, N=16, n_out=2, Kp=128)
        f.update(kw)
        return _lib.OwqPart(f["perm"], f["out_ids"], f["W_out"], f["xg"], f["y"], f["residual"], f["N"], f["n_out"], f["Kp"])

    def call(x=one, R=1, K=256, act=0, gamma=None, x2=None, parts=(part(),), n_parts=None):
        arr = (_lib.OwqPart * max(1, len(parts)))(*parts)
        rc = lib.amq_owq_stage_f16(x, R, K, act, gamma, ctypes.c_float(1e-5), x2, arr if parts is not None else None,
                                   len(parts) if n_parts is None else n_parts, None)
        return rc, lib.amq_last_error().decode()

    EINVAL, ESHAPE = -1, -2
    bad_part = part(xg=None, n_out=3)
    # each call breaks the rule under test AND every later one: the earlier rule must answer
    rc, msg = call(x=None, act=9, n_parts=4, R=9, K=100, parts=(bad_part,))
    assert rc == EINVAL and "null" in msg
    for kw in (dict(act=1), dict(act=2)):                         # gamma / x2 missing for their activation
        rc, msg = call(R=9, **kw)
        assert rc == EINVAL and "null" in msg
    rc, msg = call(x=odd, act=9, n_parts=4, R=9, K=100, parts=(bad_part,))
    assert rc == EINVAL and "16-byte" in msg
    rc, msg = call(act=9, n_parts=4, R=9, K=100, parts=(bad_part,))
    assert rc == EINVAL and "activation" in msg
    for n in (0, 4):
        rc, msg = call(n_parts=n, R=9, K=100, parts=(bad_part,))
        assert rc == ESHAPE and "n_parts" in msg
    for R in (0, 9):
        rc, msg = call(R=R, K=100, parts=(bad_part,))
        assert rc == ESHAPE and "R must" in msg
    for K in (0, 100, 192):
        rc, msg = call(K=K, parts=(bad_part,))
        assert rc == ESHAPE and "K %" in msg
    for kw in (dict(xg=None), dict(perm=None), dict(out_ids=None), dict(W_out=None), dict(y=None)):
        rc, msg = call(parts=(part(), part(n_out=3, Kp=100, N=0, **kw)))
        assert rc == EINVAL and "part 1: null" in msg, (kw, msg)
    rc, msg = call(parts=(part(xg=odd, n_out=3, Kp=100, N=0),))
    assert rc == EINVAL and "aligned" in msg
    for n_out in (3, -2, 256):
        rc, msg = call(parts=(part(n_out=n_out, Kp=100, N=0),))
        assert rc == ESHAPE and "n_out" in msg
    for Kp in (100, 0):
        rc, msg = call(parts=(part(Kp=Kp, N=0),))
        assert rc == ESHAPE and "Kp" in msg
    rc, msg = call(parts=(part(N=0),))
    assert rc == ESHAPE and "N > 0" in msg
    # a plain part needs its xg alone
    rc, msg = call(parts=(part(perm=None, out_ids=None, W_out=None, y=None, n_out=0, N=0, Kp=0),), R=9)
    assert rc == ESHAPE and "R must" in msg
    # the wrapper refuses shapes that do not belong together before the library sees them
    x = torch.zeros(2, 256, dtype=torch.float16, device=DEV)
    l = owq_part(256, 4, 16, seed=1)
    good = dict(perm=l["perm"], out_ids=l["out_ids"], W_out=l["W_out"], xg=torch.zeros(2, 256, dtype=torch.float16, device=DEV),
                y=torch.zeros(2, 16, dtype=torch.float16, device=DEV))
    for bad in (dict(good, xg=good["xg"][:1]), dict(good, y=good["y"][:1]), dict(good, out_ids=l["out_ids"][:2]),
                dict(good, residual=good["y"][:1])):
        with pytest.raises(ValueError):
            ops.owq_stage(x, [bad])
    with pytest.raises(ValueError):
        ops.owq_stage(x, [good] * 4)
    with pytest.raises(ValueError):
        ops.owq_stage(torch.zeros(9, 256, dtype=torch.float16, device=DEV), [good])


# ------------------------------------------------------------------------------------------------------------------ 2. the runner
PROMPT, STEPS = 17, 8


@functools.lru_cache(maxsize=None)
def owq_model(n_kv):
    """(dense tiny Llama, its OWQ-quantized twin, the 8 calibration windows of 64 tokens the dense model generated) -- once per module"""
    pytest.importorskip("transformers")
    from test_gpu_hf import _tiny_llama
    from amq_amd.arch import LINEARS
    from amq_amd.patching import quantize_model_owq
    dense = _tiny_llama(n_kv)
    cycle = (4, 2, 3, 3, 2, 4, 3)
    bits = {name: [cycle[(i + b) % 7] for b in range(2)] for i, name in enumerate(LINEARS)}       # a mixed per-linear assignment
    prompts = torch.randint(0, 1000, (8, 8), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        text = dense.generate(prompts, min_new_tokens=56, max_new_tokens=56, do_sample=False, num_beams=1)
    samples = [text[i:i + 1].cpu() for i in range(8)]
    # o_proj: 130 of 256 columns stay fp16 (Kp = 128 < K); one linear without outliers (a plain sibling in a staged set: k_proj beside q / v, or
    # down_proj behind the staged SiLU*mul); the rest by the reference's rule
    n_out = {"self_attn.o_proj": 130, "self_attn.k_proj" if n_kv == 2 else "mlp.down_proj": 0}
    ours, report = quantize_model_owq(copy.deepcopy(dense), {"linear": bits}, samples, n_out=n_out)
    return dense, ours, text, report


def modules_of(model):
    from amq_amd.arch import LINEARS
    for b, layer in enumerate(model.model.layers):
        for name in LINEARS:
            parent, attr = name.split(".")
            yield b, name, getattr(getattr(layer, parent), attr)


def test_the_model_holds_what_the_tests_below_need():
    from amq_amd.quant_linear import HIPOWQLinear, HIPQuantLinear
    for n_kv in (2, 1):
        _, ours, _, _ = owq_model(n_kv)
        plain = "self_attn.k_proj" if n_kv == 2 else "mlp.down_proj"
        for b, name, m in modules_of(ours):
            if name == plain:
                assert type(m) is HIPQuantLinear
            else:
                assert isinstance(m, HIPOWQLinear) and m.n_out > 0
            if name == "self_attn.o_proj":
                assert m.n_out == 130 and m.packed_features == 128 < m.infeatures


@torch.no_grad()
def fp64_logits(model, ids):
    """ids [S] -> logits [S, vocab] fp64: the Llama forward in fp64 torch over the modules' dequantize()'d weights"""
    cfg = model.config
    H, nh, nkv = cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads
    hd, eps, S = H // nh, cfg.rms_norm_eps, ids.numel()
    W = {(b, name): m.dequantize().double() for b, name, m in modules_of(model)}
    bias = {(b, name): (None if m.bias is None else m.bias.double()) for b, name, m in modules_of(model)}

    def lin(b, name, t):
        y = t @ W[(b, name)].t()
        return y if bias[(b, name)] is None else y + bias[(b, name)]

    def rms(t, w):
        return w.double() * (t * torch.rsqrt((t * t).mean(-1, keepdim=True) + eps))

    inv = model.model.rotary_emb.inv_freq.double().to(DEV)
    ang = torch.arange(S, device=DEV).double()[:, None] * inv[None]
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1)[:, None], torch.cat([ang.sin(), ang.sin()], -1)[:, None]

    def rope(t):
        rot = torch.cat([-t[..., hd // 2:], t[..., :hd // 2]], -1)
        return t * cos + rot * sin

    x = model.model.embed_tokens.weight.double()[ids.to(DEV)]
    mask = torch.full((S, S), float("-inf"), device=DEV, dtype=torch.float64).triu(1)
    for b, layer in enumerate(model.model.layers):
        h = rms(x, layer.input_layernorm.weight)
        q = rope(lin(b, "self_attn.q_proj", h).view(S, nh, hd))
        k = rope(lin(b, "self_attn.k_proj", h).view(S, nkv, hd)).repeat_interleave(nh // nkv, 1)
        v = lin(b, "self_attn.v_proj", h).view(S, nkv, hd).repeat_interleave(nh // nkv, 1)
        p = torch.softmax(torch.einsum("snd,tnd->nst", q, k) / np.sqrt(hd) + mask, -1)
        x = x + lin(b, "self_attn.o_proj", torch.einsum("nst,tnd->snd", p, v).reshape(S, H))
        h = rms(x, layer.post_attention_layernorm.weight)
        x = x + lin(b, "mlp.down_proj", torch.nn.functional.silu(lin(b, "mlp.gate_proj", h)) * lin(b, "mlp.up_proj", h))
    return rms(x, model.model.norm.weight) @ model.lm_head.weight.double().t()


def runner_run(r, ids, steps, use_graph):
    """prompt pass + steps token steps -> (tokens [steps + 1], the logits of the prompt's last row and of every step [steps + 1, vocab] fp16)"""
    r.reset()
    r.prefill(ids, use_graph=use_graph)
    toks, logits = [r.token.clone()], [r.logits.view(-1, r.vocab).clone()]
    for _ in range(steps):
        r.decode_step(use_graph)
        toks.append(r.token.clone())
        logits.append(r.logits.view(-1, r.vocab).clone())
    return torch.stack(toks), torch.stack(logits)


def prompt(seed, n=PROMPT):
    return torch.randint(0, 1000, (n,), generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("n_kv", [2, 1])
def test_runner_builds_and_matches_the_fp64_forward_as_well_as_the_modules_do(n_kv):
    """QuantLlama.from_hf over HIPOWQLinear modules: refused before this feature ("expected a HIPQuantLinear").  17 prompt tokens + 8 greedy steps:
    the logits of the 9 rows that choose a token against an fp64 forward over the dequantized weights on the runner's own tokens; HF's forward over
    the modules (a prompt pass and 8 one-token steps on its KV cache, fed the same tokens) is the yardstick: max |logit error| e_mod.  The runner
    rounds each outlier partial to fp16 before the packed product instead of after -- one more fp16 rounding per linear among a pipeline of
    comparable ones -- and must stay within 2 x e_mod."""
    from amq_amd.llama import QuantLlama
    _, ours, _, _ = owq_model(n_kv)
    r = QuantLlama.from_hf(ours, max_seq=64)
    assert r.owq and r.plan.staged
    assert r.linear_bytes_per_token() > sum(l.qn.numel() * 4 + l.mn.numel() * 2 for blk in r.blocks for l in (blk[n] for n in r.cfg["linear"]))
    ids = prompt(21)
    toks, logits = runner_run(r, ids, STEPS, use_graph=False)
    r.check()
    seq = torch.cat([ids, toks[:STEPS, 0]])                          # the 25 tokens whose rows 16 .. 24 chose toks[0 .. 8]
    want = fp64_logits(ours, seq)[PROMPT - 1:]
    with torch.no_grad():
        out = ours(seq[None, :PROMPT], use_cache=True)
        rows, past = [out.logits[0, -1]], out.past_key_values
        for t in toks[:STEPS, 0]:
            out = ours(t.view(1, 1), past_key_values=past, use_cache=True)
            rows.append(out.logits[0, -1])
            past = out.past_key_values
    e_mod = float((torch.stack(rows).double() - want).abs().max())
    e_run = float((logits[:, 0].double() - want).abs().max())
    OBSERVED[f"logits_n_kv{n_kv}"] = {"e_mod": e_mod, "e_runner": e_run, "max_abs_logit": float(want.abs().max())}
    print(f"n_kv={n_kv}: max |logit - fp64| modules {e_mod:.4e}, runner {e_run:.4e}, of max |logit| {float(want.abs().max()):.3f}")
    assert e_run <= 2.0 * e_mod, (e_run, e_mod)
    # the replayed graphs (prompt and step) give the eager launches' bits
    toks_g, logits_g = runner_run(r, ids, STEPS, use_graph=True)
    assert torch.equal(toks_g, toks) and same(logits_g, logits)
    r.check()


def test_a_model_without_owq_layers_keeps_its_plan():
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = dict(arch._cfg(2, 256, 512, 2, 2, 1, vocab=1000))
    for B in (1, 3):
        m = QuantLlama(cfg, None, device=DEV, max_seq=32, seed=4, batch=B)
        assert not m.owq and not m.plan.staged and m._staged is None


@pytest.mark.parametrize("n_kv", [2, 1])
def test_batched_runner_against_single_sequence_runs(n_kv):
    """batch = 3: every sequence against its own batch-1 run, bit for bit -- tokens and the logits of every step.  The stage kernel is
    row-independent by its specification (section 1: every row count against the same composition) and the packed GEMV gives a row the same bits
    among 3 rows as alone at these widths.  (The plain runner's own batched tests, tests/test_gpu_decode.py and tests/test_gpu_ragged.py, hold a
    batch to its single-sequence runs within 1e-2 of the largest logit and on 0.8 of the greedy choices; that yardstick is asserted first, so a
    failure says which of the two was missed.)  Graph == eager."""
    from test_gpu_ragged import _against_each_alone
    from amq_amd.llama import QuantLlama
    _, ours, _, _ = owq_model(n_kv)
    B, steps = 3, STEPS
    ids = torch.stack([prompt(31 + b) for b in range(B)])
    mb = QuantLlama.from_hf(ours, max_seq=64, batch=B)
    mb.prefill(ids, use_graph=False)
    toks, logits = [mb.token.clone()], [mb.logits.float().view(B, -1).clone()]
    for _ in range(1, steps):
        mb.decode_step(False)
        toks.append(mb.token.clone())
        logits.append(mb.logits.float().view(B, -1).clone())
    toks, logits = torch.stack(toks, 1), torch.stack(logits)
    mb.check()
    m1 = QuantLlama.from_hf(ours, max_seq=64)
    _against_each_alone(m1, ids, [PROMPT] * B, toks, logits)
    exact = []
    for b in range(B):
        t1, l1 = runner_run(m1, ids[b], steps - 1, use_graph=False)
        exact.append(bool(torch.equal(t1[:, 0], toks[b])) and same(l1[:, 0].float(), logits[:, b]))
    OBSERVED[f"batch3_rows_bit_equal_n_kv{n_kv}"] = exact
    print("batch-3 rows bit-equal to their batch-1 runs:", exact)
    assert all(exact), exact
    mb.reset()
    out_g = mb.generate(ids, steps, use_graph=True)
    assert torch.equal(out_g, toks) and torch.equal(mb.logits.float().view(B, -1), logits[-1])
    mb.check()


def test_ragged_batch_against_single_sequence_runs():
    """prompts of unequal length: as tests/test_gpu_ragged.py asserts for plain models"""
    from test_gpu_ragged import _against_each_alone, _ragged_run
    from amq_amd.llama import QuantLlama
    _, ours, _, _ = owq_model(2)
    lengths, S, steps = [17, 5, 11], 17, 14
    ids = torch.stack([prompt(41 + b) for b in range(3)])
    for b, n in enumerate(lengths):
        ids[b, n:] = 0
    mb = QuantLlama.from_hf(ours, max_seq=64, batch=3, ragged=True)
    toks, logits = _ragged_run(mb, ids, lengths, steps)
    assert mb.pos.tolist() == [n + steps - 1 for n in lengths]
    mb.check()
    _against_each_alone(QuantLlama.from_hf(ours, max_seq=64), ids, lengths, toks, logits)
    mb.reset()
    out_g = mb.generate(ids, steps, use_graph=True, lengths=lengths)
    assert torch.equal(out_g, toks) and torch.equal(mb.logits.float().view(3, -1), logits[-1])
    mb.check()


@pytest.mark.parametrize("n_kv", [2, 1])
def test_lookup_runner_gives_the_plain_greedy_output(n_kv):
    from amq_amd.llama import QuantLlama
    _, ours, text, _ = owq_model(n_kv)
    ids = text[0, :PROMPT].contiguous()                               # (text the dense model wrote: something to look up)
    plain = QuantLlama.from_hf(ours, max_seq=64).generate(ids, STEPS)
    look = QuantLlama.from_hf(ours, max_seq=64, lookup=3)
    assert look.plan.staged and look.R == 4
    got = look.generate(ids, STEPS)
    look.check()
    assert torch.equal(got.reshape(-1)[:STEPS], plain.reshape(-1)), (got.tolist(), plain.tolist())


def test_the_ab_step_forms_are_refused():
    from amq_amd.llama import QuantLlama
    _, ours, _, _ = owq_model(2)
    with pytest.raises(ValueError, match="OWQ"):
        QuantLlama.from_hf(ours, max_seq=64, engine=True)

    class Fused(QuantLlama):
        FUSE_QKV_ATTN = True

    with pytest.raises(ValueError, match="OWQ"):
        Fused.from_hf(ours, max_seq=64)


def test_hf_surface_generate_and_runner_reuse():
    from amq_amd import hf_fast
    from amq_amd.llama import QuantLlama
    _, ours, _, _ = owq_model(2)
    ids = prompt(51)[None]
    eos = ours.generation_config.eos_token_id
    eos = [] if eos is None else (list(eos) if isinstance(eos, (list, tuple)) else [eos])
    r = QuantLlama.from_hf(ours, max_seq=64)
    r.set_suppressed(eos)
    want = r.generate(ids[0], STEPS)
    try:
        hf_fast.convert_model_to_hip(ours)
        with torch.no_grad():
            out = ours.generate(ids, max_new_tokens=STEPS, min_new_tokens=STEPS, do_sample=False)
        bound = dict(hf_fast._RUNNERS[ours])
        assert bound and all(b.owq for b in bound.values())                          # the call went through a staged runner
        assert torch.equal(out[0, :PROMPT], ids[0]) and torch.equal(out[0, PROMPT:], want)
        with torch.no_grad():
            again = ours.generate(ids, max_new_tokens=STEPS, min_new_tokens=STEPS, do_sample=False)
        assert torch.equal(again, out)
        assert all(hf_fast._RUNNERS[ours][k] is b for k, b in bound.items())        # _same_weights: the runner is reused
        with torch.no_grad():
            open_ended = ours.generate(ids, max_new_tokens=STEPS, do_sample=False)      # (HF's own loop over the patched forward)
        n = open_ended.shape[1] - PROMPT
        OBSERVED["hf_open_ended_equal_tokens"] = int((open_ended[0, PROMPT:] == want[:n]).sum()), n
    finally:
        hf_fast.revert_model_to_hf(ours)


def test_benchmark_speed_builds_its_runner_over_the_modules():
    """the harness' fast path (use_ft=True) over an OWQ model: QuantLlama.from_hf inside benchmark_speed, the token step captured and timed"""
    from amq_amd.speed import benchmark_speed
    _, ours, _, _ = owq_model(2)
    data = benchmark_speed(ours, None, use_ft=True, iteration=1, sizes=(1, 16, 8), mode="TPS", get_peak_memory=False)
    assert data["tps"] and all(v > 0 for v in data["tps"].values()), data


def hf_forward_logits(model, windows):
    with torch.no_grad():
        return [model(w.to(DEV)).logits for w in windows]


def test_eval_ppl_and_eval_loss_on_the_runners_own_logits():
    """evaluate.eval_ppl / eval_loss over two 64-token windows of an OWQ model, against the same reductions in fp64 torch over the logits of the
    runner's own scoring pass, within the bars tests/test_gpu_evalmetrics.py holds plain models to"""
    from amq_amd import evaluate
    from amq_amd.llama import QuantLlama
    dense, ours, text, _ = owq_model(2)
    windows = [text[0:1].cpu(), text[1:2].cpu()]
    dense_logits = hf_forward_logits(dense, windows)
    r = QuantLlama.from_hf(ours, max_seq=64)
    nll_rows, jsd_rows, nll_bar, jsd_bar = [], [], mref.NLL_FLOOR, mref.JSD_FLOOR
    for w, d in zip(windows, dense_logits):
        last = torch.empty(1, r.vocab, dtype=torch.float16, device=DEV)
        mine = r._logits_of_rows(r._rows_pass(w.to(DEV), 0, cache=False), 1, 64, last)
        flat, dflat, lab = mine[0, :-1].cpu(), d[0, :-1].cpu(), w[0, 1:]
        en, ej = mref.nll_expected(flat, lab), mref.jsd_expected(flat, dflat)
        nll_bar, jsd_bar = max(nll_bar, en["nll_bar"]), max(jsd_bar, ej["jsd_bar"])
        nll_rows.append(en["nll"].view(1, 63))
        jsd_rows.append(ej["jsd"].view(1, 63))
    for seqlen in (64, 2048):
        ppl = evaluate.eval_ppl(ours, None, windows, seqlen=seqlen)
        loss = evaluate.eval_loss(ours, None, windows, dense_logits, seqlen=seqlen)
        want_ppl, want_loss = mref.ppl_of(nll_rows, seqlen), mref.loss_of(jsd_rows, seqlen)
        print("own logits: eval_ppl", ppl, want_ppl, "eval_loss", loss, want_loss)
        assert abs(np.log(ppl) - np.log(want_ppl)) <= 3 * nll_bar
        assert abs(loss - want_loss) <= 3 * jsd_bar


def test_eval_ppl_and_eval_loss_against_the_hf_forward_logits():
    """The same two metrics against fp64 torch over the logits of HF's forward over the modules, at the same bars (3 x the per-row bar of
    tests/evalmetrics_ref.py, as tests/test_gpu_evalmetrics.py::test_score_rows_and_evaluate_end_to_end)."""
    from amq_amd import evaluate
    dense, ours, text, _ = owq_model(2)
    windows = [text[0:1].cpu(), text[1:2].cpu()]
    dense_logits = hf_forward_logits(dense, windows)
    mod_logits = hf_forward_logits(ours, windows)
    nll_rows, jsd_rows, nll_bar, jsd_bar = [], [], mref.NLL_FLOOR, mref.JSD_FLOOR
    for w, m, d in zip(windows, mod_logits, dense_logits):
        flat, dflat, lab = m[0, :-1].cpu(), d[0, :-1].cpu(), w[0, 1:]
        en, ej = mref.nll_expected(flat, lab), mref.jsd_expected(flat, dflat)
        nll_bar, jsd_bar = max(nll_bar, en["nll_bar"]), max(jsd_bar, ej["jsd_bar"])
        nll_rows.append(en["nll"].view(1, 63))
        jsd_rows.append(ej["jsd"].view(1, 63))
    ppl = evaluate.eval_ppl(ours, None, windows, seqlen=64)
    loss = evaluate.eval_loss(ours, None, windows, dense_logits, seqlen=64)
    want_ppl, want_loss = mref.ppl_of(nll_rows, 64), mref.loss_of(jsd_rows, 64)
    OBSERVED["eval_vs_hf_forward"] = {"ppl": ppl, "ppl_hf_forward_fp64": want_ppl, "loss": loss, "loss_hf_forward_fp64": want_loss,
                                      "bar_log_ppl": 3 * nll_bar, "bar_loss": 3 * jsd_bar}
    print("HF-forward logits: eval_ppl", ppl, want_ppl, "eval_loss", loss, want_loss, "bars", 3 * nll_bar, 3 * jsd_bar)
    assert abs(np.log(ppl) - np.log(want_ppl)) <= 3 * nll_bar
    assert abs(loss - want_loss) <= 3 * jsd_bar


def test_zz_observed_parity_is_recorded():
    """last in the file: what the device gave above goes to profiles/owq_decode.json under "parity" """
    if "logits_n_kv2" not in OBSERVED:      # (run alone: nothing to record)
        return
    try:
        doc = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        doc["parity"] = {"device": torch.cuda.get_device_name(0), "cases": OBSERVED}
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError as e:                    # a read-only checkout: the assertions above are what counts
        print("not recorded:", e)
