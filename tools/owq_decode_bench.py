"""What the staged token step costs (DESIGN.md 3.12 "In the runner"): a Llama-2-7B-shaped model at 3 bit, group 128, whose linears are OWQ layers
with ``n_out`` by the reference's rule at 3.25 average bits (54 / 20 / 54 fp16 columns: attention, gate / up, down) -- synthetic packed weights,
random outlier positions, random fp16 outlier columns (values do not affect speed) -- decoded

  owq_runner     QuantLlama.from_hf over the HIPOWQLinear modules: the staged plan, 12 launches a block, replayed from its hipGraph
  plain_runner   QuantLlama of the same shapes and bits without outliers: the five-launch step, from its hipGraph
  plain_staged   the plain runner's weights walked by the staged plan (every part a plain sibling: the stage launches only normalise / activate,
                 then one GEMV per linear): the launch structure without the outlier columns and gathers -- what of the gap is launch count
  hf_forward     the same OWQ model under HF's own generate over the modules (what an OWQ model ran under before the runner took it)

in one process, the runner legs alternating, medians of ``--repeats`` windows of ``--steps`` steps after a warm-up window, spreads beside them.
Also one 2048-token scoring window: ``score_rows`` of the OWQ runner and of the plain one, and HF's forward + cross entropy over the modules.
The result is merged into ``--out`` under "timing" (tests/test_gpu_owq_runner.py keeps its observed parity under "parity").

    python tools/owq_decode_bench.py [--repeats 5] [--steps 128] [--blocks 32] [--out profiles/owq_decode.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = "cuda:0"
BITS, AVG_BITS, PROMPT, WINDOW = 3, 3.25, 64, 2048


def synthetic_owq_model(blocks, seed=0):
    """a LlamaForCausalLM of Llama-2-7B's shapes (``blocks`` decoder layers) on the GPU whose decoder linears are synthetic HIPOWQLinear modules"""
    from transformers import LlamaConfig, LlamaForCausalLM
    from amq_amd import ops
    from amq_amd.arch import LINEARS
    from amq_amd.llama import _synthetic_linear
    from amq_amd.patching import owq_n_out
    from amq_amd.quant_linear import HIPOWQLinear
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=blocks, num_attention_heads=32, num_key_value_heads=32,
                      vocab_size=32000, max_position_embeddings=4096, rms_norm_eps=1e-5, attn_implementation="sdpa")
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        with torch.device(DEV):
            model = LlamaForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(before)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    n_outs = {}
    for layer in model.model.layers:
        for name in LINEARS:
            parent, attr = name.split(".")
            dense = getattr(getattr(layer, parent), attr)
            N, K = dense.weight.shape
            n_out = owq_n_out(K, AVG_BITS, name)
            n_outs[name] = n_out
            Kp = ops.owq_packed_columns(K, n_out)
            mod = HIPOWQLinear(BITS, 128, K, N, n_out, name=attr)
            lin = _synthetic_linear(N, Kp, BITS, gen, torch.device(DEV))
            mod.inner._set_native(lin.qn, lin.mn, lin.mode)
            ids = torch.randperm(K, device=DEV, generator=gen)
            perm = torch.full((Kp,), -1, dtype=torch.int32, device=DEV)
            perm[:K - n_out] = ids[:K - n_out].to(torch.int32)
            mod.perm, mod.out_ids = perm, torch.sort(ids[K - n_out:])[0].to(torch.int32).contiguous()
            mod.W_out = (torch.randn(N, n_out, device=DEV, generator=gen) * 0.02).to(torch.float16)
            setattr(getattr(layer, parent), attr, mod)
    torch.cuda.empty_cache()
    return model, n_outs


def staged_over_plain(r):
    """the plain runner's weights under the staged plan: every part is a plain sibling (no gather, no outlier columns)"""
    from amq_amd.llama import DOWN_GEMV, NORM_LAUNCH, StepPlan
    r.owq = True
    r.plan = StepPlan(NORM_LAUNCH, NORM_LAUNCH, DOWN_GEMV, staged=True)
    r._staged = r._build_staged()
    r.graph = r.sample_graph = None
    return r


def window_ms(r, ids, steps):
    """ms of ``steps`` replayed token steps behind a prompt pass"""
    r.reset()
    r.prefill(ids)
    r.decode_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        r.decode_step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed_ms(fn, repeats=3):
    fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--max-seq", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "owq_decode.json"))
    args = ap.parse_args()
    from amq_amd.arch import MODEL_CONFIGS, uniform_arch
    from amq_amd.llama import QuantLlama

    model, n_outs = synthetic_owq_model(args.blocks)
    cfg = dict(MODEL_CONFIGS["Llama-2-7b-hf"], n_block=args.blocks)
    arch = uniform_arch(cfg, BITS)["linear"]
    legs = {"owq_runner": QuantLlama.from_hf(model, max_seq=args.max_seq),
            "plain_runner": QuantLlama(cfg, arch, device=DEV, max_seq=args.max_seq, seed=1),
            "plain_staged": staged_over_plain(QuantLlama(cfg, arch, device=DEV, max_seq=args.max_seq, seed=1))}
    ids = torch.randint(0, 32000, (PROMPT,), generator=torch.Generator().manual_seed(2)).to(DEV)
    runs = {k: [] for k in legs}
    for rep in range(args.repeats + 1):             # (the first window warms up: graphs are captured in it)
        for k, r in legs.items():
            ms = window_ms(r, ids, args.steps)
            if rep:
                runs[k].append(ms)
    timing = {"device": torch.cuda.get_device_name(0), "model": f"Llama-2-7B shapes, {args.blocks} blocks, {BITS} bit, group 128",
              "n_out": n_outs, "prompt": PROMPT, "steps": args.steps, "repeats": args.repeats, "max_seq": args.max_seq, "decode": {}}
    for k, ts in runs.items():
        med = statistics.median(ts)
        timing["decode"][k] = {"ms_per_step": round(med / args.steps, 4), "tokens_per_s": round(1e3 * args.steps / med, 1),
                               "spread_pct": round(100.0 * (max(ts) - min(ts)) / med, 2),
                               "linear_bytes_per_token": legs[k].linear_bytes_per_token()}
    # HF's own generate over the modules: per-token time from two lengths (the prompt pass and the call's fixed costs cancel)
    def hf_generate(n):
        with torch.no_grad():
            model.generate(ids[None], min_new_tokens=n, max_new_tokens=n, do_sample=False, num_beams=1, attention_mask=torch.ones_like(ids[None]))
    short, long = 8, 40
    hf_ms = (timed_ms(lambda: hf_generate(long)) - timed_ms(lambda: hf_generate(short))) / (long - short)
    timing["decode"]["hf_forward"] = {"ms_per_step": round(hf_ms, 4), "tokens_per_s": round(1e3 / hf_ms, 1)}
    d = timing["decode"]
    gap = d["owq_runner"]["ms_per_step"] - d["plain_runner"]["ms_per_step"]
    launches = d["plain_staged"]["ms_per_step"] - d["plain_runner"]["ms_per_step"]
    timing["gap"] = {"owq_minus_plain_ms_per_step": round(gap, 4), "staged_structure_alone_ms_per_step": round(launches, 4),
                     "share_of_gap_that_is_launch_structure": round(launches / gap, 3) if gap > 0 else None,
                     "launches_per_block": {"plain_runner": 5, "plain_staged": 11, "owq_runner": 12}}
    # one scoring window
    for k in ("owq_runner", "plain_runner"):
        legs[k] = None
    torch.cuda.empty_cache()
    win = torch.randint(0, 32000, (1, WINDOW), generator=torch.Generator().manual_seed(3)).to(DEV)
    score_owq = QuantLlama.from_hf(model, max_seq=WINDOW)
    score_plain = QuantLlama(cfg, arch, device=DEV, max_seq=WINDOW, seed=1)

    def hf_score():
        with torch.no_grad():
            lg = model(win).logits
            return torch.nn.functional.cross_entropy(lg[0, :-1].float(), win[0, 1:], reduction="none")

    timing["score_window_ms"] = {"tokens": WINDOW, "owq_runner": round(timed_ms(lambda: score_owq.score_rows(win)), 2),
                                 "plain_runner": round(timed_ms(lambda: score_plain.score_rows(win)), 2),
                                 "hf_forward": round(timed_ms(hf_score), 2)}
    print(json.dumps(timing, indent=1))
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["timing"] = timing
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
