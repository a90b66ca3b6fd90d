"""What sampled decoding costs: the captured token step ending in the greedy tail (decode_tail_kernel) against the one ending in the sampled tail
(sample_kernel, amq_sample.hip) at temperature 0.8 / top_k 50 / top_p 0.9, in one process, on the 7B avg-3 synthetic model bench.py uses and on
the Qwen2.5-7B shape (vocab 152064).  Each leg is timed ``--repeats`` times, alternating, so the run-to-run spread is part of the result.

    python tools/sampling_bench.py [--models Llama-2-7b-hf,Qwen2.5-7B] [--steps 256] [--repeats 5] [--greedy-only] [--out profiles/sampling_step.json]

``--greedy-only`` runs on a tree without the sampled tail too (the "greedy step must not move" comparison against the parent commit).
Kernel durations of the two tails: run the same command under ``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/sampling_bench.py ...`` and
read decode_tail_kernel / sample_kernel from the stats file (a traced run's step times are not the ones to quote).
``--hf``: generate(do_sample=True) on a 2-layer HF Llama with the 7B widths and vocabulary, converted with and without sampling=True."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _time_steps(m, steps, sampled):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.decode_step(True, sampled=sampled) if sampled is not None else m.decode_step(True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def step_times(model, steps, repeats, greedy_only, prompt=64):
    import bench
    dev = torch.device("cuda:0")
    m, _, _ = bench.build_model(dev, max_seq=prompt + 8 + steps, model=model, pinned=() if model != bench.MODEL else None)
    ids = torch.randint(3, m.vocab, (prompt,), generator=torch.Generator().manual_seed(0)).to(dev)
    legs = {"greedy": []} if greedy_only else {"greedy": [], "sampled": []}
    if not greedy_only:
        m.set_sampling(temperature=0.8, top_k=50, top_p=0.9, seed=1)
    for rep in range(repeats + 1):                      # (the first round captures and warms up: not kept)
        for leg in legs:
            m.prefill(ids)
            t = _time_steps(m, steps, None if greedy_only else leg == "sampled")
            if rep:
                legs[leg].append(t)
    res = {"model": model, "vocab": m.vocab, "steps": steps, "prompt": prompt}
    for leg, ts in legs.items():
        res[leg + "_ms"] = statistics.median(ts)
        res[leg + "_ms_runs"] = [round(t, 5) for t in ts]
        res[leg + "_spread_pct"] = 100.0 * (max(ts) - min(ts)) / statistics.median(ts)
        res[leg + "_tokens_per_s"] = 1e3 / statistics.median(ts)
    if not greedy_only:
        res["sampled_over_greedy_pct"] = 100.0 * (res["sampled_ms"] / res["greedy_ms"] - 1.0)
    return res


def hf_generate(new_tokens=64, repeats=3):
    """a 2-layer Llama with the 7B widths and vocabulary, random HQQ weights: generate(do_sample=True, top_k=50, top_p=0.9), HF's loop vs the runner"""
    import transformers
    from amq_amd import hf_fast
    from amq_amd.hqq_format import random_hqq
    from amq_amd.patching import HQQWeightsModule, prepare_for_inference
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=32,
                                   vocab_size=32000, max_position_embeddings=1024, attn_implementation="eager")
    model = transformers.LlamaForCausalLM(cfg).to(torch.float16).to(dev).eval()
    i = 0
    for layer in model.model.layers:
        for parent in (layer.self_attn, layer.mlp):
            for name in ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"):
                lin = getattr(parent, name, None)
                if lin is not None:
                    n, k = lin.weight.shape
                    setattr(parent, name, HQQWeightsModule(random_hqq(n, k, (4, 2, 3, 3, 2, 4, 3)[i % 7], seed=i).to(dev)))
                    i += 1
    prepare_for_inference(model, backend="hip")
    ids = torch.randint(3, 32000, (1, 64), generator=torch.Generator().manual_seed(0)).to(dev)
    kw = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.8, min_new_tokens=new_tokens, max_new_tokens=new_tokens,
              attention_mask=torch.ones_like(ids), pad_token_id=0)
    out = {}
    for name, flag in (("hf_loop", False), ("runner", True)):
        hf_fast.convert_model_to_hip(model, sampling=flag)
        ts = []
        for rep in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate(ids, **kw)
            torch.cuda.synchronize()
            if rep:
                ts.append(new_tokens / (time.perf_counter() - t0))
        out[name + "_tokens_per_s"] = statistics.median(ts)
    out["speedup"] = out["runner_tokens_per_s"] / out["hf_loop_tokens_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="Llama-2-7b-hf,Qwen2.5-7B")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--greedy-only", action="store_true")
    ap.add_argument("--hf", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"steps": [step_times(mod, a.steps, a.repeats, a.greedy_only) for mod in a.models.split(",") if mod]}
    if a.hf:
        res["hf_generate"] = hf_generate()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
