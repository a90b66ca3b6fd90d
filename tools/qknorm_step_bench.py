"""What Qwen3's per-head q / k RMSNorm costs inside the captured token step: ms per step of a synthetic Qwen3-8B-shaped runner (36 blocks, hidden 4096,
32 / 8 heads, intermediate 12288, vocab 151936, avg-3-bit) built with the norm (the amq_*_qkn_f16 instantiations of the attention kernels) against the
same runner built ``qk_norm=False`` (the kernels every other family runs), in one process, alternating repeats, at batch 1 and 8 and at 64 and ~8000
cached keys (the single-workgroup kernel; the long-cache grouped-query route).

    python tools/qknorm_step_bench.py [--steps 128] [--repeats 5] [--batches 1,8] [--keys 64,8000] [--out profiles/qknorm_step.json]

The cache rows behind the 64-token prompt are zeros (valid fp16): only the time is read, not the tokens."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _time_steps(m, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.decode_step(True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def measure(batch, keys, steps, repeats, model="Qwen3-8B", prompt=64):
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    dev = torch.device("cuda:0")
    cfg = arch.MODEL_CONFIGS[model]
    arch_linear, usage = arch.synthesize_arch(cfg, 3.0, seed=0)
    max_seq = max(256, keys + steps + 8)
    max_seq = -(-max_seq // 256) * 256
    legs = {}
    for name, flag in (("qk_norm", True), ("no_norm", False)):
        legs[name] = QuantLlama(dict(cfg, qk_norm=flag), arch_linear["linear"], device=dev, max_seq=max_seq, batch=batch, seed=0)
    ids = torch.randint(3, cfg["vocab_size"], (batch, prompt) if batch > 1 else (prompt,), generator=torch.Generator().manual_seed(0)).to(dev)
    runs = {name: [] for name in legs}
    for rep in range(repeats + 1):                      # (the first round captures and warms up: not kept)
        for name, m in legs.items():
            m.prefill(ids)
            if keys > prompt:
                tok = m.token.clone()
                m.set_pos(keys)
                m.set_token(tok)
            t = _time_steps(m, steps)
            m.check()
            if rep:
                runs[name].append(t)
    res = {"model": model, "bits_usage": round(usage, 4), "batch": batch, "cached_keys": keys, "max_seq": max_seq, "steps": steps}
    for name, ts in runs.items():
        res[name + "_ms"] = statistics.median(ts)
        res[name + "_ms_runs"] = [round(t, 5) for t in ts]
        res[name + "_spread_pct"] = 100.0 * (max(ts) - min(ts)) / statistics.median(ts)
    res["norm_cost_us_per_step"] = 1e3 * (res["qk_norm_ms"] - res["no_norm_ms"])
    res["norm_cost_pct"] = 100.0 * (res["qk_norm_ms"] / res["no_norm_ms"] - 1.0)
    del legs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--keys", default="64,8000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"cases": []}
    for b in (int(v) for v in a.batches.split(",") if v):
        for k in (int(v) for v in a.keys.split(",") if v):
            res["cases"].append(measure(b, k, a.steps, a.repeats))
            print(json.dumps(res["cases"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
