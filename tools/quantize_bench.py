"""What quantizing a 7B model costs: ops.hqq_quantize (solve + stop + emit kernels and its one 88-byte read-back) per layer shape of Llama-2-7B at
2 / 3 / 4 bit, group 128, against the same solver run as framework passes on the same device:

  kernel   ops.hqq_quantize(W, bits, 128)
  torch    tests/hqq_solver_ref.solve(W, bits, 128) on the GPU + hqq_format.pack_rows -- the loop as torch ops, what running the reference's Python on
           ROCm gives (its fp32 arithmetic; about 15 passes per iteration over an fp32 copy of W)

The comparison leg is the reference's procedure, not the code under test.  Legs alternate in one process; median of ``--repeats`` after one warm-up
round, spreads beside it.  The model total is 32 blocks x (4 attention + 2 gate / up + 1 down) layers x the three bit-widths (the per-bit model bank the
search holds).  The result is merged into ``--out`` under "timing" (tests/test_gpu_hqq_quantize.py keeps its observed counts under "parity" there).

    python tools/quantize_bench.py [--repeats 5] [--out profiles/hqq_quantize.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

DEV = "cuda:0"
# (name, N, K, layers per block): the linears of Llama-2-7B
SHAPES = [("attention q/k/v/o", 4096, 4096, 4), ("mlp gate/up", 11008, 4096, 2), ("mlp down", 4096, 11008, 1)]
BLOCKS = 32


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    del out
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import hqq_solver_ref as ref
    from amq_amd import ops
    from amq_amd.hqq_format import pack_rows

    def torch_leg(W, bits):
        r = ref.solve(W, bits, 128)
        return pack_rows(r["q"], bits), r["scale"], r["zero"]

    rows, total = [], {"kernel_ms": 0.0, "torch_ms": 0.0}
    with torch.inference_mode():
        for name, N, K, per_block in SHAPES:
            W = (torch.randn(N, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(N + K)) * 0.02).to(torch.float16)
            for bits in (2, 3, 4):
                legs = {"kernel": lambda: ops.hqq_quantize(W, bits, 128), "torch": lambda: torch_leg(W, bits)}
                runs = {k: [] for k in legs}
                for rep in range(a.repeats + 1):            # (the first round warms up: not kept)
                    for leg, fn in legs.items():
                        ms = _timed(fn)
                        if rep:
                            runs[leg].append(ms)
                    torch.cuda.empty_cache()
                row = {"layer": name, "N": N, "K": K, "bits": bits, "group": 128, "layers_per_block": per_block, "repeats": a.repeats}
                for leg, ts in runs.items():
                    row[leg + "_ms"] = round(statistics.median(ts), 3)
                    row[leg + "_ms_runs"] = [round(t, 3) for t in ts]
                    row[leg + "_spread_pct"] = round(100.0 * (max(ts) - min(ts)) / statistics.median(ts), 2)
                    total[leg + "_ms"] += row[leg + "_ms"] * per_block * BLOCKS
                row["torch_over_kernel"] = round(row["torch_ms"] / row["kernel_ms"], 2)
                rows.append(row)
                print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "layers": rows,
           "model": {"name": "Llama-2-7b-hf", "what": "every decoder linear at 2, 3 and 4 bit (sum of the per-layer medians)",
                     "kernel_s": round(total["kernel_ms"] / 1e3, 3), "torch_s": round(total["torch_ms"] / 1e3, 3),
                     "torch_over_kernel": round(total["torch_ms"] / total["kernel_ms"], 2)}}
    print(json.dumps(res["model"]), flush=True)
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["timing"] = res
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
