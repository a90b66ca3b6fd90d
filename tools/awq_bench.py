"""What AWQ's two weight-side passes cost per layer shape of Llama-2-7B at 3 bit, group 128, T = 512 sampled rows:

  clip_kernel      ops.awq_clip(W, X, 3, 128): the search on the matrix cores (v_mfma_f32_16x16x4_f32: the form that ran is recorded as "clip_form")
                   and its one 4-byte read-back
  clip_torch       the reference's procedure (awq_utils/auto_clip.py:27-87: slabs of 256 rows, per slab the dense outputs and 10 clipped,
                   fake-quantized candidates as [256, T, K / G, G] fp16 temporaries) restated as torch fp16 ops on the same device
  search_kernel    ops.awq_quantize(W, 3, 128, col_scale=s, dense=True): one fake-quantization of the scale search (it runs 20 per search)
  search_torch     the same as torch fp16 ops (scale, pseudo-quantize per group, unscale)
  pack_kernel      ops.awq_quantize(W, 3, 128, hi=hi, lo=lo): bounds to Format A

The comparison legs are the reference's procedure, not the code under test: their fp16 arithmetic and summation order are torch's, so their bits
are not the kernels'.  The legs alternate in one process; median of ``--repeats`` after one warm-up round, spreads beside it.  The result is
merged into ``--out`` under "timing" (the tests keep their observed parity under "parity" and "cpu_parity" there).

    python tools/awq_bench.py [--repeats 5] [--tokens 512] [--out profiles/awq_quantize.json]
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
SHAPES = [("attention q/k/v/o", 4096, 4096), ("mlp gate/up", 11008, 4096), ("mlp down", 4096, 11008)]
BITS, GROUP, STEPS = 3, 128, 10
CLIP_FORM = "v_mfma_f32_16x16x4_f32, one wave per (8 rows, group), X read from global memory per wave"


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    del out
    return ms


def torch_fake_quant(w, bits, group):
    """pseudo_quantize_tensor (zero_point) over the last dimension's groups, in w's dtype"""
    shape = w.shape
    w = w.reshape(-1, group)
    maxq = 2 ** bits - 1
    mx, mn = w.amax(dim=1, keepdim=True), w.amin(dim=1, keepdim=True)
    s = (mx - mn).clamp(min=1e-5) / maxq
    z = (-torch.round(mn / s)).clamp_(0, maxq)
    return ((torch.clamp(torch.round(w / s) + z, 0, maxq) - z) * s).reshape(shape)


def torch_clip(W, X, bits, group):
    """auto_clip_layer_asym's loop as torch ops on W's device: (best_max, best_min) [N, K / group, 1]"""
    N, K = W.shape
    x = X.reshape(1, X.shape[0], -1, group)
    w_all = W.reshape(N, 1, -1, group)
    slab = 256 if N % 256 == 0 else 64
    his, los = [], []
    for lo_row in range(0, N, slab):
        w = w_all[lo_row:lo_row + slab]
        org = (x * w).sum(dim=-1)
        mx, mn = w.amax(dim=-1, keepdim=True), w.amin(dim=-1, keepdim=True)
        best_hi, best_lo = mx.clone(), mn.clone()
        errs = torch.full_like(mx, float("inf"))       # (the reference's 1e9 does not fit fp16)
        for i in range(STEPS):
            hi, lo = mx * (1 - i / 20), mn * (1 - i / 20)
            q = torch_fake_quant(torch.clamp(w, lo, hi), bits, group)
            err = ((x * q).sum(dim=-1) - org).pow(2).mean(dim=1).view(errs.shape)
            better = err < errs
            errs[better] = err[better]
            best_hi[better] = hi[better]
            best_lo[better] = lo[better]
        his.append(best_hi)
        los.append(best_lo)
    return torch.cat(his).squeeze(1), torch.cat(los).squeeze(1)


def _runs(row, leg, ts):
    row[leg + "_ms"] = round(statistics.median(ts), 3)
    row[leg + "_ms_runs"] = [round(t, 3) for t in ts]
    row[leg + "_spread_pct"] = round(100.0 * (max(ts) - min(ts)) / statistics.median(ts), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from amq_amd import ops

    rows = []
    with torch.inference_mode():
        for name, N, K in SHAPES:
            g = torch.Generator(device=DEV).manual_seed(N + K)
            W = (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(torch.float16)
            X = torch.randn(a.tokens, K, device=DEV, generator=g)
            X[:, ::61] *= 10.0
            X = X.to(torch.float16)
            s = (0.5 + torch.rand(K, device=DEV, generator=g)).float()
            hi, lo = ops.awq_clip(W, X, BITS, GROUP)
            legs = {"clip_kernel": lambda: ops.awq_clip(W, X, BITS, GROUP), "clip_torch": lambda: torch_clip(W, X, BITS, GROUP),
                    "search_kernel": lambda: ops.awq_quantize(W, BITS, GROUP, col_scale=s, dense=True),
                    "search_torch": lambda: torch_fake_quant(W * s.to(W.dtype), BITS, GROUP) / s.to(W.dtype),
                    "pack_kernel": lambda: ops.awq_quantize(W, BITS, GROUP, hi=hi, lo=lo)}
            runs = {k: [] for k in legs}
            for rep in range(a.repeats + 1):            # (the first round warms up: not kept)
                for leg, fn in legs.items():
                    ms = _timed(fn)
                    if rep:
                        runs[leg].append(ms)
                torch.cuda.empty_cache()
            row = {"layer": name, "N": N, "K": K, "T": a.tokens, "bits": BITS, "group": GROUP, "repeats": a.repeats, "clip_form": CLIP_FORM}
            for leg, ts in runs.items():
                _runs(row, leg, ts)
            row["clip_kernel_tflops"] = round(2.0 * a.tokens * K * N * STEPS / (row["clip_kernel_ms"] * 1e-3) / 1e12, 2)
            row["clip_torch_over_kernel"] = round(row["clip_torch_ms"] / row["clip_kernel_ms"], 2)
            row["search_torch_over_kernel"] = round(row["search_torch_ms"] / row["search_kernel_ms"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "layers": rows}
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["timing"] = res
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
