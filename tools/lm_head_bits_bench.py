#!/usr/bin/env python3
"""The lm_head at 16 / 8 / 4 bits (QuantLlama(lm_head_bits=)), all legs in ONE process, alternating, hipGraph replay, HIP events:

  (i)   the lm_head launch alone at the three vocabularies and R = 1, 4, 8 rows: fp16 (ops.gemv_f16w), 8 bit (ops.lm8_gemv), 4 bit
        (ops.gemv_grouped, RMSNorm prologue) -- every launch of a graph reads its own copy of the layer (> 600 MB in rotation: cold in HBM);
        us per launch (median of the alternating rounds, with their min / max) and achieved GB/s on the layer's bytes;
  (ii)  the whole synthetic avg-3-bit token step (batch 1) of the three model shapes at lm_head_bits 16 / 8 / 4: the captured step replayed,
        the three runners taking turns (a step streams > 2.6 GB: cold by its size);
  (iii) logit drift of 8 and 4 bits against the fp16 lm_head on the same hidden rows, max |dlogit| / max |logit| -- SYNTHETIC Gaussian weights,
        not a perplexity;
  (iv)  what the lm_head of a 2048-row scoring window costs: the fp16 MFMA GEMM against the 8-bit weight-streaming kernel, 8 rows a launch, and
        against the route the runner takes from 64 rows on (slices of the layer dequantized into a scratch + the fp16 GEMM, per 512-row piece).

usage: lm_head_bits_bench.py [--out profiles/lm_head_bits.json] [--quick] [--only window]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from amq_amd import arch as arch_mod  # noqa: E402
from amq_amd import ops  # noqa: E402
from amq_amd.hqq_format import LM8Weights, quantize_lm8  # noqa: E402
from amq_amd.llama import QuantLlama, _synthetic_linear, lm8_logits_sliced  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [("Llama-2-7b-hf", 32000, 4096), ("Llama-3.1-8B", 128256, 4096), ("Qwen2.5-7B", 152064, 3584)]
ROTATION_BYTES = 600 << 20
EPS = 1e-5


def _graph(fn, copies):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in range(copies):
            fn(c)
    g.replay()
    torch.cuda.synchronize()
    return g


def _alternate(graphs, per_replay, rounds):
    """graphs: {leg: graph}; every round replays each leg once, in turn -> {leg: [us per unit, one value per round]}"""
    out = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if hasattr(g, "prepare"):
                g.prepare()
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / per_replay[k])
    return out


def _stats(us):
    return {"us": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}


def synthetic_lm8(n, k, gen):
    codes = torch.randint(0, 256, (n, k), dtype=torch.uint8, device=DEV, generator=gen)
    meta = torch.empty(n, k // 128, 2, dtype=torch.float16, device=DEV)
    meta[..., 0] = 0.25 / (math.sqrt(k) * 73.9)         # (unit-gain rows: codes uniform in 0 .. 255 have a standard deviation of 73.9)
    meta[..., 1] = 127.5
    return LM8Weights(codes, meta, (n, k))


def launch_leg(rounds):
    rows_out = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    for name, n, k in SHAPES:
        nbytes = {"fp16": n * k * 2, "8bit": n * k + n * (k // 128) * 4, "4bit": n * k // 2 + n * (k // 128) * 4}
        copies = {leg: max(2, -(-ROTATION_BYTES // b)) for leg, b in nbytes.items()}
        w16 = [(torch.randn(n, k, device=DEV, generator=gen) / math.sqrt(k)).to(torch.float16) for _ in range(copies["fp16"])]
        w8 = [synthetic_lm8(n, k, gen) for _ in range(copies["8bit"])]
        w4 = [_synthetic_linear(n, k, 4, gen, DEV) for _ in range(copies["4bit"])]
        gamma = (1.0 + 0.05 * torch.randn(k, device=DEV, generator=gen)).to(torch.float16)
        for R in (1, 4, 8):
            x = torch.randn(R, k, device=DEV, generator=gen).to(torch.float16)
            xin = x[0] if R == 1 else x
            y = torch.empty(R, n, dtype=torch.float16, device=DEV)
            yo = y[0] if R == 1 else y
            graphs = {
                "fp16": _graph(lambda c: ops.gemv_f16w(xin, w16[c], gamma=gamma, eps=EPS, out=yo), copies["fp16"]),
                "8bit": _graph(lambda c: ops.lm8_gemv(xin, w8[c], gamma=gamma, eps=EPS, out=yo), copies["8bit"]),
                "4bit": _graph(lambda c: ops.gemv_grouped(x, [w4[c].seg(y)], k, prologue=ops.PRO_RMSNORM, gamma=gamma, eps=EPS), copies["4bit"]),
            }
            us = _alternate(graphs, copies, rounds)
            rec = {"leg": "launch", "model": name, "N": n, "K": k, "rows": R}
            for leg in graphs:
                s = _stats(us[leg])
                rec[leg] = dict(s, bytes=nbytes[leg], gb_per_s=round(nbytes[leg] / s["us"] / 1e3, 1), copies=copies[leg])
            rec["8bit_faster_than_fp16_beyond_spread"] = rec["8bit"]["us_max"] < rec["fp16"]["us_min"]
            print(json.dumps(rec), flush=True)
            rows_out.append(rec)
            del graphs
        del w16, w8, w4
        torch.cuda.empty_cache()
    return rows_out


class _Steps:
    """`n` replays of a runner's captured token step, every round from the position behind its prompt (every step streams the whole model)"""

    def __init__(self, m, n):
        self.m, self.n, self.pos, self.tok = m, n, m.pos.clone(), m.token.clone()

    def prepare(self):
        self.m.pos.copy_(self.pos)
        self.m.set_token(self.tok)
        torch.cuda.synchronize()

    def replay(self):
        for _ in range(self.n):
            self.m.graph.replay()


def step_leg(rounds, steps):
    out = []
    for name, _, _ in SHAPES:
        cfg = arch_mod.MODEL_CONFIGS[name]
        pinned = arch_mod.PINNED_7B if name == "Llama-2-7b-hf" else ()
        linear = arch_mod.synthesize_arch(cfg, 3.0, seed=0, pinned=pinned)[0]["linear"]
        runners, graphs = {}, {}
        for bits in (16, 8, 4):
            m = QuantLlama(cfg, linear, device=DEV, max_seq=256, seed=0, lm_head_bits=bits)
            m.prefill(torch.randint(0, cfg["vocab_size"], (64,), generator=torch.Generator().manual_seed(1)))
            m.capture()
            runners[bits] = m
            graphs[bits] = _Steps(m, steps)
        for g in graphs.values():
            g.prepare()
            g.replay()
        torch.cuda.synchronize()
        us = _alternate(graphs, {b: steps for b in graphs}, rounds)
        rec = {"leg": "step", "model": name, "arch": "synthesized avg 3.0 bit, group 128", "context": 64, "steps_per_round": steps}
        for bits, m in runners.items():
            m.check()
            s = _stats(us[bits])
            rec[str(bits)] = dict(s, tokens_per_s=round(1e6 / s["us"], 1), lm_head_bytes=m.lm_head_bytes(), bytes_per_token=m.total_bytes_per_token(64))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del runners, graphs
        torch.cuda.empty_cache()
    return out


def drift_leg():
    out = []
    for name, n, k in SHAPES:
        gen = torch.Generator(device=DEV).manual_seed(7)
        W = (torch.randn(n, k, device=DEV, generator=gen) / math.sqrt(k)).to(torch.float16)
        gamma = (1.0 + 0.05 * torch.randn(k, device=DEV, generator=gen)).to(torch.float16)
        x = torch.randn(8, k, device=DEV, generator=gen).to(torch.float16)
        base = ops.gemv_f16w(x, W, gamma=gamma, eps=EPS).float()
        l8 = ops.lm8_gemv(x, quantize_lm8(W), gamma=gamma, eps=EPS).float()
        q4 = QuantLlama.pack_lm_head(W, 4)
        y4 = torch.empty(8, n, dtype=torch.float16, device=DEV)
        ops.gemv_grouped(x, [q4.seg(y4)], k, prologue=ops.PRO_RMSNORM, gamma=gamma, eps=EPS)
        top = float(base.abs().max())
        rec = {"leg": "drift", "model": name, "N": n, "K": k, "rows": 8, "weights": "synthetic Gaussian (not a checkpoint; not a perplexity)",
               "max_abs_logit": round(top, 4),
               "8bit_max_dlogit_over_max_logit": round(float((l8 - base).abs().max()) / top, 6),
               "4bit_max_dlogit_over_max_logit": round(float((y4.float() - base).abs().max()) / top, 6),
               "8bit_argmax_agree": int((l8.argmax(-1) == base.argmax(-1)).sum()), "4bit_argmax_agree": int((y4.float().argmax(-1) == base.argmax(-1)).sum())}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del W, q4
        torch.cuda.empty_cache()
    return out


def window_leg(rounds, rows=2048):
    name, n, k = SHAPES[1]
    gen = torch.Generator(device=DEV).manual_seed(3)
    W = (torch.randn(n, k, device=DEV, generator=gen) / math.sqrt(k)).to(torch.float16)
    w8 = quantize_lm8(W)
    gamma = (1.0 + 0.05 * torch.randn(k, device=DEV, generator=gen)).to(torch.float16)
    x = torch.randn(rows, k, device=DEV, generator=gen).to(torch.float16)
    out = torch.empty(rows, n, dtype=torch.float16, device=DEV)

    def f16(c):
        ops.gemm_f16w(ops.rmsnorm(x, gamma, EPS), W, out=out)

    def b8(c):
        for r0 in range(0, rows, 8):
            ops.lm8_gemv(x[r0:r0 + 8], w8, gamma=gamma, eps=EPS, out=out[r0:r0 + 8])

    scratch = torch.empty(QuantLlama.LM8_SLICE_ROWS, k, dtype=torch.float16, device=DEV)

    def b8s(c):                                         # what score_rows runs: pieces of SCORE_ROWS rows, the layer dequantized in slices for each
        for r0 in range(0, rows, QuantLlama.SCORE_ROWS):
            r1 = min(rows, r0 + QuantLlama.SCORE_ROWS)
            lm8_logits_sliced(ops.rmsnorm(x[r0:r1], gamma, EPS), w8, out[r0:r1], scratch)

    legs = {"fp16_gemm": _graph(f16, 1), "8bit_streamed": _graph(b8, 1), "8bit_sliced": _graph(b8s, 1)}
    us = _alternate(legs, {leg: 1 for leg in legs}, rounds)
    rec = {"leg": "scoring window", "model": name, "N": n, "K": k, "rows": rows, "piece_rows": QuantLlama.SCORE_ROWS,
           "slice_rows": QuantLlama.LM8_SLICE_ROWS,
           "fp16_gemm_ms": round(statistics.median(us["fp16_gemm"]) / 1e3, 2), "8bit_streamed_ms": round(statistics.median(us["8bit_streamed"]) / 1e3, 2),
           "8bit_sliced_ms": round(statistics.median(us["8bit_sliced"]) / 1e3, 2)}
    print(json.dumps(rec), flush=True)
    return [rec]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lm_head_bits.json"))
    p.add_argument("--only", default=None, choices=("window",))
    p.add_argument("--quick", action="store_true", help="fewer rounds (a rehearsal of the script, not a measurement)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lm_head_bits_bench.py measures on the GPU: none found")
    rounds = 3 if args.quick else 9
    res = {"device": torch.cuda.get_device_name(0), "method": "one process, legs alternating per round, hipGraph replay, HIP events; median (min, max) "
           "over the rounds; launch legs rotate > 600 MB of layer copies", "rounds": rounds}
    if args.only == "window":                           # (re-measure leg (iv) alone into an existing file)
        with open(args.out) as f:
            res = json.load(f)
        res["scoring_window"] = window_leg(3)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    res["launch"] = launch_leg(rounds)
    res["drift"] = drift_leg()
    res["scoring_window"] = window_leg(3)
    res["step"] = step_leg(rounds, 8 if args.quick else 32)
    big = [r for r in res["launch"] if r["rows"] == 1 and r["N"] > 100000]
    res["done_condition_R1_large_vocabularies"] = all(r["8bit_faster_than_fp16_beyond_spread"] for r in big)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out, "| R = 1 condition on the large vocabularies:", res["done_condition_R1_large_vocabularies"], flush=True)


if __name__ == "__main__":
    main()
