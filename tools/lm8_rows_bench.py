#!/usr/bin/env python3
"""The 8-bit lm_head's tiled many-row kernel (ops.lm8_gemm_rows, QuantLlama(lm8_kernel="tiled")) against the routes the runner takes
without it, all legs in ONE process, alternating, hipGraph replay, HIP events, every launch of a graph on its own copy of the layer (> 600 MB in
rotation: cold in HBM) -- the method of lm_head_bits_bench.py, whose helpers this imports:

  (i)  many-row logits at M = 17, 32, 63, 64, 128, 512, 2048 rows and the three vocabularies: "tiled" (ops.rmsnorm + ops.lm8_gemm_rows), the
       routes of the same call without it -- below 64 rows the 8-row ops.lm8_gemv pieces ("dot") and the 16-row ops.lm8_gemm pieces ("mfma"), from
       64 rows on the dequantized slices (lm8_logits_sliced behind ops.rmsnorm) -- and "fp16" (ops.rmsnorm + ops.gemm_f16w over an fp16 lm_head);
  (ii) two whole paths of the synthetic avg-3-bit Llama-3.1-8B shape at lm_head_bits=8, lm8_kernel "dot" against "tiled": score_rows of a
       2048-token window, and a 64-row prompt pass that forms all-row logits.

usage: lm8_rows_bench.py [--out profiles/lm8_gemm_rows.json] [--quick] [--only launch | paths]"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lm_head_bits_bench import DEV, EPS, ROTATION_BYTES, SHAPES, _alternate, _graph, _stats, synthetic_lm8  # noqa: E402
from amq_amd import arch as arch_mod  # noqa: E402
from amq_amd import ops  # noqa: E402
from amq_amd.llama import QuantLlama, lm8_logits_sliced  # noqa: E402

ROWS = (17, 32, 63, 64, 128, 512, 2048)


def _verdict(rec, leg, other):
    """ahead or behind by more than the spread of the rounds, else "level\""""
    return "ahead" if rec[leg]["us_max"] < rec[other]["us_min"] else "behind" if rec[leg]["us_min"] > rec[other]["us_max"] else "level"


def launch_leg(rounds, shapes, rows):
    out = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    for name, n, k in shapes:
        c16, c8 = max(2, -(-ROTATION_BYTES // (n * k * 2))), max(2, -(-ROTATION_BYTES // (n * k)))
        w16 = [(torch.randn(n, k, device=DEV, generator=gen) / math.sqrt(k)).to(torch.float16) for _ in range(c16)]
        w8 = [synthetic_lm8(n, k, gen) for _ in range(c8)]
        gamma = (1.0 + 0.05 * torch.randn(k, device=DEV, generator=gen)).to(torch.float16)
        scratch = torch.empty(min(QuantLlama.LM8_SLICE_ROWS, n), k, dtype=torch.float16, device=DEV)
        for M in rows:
            x = torch.randn(M, k, device=DEV, generator=gen).to(torch.float16)
            y = torch.empty(M, n, dtype=torch.float16, device=DEV)

            def pieces(op, step):
                def fn(c):
                    for r0 in range(0, M, step):
                        r1 = min(M, r0 + step)
                        (ops.lm8_gemv if r1 - r0 == 1 else op)(x[r0] if r1 - r0 == 1 else x[r0:r1], w8[c], gamma=gamma, eps=EPS,
                                                              out=y[r0] if r1 - r0 == 1 else y[r0:r1])
                return fn

            legs = {"tiled": (lambda c: ops.lm8_gemm_rows(ops.rmsnorm(x, gamma, EPS), w8[c], out=y), c8),
                    "fp16": (lambda c: ops.gemm_f16w(ops.rmsnorm(x, gamma, EPS), w16[c], out=y), c16)}
            if M < QuantLlama.LM8_SLICED_FROM:
                legs["dot_pieces"] = (pieces(ops.lm8_gemv, 8), c8)
                legs["mfma_pieces"] = (pieces(ops.lm8_gemm, 16), c8)
            else:
                legs["sliced"] = (lambda c: lm8_logits_sliced(ops.rmsnorm(x, gamma, EPS), w8[c], y, scratch), c8)
            graphs = {leg: _graph(fn, c) for leg, (fn, c) in legs.items()}
            us = _alternate(graphs, {leg: c for leg, (_, c) in legs.items()}, rounds)
            rec = {"leg": "launch", "model": name, "N": n, "K": k, "rows": M}
            for leg in graphs:
                rec[leg] = _stats(us[leg])
            for other in graphs:
                if other != "tiled":
                    rec["tiled_vs_" + other] = _verdict(rec, "tiled", other)
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del graphs
        del w16, w8, scratch
        torch.cuda.empty_cache()
    return out


class _Eager:
    """a leg that is no graph of its own (score_rows, a prompt pass through its captured graph): _alternate times one call"""

    def __init__(self, fn):
        self.replay = fn


def paths_leg(rounds):
    name = SHAPES[1][0]
    cfg = arch_mod.MODEL_CONFIGS[name]
    linear = arch_mod.synthesize_arch(cfg, 3.0, seed=0)[0]["linear"]
    runners, packed = {}, None
    for kernel in ("dot", "tiled"):
        m = QuantLlama(cfg, linear, device=DEV, max_seq=2048, seed=0, lm_head_bits=8, lm_head_packed=packed, lm8_kernel=kernel)
        m.all_logits = True
        packed = runners.setdefault(kernel, m).lm_head_q
    out = []
    gen = torch.Generator().manual_seed(1)
    for what, S, call in (("score_rows, one 2048-token window", 2048, lambda m, ids: m.score_rows(ids)),
                          ("all-logits prompt pass, 64 rows", 64, lambda m, ids: m.prefill(ids))):
        ids = torch.randint(0, cfg["vocab_size"], (S,), generator=gen).to(DEV)
        legs = {k: _Eager(lambda m=m: call(m, ids)) for k, m in runners.items()}
        for g in legs.values():
            g.replay()
        torch.cuda.synchronize()
        us = _alternate(legs, {k: 1 for k in legs}, rounds)
        rec = {"leg": "path", "model": name, "arch": "synthesized avg 3.0 bit, group 128", "what": what}
        for k in legs:
            rec[k] = _stats(us[k])
        rec["tiled_vs_dot"] = _verdict(rec, "tiled", "dot")
        rec["lm8_scratch_bytes"] = {k: 0 if m._lm8_scratch is None else m._lm8_scratch.numel() * 2 for k, m in runners.items()}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lm8_gemm_rows.json"))
    p.add_argument("--only", default=None, choices=("launch", "paths"))
    p.add_argument("--quick", action="store_true", help="fewer rounds, one shape, three row counts (a rehearsal of the script, not a measurement)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lm8_rows_bench.py measures on the GPU: none found")
    rounds = 3 if args.quick else 7
    res = {"device": torch.cuda.get_device_name(0), "method": "one process, legs alternating per round, hipGraph replay (paths: eager calls), HIP "
           "events; median (min, max) over the rounds; launch legs rotate > 600 MB of layer copies", "rounds": rounds,
           "tile": {"BM": ops.LM8_ROWS_BM, "BN": 256, "waves": 4, "instruction": "v_mfma_f32_32x32x16_f16"}}
    if args.only != "paths":
        res["launch"] = launch_leg(rounds, SHAPES[1:2] if args.quick else SHAPES, (17, 64, 512) if args.quick else ROWS)
    if args.only != "launch":
        res["paths"] = paths_leg(rounds)
    res["not_measured"] = "a real checkpoint, perplexity, counters"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
