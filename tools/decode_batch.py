#!/usr/bin/env python3
"""decode throughput against the batch (graph replay, 64-token prompts, Llama-2-7B avg-3 synthetic weights): sequences per step
share one pass over the weights.  usage: decode_batch.py [--ragged | --ragged=spread] [batches, comma separated] [steps]
--ragged: the runner with a position per sequence (QuantLlama(ragged=True)) at equal 64-token prompts -- the same work as the plain step, so the
difference is what the per-sequence step state costs; --ragged=spread: prompt lengths spread evenly over 16 .. 256 (right-padded to 256).
(NORM_SUMS=0: the 5 .. 8-row steps with one rmsnorm launch per norm instead of the partial-sum RMSNorm, A/B)"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from amq_amd import arch, ops
from amq_amd.llama import QuantLlama
if os.environ.get("GEMV_WAVES") or os.environ.get("GEMV_DEPTH") or os.environ.get("GEMV_DOT"):
    ops.DEFAULT_GEMV_OPTS = ops.GemvOpts(waves=int(os.environ.get("GEMV_WAVES", "0")), depth=int(os.environ.get("GEMV_DEPTH", "0")),
                                         dot=int(os.environ.get("GEMV_DOT", "0")))   # A/B: waves per workgroup, ring depth, v_dot2 body at one row

if os.environ.get("NORM_SUMS") == "0":
    QuantLlama.NORM_SUMS = False
ragged = next((v for v in sys.argv[1:] if v.startswith("--ragged")), None)
argv = [v for v in sys.argv[1:] if not v.startswith("--")]
batches = [int(v) for v in (argv[0].split(",") if len(argv) > 0 else "1,2,4,8".split(","))]
steps = int(argv[1]) if len(argv) > 1 else 128
spread = ragged == "--ragged=spread"
S = 256 if spread else 64
name = os.environ.get("SWEEP_MODEL", "Llama-2-7b-hf")
dev = torch.device("cuda:0")
cfg = arch.MODEL_CONFIGS[name]
a, usage = arch.synthesize_arch(cfg, 3.0, seed=0, pinned=arch.PINNED_7B if "7b" in name else ())
for B in batches:
    m = QuantLlama(cfg, a["linear"], device=dev, max_seq=S + steps + 24, seed=0, batch=B, ragged=ragged is not None)
    ids = torch.randint(0, m.vocab - 1, (B, S), generator=torch.Generator().manual_seed(0)).to(dev)
    if ragged is not None:
        lengths = [16 + (240 * b) // max(1, B - 1) for b in range(B)] if spread else [S] * B
        m.prefill(ids, use_graph=False, lengths=lengths)
    else:
        m.prefill(ids if B > 1 else ids[0], use_graph=False)
    m.capture()
    for _ in range(8):
        m.decode_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.decode_step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    m.check()
    tag = "" if ragged is None else (f" ragged, lengths {lengths[0]} .. {lengths[-1]}")
    print(f"{name} batch {B}{tag}: {dt*1e3:.3f} ms/step  {1/dt:7.1f} steps/s  {B/dt:8.1f} tokens/s aggregate", flush=True)
    del m
    torch.cuda.empty_cache()
