#!/usr/bin/env python3
"""The 8-bit KV cache against the fp16 cache, measured in ONE run -> profiles/kv8_attention.json.

  launch   per-launch time of ops.attn_decode (fp16 cache, auto policy) and ops.attn_decode_kv8 (auto policy) at (n_heads, n_kv_heads) in
           {(32, 32), (32, 8), (28, 4)} x {256, 2048, 4096, 16384, 32768} cached keys x batch {1, 8}: L layers' worth of distinct caches (at least
           1.5 GiB per leg, far beyond the 256 MiB Infinity Cache: every launch reads its rows from HBM), one launch per layer replayed from a
           hipGraph, HIP events around enough replays for >= 40 ms, the two legs alternating, median of the rounds; also as bytes of K + V read per
           second (256 / 132 bytes per row and its scale).
  step     whole-step tokens/s of the synthetic Llama-2-7B at an average of 3 bits, at 64 and at 4000 cached keys, kv_bits 16 and 8 (graph-replayed
           steps between two device synchronisations).
  drift    max |logit(kv_bits=8) - logit(kv_bits=16)| / max |logit| over 32 decode steps of the tiny test model and of the synthetic 7B, both runners
           fed the fp16 runner's tokens.  Synthetic weights: a recorded number, not a perplexity.

usage: kv8_attention_time.py [--out profiles/kv8_attention.json] [--part launch,step,drift] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from amq_amd import arch as arch_mod, ops  # noqa: E402
from amq_amd.llama import QuantLlama       # noqa: E402

HEADS = ((32, 32), (32, 8), (28, 4))
KEYS = (256, 2048, 4096, 16384, 32768)
BATCHES = (1, 8)
LEG_BYTES = 3 << 29            # distinct cache bytes per leg: 1.5 GiB
LEG_BYTES_MAX = 40 << 30       # a leg whose two layers would pass this is left out ("where memory allows")
DEV = torch.device("cuda:0")


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            fn()
    torch.cuda.current_stream(DEV).wait_stream(side)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    return g


def timed(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def launch_shape(nh, nkv, T, B, rounds):
    max_seq = T + 64
    row16, row8 = 2 * B * nkv * (T + 1) * 256, 2 * B * nkv * (T + 1) * 132          # K + V bytes one launch reads
    L = max(2, min(32, -(-LEG_BYTES // (2 * B * nkv * max_seq * 256))))
    if L * 2 * B * nkv * max_seq * 256 > LEG_BYTES_MAX:
        return dict(n_heads=nh, n_kv_heads=nkv, keys=T, batch=B, skipped="cache beyond the memory set aside")
    gen = torch.Generator(device=DEV).manual_seed(T + B)
    kc = [torch.randn(B, nkv, max_seq, 128, device=DEV, generator=gen).half() for _ in range(L)]
    vc = [torch.randn(B, nkv, max_seq, 128, device=DEV, generator=gen).half() for _ in range(L)]
    c8 = []
    for l in range(L):
        kc8, ks, vc8, vs = ops.kv8_alloc(B, nkv, max_seq, DEV)
        kc8.random_(-127, 128, generator=gen); vc8.random_(-127, 128, generator=gen)
        ks.uniform_(0.005, 0.03, generator=gen); vs.uniform_(0.005, 0.03, generator=gen)
        c8.append((kc8, ks, vc8, vs))
    q = torch.randn(B, nh * 128, device=DEV, generator=gen).half()
    k = torch.randn(B, nkv * 128, device=DEV, generator=gen).half()
    v = torch.randn(B, nkv * 128, device=DEV, generator=gen).half()
    out = torch.empty(B, nh * 128, device=DEV, dtype=torch.float16)
    cur, pos, err = ops.new_step_state(DEV)
    table = ops.rope_table(max_seq, 10000.0, DEV)
    cur.copy_(table.view(max_seq, 128)[T]); pos.fill_(T)

    def leg16():
        for l in range(L):
            ops.attn_decode(q, k, v, kc[l], vc[l], out, pos, nh, nkv, cur=cur)

    def leg8():
        for l in range(L):
            ops.attn_decode_kv8(q, k, v, *c8[l], out, pos, nh, nkv, cur=cur)

    g16, g8 = graph_of(leg16), graph_of(leg8)
    reps = max(3, int(0.04 / max(timed(g16, 2), 1e-6)) + 1)
    t16, t8 = [], []
    for _ in range(rounds):                                  # the legs alternate
        t16.append(timed(g16, reps) / L)
        t8.append(timed(g8, reps) / L)
    assert int(err.item()) == 0
    m16, m8 = statistics.median(t16), statistics.median(t8)
    return dict(n_heads=nh, n_kv_heads=nkv, keys=T, batch=B, layers=L, replays=reps, rounds=rounds,
                fp16_us=round(m16 * 1e6, 2), kv8_us=round(m8 * 1e6, 2), kv8_over_fp16=round(m8 / m16, 3),
                fp16_us_rounds=[round(t * 1e6, 2) for t in t16], kv8_us_rounds=[round(t * 1e6, 2) for t in t8],
                fp16_read_gbps=round(row16 / m16 / 1e9, 1), kv8_read_gbps=round(row8 / m8 / 1e9, 1),
                fp16_splits=ops.attn_decode_splits(max_seq, nh, B, nkv), kv8_splits=ops.attn_decode_kv8_splits(max_seq, nh, B, nkv))


def synthetic_7b(max_seq, kv_bits):
    cfg = arch_mod.MODEL_CONFIGS["Llama-2-7b-hf"]
    linear = arch_mod.synthesize_arch(cfg, 3.0, seed=0, pinned=arch_mod.PINNED_7B)[0]["linear"]
    return QuantLlama(cfg, linear, device="cuda:0", max_seq=max_seq, seed=0, kv_bits=kv_bits)


def step_rate(keys, steps=64, rounds=3):
    res = {}
    ids = torch.randint(0, 31999, (keys,), generator=torch.Generator().manual_seed(keys)).to(DEV)
    models = {kb: synthetic_7b(keys + 4 * steps + 32, kb) for kb in (16, 8)}
    rates = {16: [], 8: []}
    for _ in range(rounds):
        for kb, m in models.items():                         # the two runners alternate
            m.reset()
            m.prefill(ids)
            for _ in range(4):
                m.decode_step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                m.decode_step()
            torch.cuda.synchronize()
            rates[kb].append(steps / (time.perf_counter() - t0))
            m.check()
    for kb in (16, 8):
        res[f"kv{kb}_tokens_per_s"] = round(statistics.median(rates[kb]), 1)
        res[f"kv{kb}_rounds"] = [round(r, 1) for r in rates[kb]]
        res[f"kv{kb}_kv_gb_per_token"] = round((models[kb].total_bytes_per_token(keys) - models[kb].total_bytes_per_token(0)) / 1e9, 3)
    res.update(keys=keys, steps=steps, model="Llama-2-7b-hf, synthetic weights, 3.0 bits on average")
    return res


def drift(m16, m8, prompt, steps=32):
    worst = 0.0
    a, b = m16.prefill(prompt).clone(), m8.prefill(prompt).clone()
    prompt_equal = bool(torch.equal(a, b))
    for _ in range(steps):
        m8.set_token(m16.token)                              # both runners decode the fp16 runner's tokens
        m16.decode_step()
        m8.decode_step()
        a, b = m16.logits.float().view(-1), m8.logits.float().view(-1)
        worst = max(worst, float((a - b).abs().max() / a.abs().max()))
    m16.check(); m8.check()
    return dict(steps=steps, prompt=int(prompt.numel()), prompt_logits_equal=prompt_equal, max_dlogit_over_max_logit=float(f"{worst:.3e}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kv8_attention.json"))
    ap.add_argument("--part", default="launch,step,drift")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    parts = args.part.split(",")
    res = dict(device=torch.cuda.get_device_name(0), method=__doc__.split("usage:")[0].strip())

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    if "launch" in parts:
        res["launch"] = []
        for nh, nkv in HEADS:
            for T in KEYS:
                for B in BATCHES:
                    r = launch_shape(nh, nkv, T, B, args.rounds)
                    res["launch"].append(r)
                    print(json.dumps(r), flush=True)
                    torch.cuda.empty_cache()
                    save()
    if "step" in parts:
        res["step"] = []
        for keys in (64, 4000):
            r = step_rate(keys, rounds=args.rounds)
            res["step"].append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
            save()
    if "drift" in parts:
        cfg = dict(arch_mod._cfg(2, 512, 1024, 4, 2, 1, vocab=1024))
        tiny = [QuantLlama(cfg, None, device="cuda:0", max_seq=128, seed=3, kv_bits=kb) for kb in (16, 8)]
        p = torch.randint(0, 1024, (24,), generator=torch.Generator().manual_seed(1)).to(DEV)
        res["drift"] = dict(tiny=drift(tiny[0], tiny[1], p))
        big = [synthetic_7b(256, kb) for kb in (16, 8)]
        p = torch.randint(0, 31999, (64,), generator=torch.Generator().manual_seed(2)).to(DEV)
        res["drift"]["synthetic_7b"] = drift(big[0], big[1], p)
        res["drift"]["note"] = "synthetic weights: a recorded number, not a perplexity"
        print(json.dumps(res["drift"]), flush=True)
        save()
    save()


if __name__ == "__main__":
    main()
