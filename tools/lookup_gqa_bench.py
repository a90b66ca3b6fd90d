"""The rows attention of a prompt-lookup verify step on grouped-query models: the per-head split kernel (ops.attn_decode_rows(grouped=False)) against
the matrix-core kernel (grouped=True, amq_attn_decode_rows_gqa_f16).

    python tools/lookup_gqa_bench.py [--part launch,step] [--nbw2 amq_amd/libamq_hip_nbw2.so] [--out profiles/lookup_gqa.json]

(a) per launch: L layers' worth of distinct K / V caches (HBM-cold: together far beyond the 256 MiB Infinity Cache), one launch per layer replayed
    from a hipGraph, HIP events; 32/8, 28/4 and 64/8 heads x 2048 / 8192 / 32768 rows of cache (the step sits 48 rows from its end) x R = 2, 4, 8.
    The legs -- per-head, grouped at the policy's split count, at half and at twice that count, and (``--nbw2``: a build with -DAMQ_GQA_ROWS_NBW=2,
    `make -C amq_amd/csrc tuvariant TU=amq_attn_prefill TAG=nbw2 EXTRA="-DAMQ_GQA_ROWS_NBW=2 -mllvm -amdgpu-mfma-vgpr-form"`) two row blocks per
    workgroup instead of one block per grid row -- alternate in ONE process over 5 rounds: median and spread per leg.
(b) whole step: the Llama-3.1-8B shape (avg-3 synthetic), max_seq 8192, a 7900-token prompt, D = 3 and 7, external drafts that are never accepted
    (one token per step: the step time alone), the captured step with QuantLlama.ROWS_GQA_FROM = None and = 2048 alternating over 5 rounds.
"from": the smallest measured cache length from which grouped wins at every measured (heads, R) by more than the recorded spread, at that length
and every longer one (floor 2048; null: nowhere)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HEADS = [(32, 8), (28, 4), (64, 8)]
CACHES = [2048, 8192, 32768]
ROWS = [2, 4, 8]
ROUNDS, REPS = 5, 5
SUP = 5


def _med(ts):
    return dict(us=round(statistics.median(ts), 3), runs=[round(t, 3) for t in ts], spread_pct=round(100.0 * (max(ts) - min(ts)) / statistics.median(ts), 2))


def _graph(dev, fn):
    """fn's launches as a hipGraph (warmed up on the capturing stream first: its scratch pools are per stream)"""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(gr, stream=side):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    gr.replay()
    torch.cuda.synchronize()
    return gr


def _time_graph(gr, per):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS / per


def per_launch(dev, nbw2):
    from amq_amd import _lib, ops
    res = []
    for nh, nkv in HEADS:
        for max_seq in CACHES:
            p = max_seq - 48
            layer_bytes = 2 * nkv * max_seq * 256
            L = max(4, min(160, -(-(768 << 20) // layer_bytes)))
            g = torch.Generator(device=dev).manual_seed(0)
            kc = [torch.randn(1, nkv, max_seq, 128, device=dev, generator=g).half() for _ in range(L)]
            vc = [torch.randn(1, nkv, max_seq, 128, device=dev, generator=g).half() for _ in range(L)]
            table = ops.rope_table(max_seq, 10000.0, dev)
            for R in ROWS:
                q = torch.randn(R, nh * 128, device=dev, generator=g).half()
                k = torch.randn(R, nkv * 128, device=dev, generator=g).half()
                v = torch.randn(R, nkv * 128, device=dev, generator=g).half()
                out = torch.empty(R, nh * 128, device=dev, dtype=torch.float16)
                cur, pos, err = ops.new_step_state(dev, batch=R)
                pos.copy_(torch.arange(p, p + R, dtype=torch.int32))
                cur.copy_(table.view(max_seq, 128)[p:p + R])
                ns = ops.attn_decode_splits(max_seq, nh, ops.attn_rows_gqa_blocks(R, nh, nkv), nkv)

                def leg(grouped, n_splits, lib=None):
                    def launches():
                        for l in range(L):
                            ops.attn_decode_rows(q, k, v, kc[l], vc[l], out, cur, pos, nh, nkv, n_splits=n_splits, grouped=grouped)
                    if lib is None:
                        return _graph(dev, launches)
                    with _lib.routed_to(lib):
                        return _graph(dev, launches)
                legs = {"per_head": leg(False, 0), f"grouped_splits_{ns}": leg(True, ns)}
                for other in (max(1, ns // 2), min(1024, ns * 2)):
                    if other != ns:
                        legs[f"grouped_splits_{other}"] = leg(True, other)
                if nbw2 is not None:
                    legs[f"grouped_2_blocks_per_workgroup_splits_{ns}"] = leg(True, ns, nbw2)
                ts = {name: [] for name in legs}
                for rnd in range(ROUNDS + 1):               # (the first round warms up: not kept)
                    for name, gr in legs.items():
                        t = _time_graph(gr, L)
                        if rnd:
                            ts[name].append(t)
                assert err.tolist() == [0] * R
                row = dict(heads=[nh, nkv], max_seq=max_seq, p=p, rows=R, layers=L, policy_splits=ns,
                           row_blocks=ops.attn_rows_gqa_blocks(R, nh, nkv), legs={name: _med(t) for name, t in ts.items()})
                a, b = row["legs"]["per_head"], row["legs"][f"grouped_splits_{ns}"]
                row["grouped_over_per_head"] = round(b["us"] / a["us"], 4)
                row["grouped_wins_beyond_spread"] = max(b["runs"]) < min(a["runs"])
                print(json.dumps(row), flush=True)
                res.append(row)
            del kc, vc
            torch.cuda.empty_cache()
    return res


def whole_step(dev, steps=40, prompt=7900, max_seq=8192):
    from amq_amd import arch, ops
    from amq_amd.llama import QuantLlama
    cfg = arch.MODEL_CONFIGS["Llama-3.1-8B"]
    a, _ = arch.synthesize_arch(cfg, 3.0, seed=0)
    ids = torch.randint(8, 32000, (prompt,), generator=torch.Generator().manual_seed(0)).to(dev)
    res = []
    for D in (3, 7):
        R = D + 1
        m = QuantLlama(cfg, a["linear"], device=dev, max_seq=max_seq, seed=0, lookup=D)
        m.set_suppressed([SUP])
        m.set_lookup_mode(True)
        graphs = {}
        for name, frm in (("per_head", None), ("grouped", 2048)):
            QuantLlama.ROWS_GQA_FROM = frm
            m.reset()
            m.prefill(ids)
            m.graph = None
            m.capture()
            graphs[name] = m.graph
        tin = torch.zeros(R, dtype=torch.int64, device=dev)
        tin[1:].fill_(SUP)
        never = torch.full((D,), SUP, dtype=torch.int32, device=dev)

        def run(gr):
            m.reset()
            m.prefill(ids)

            def step():
                tin[:1].copy_(m.token[:1])
                ops.set_token(tin, m.embed, m.token, m.pos, m.x, table=m.rope_tab, cur=m.rope_cur)
                m.lookup_state[ops.LOOKUP_DRAFT + 1:ops.LOOKUP_DRAFT + 1 + D].copy_(never)
                gr.replay()
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) / steps * 1e6
            count, st = m.lookup_sync()
            assert count - prompt - 1 == st == steps + 1, (count, st)     # never accepted: one token per step
            m.check()
            return t
        ts = {name: [] for name in graphs}
        for rnd in range(ROUNDS + 1):
            for name, gr in graphs.items():
                t = run(gr)
                if rnd:
                    ts[name].append(t)
        row = dict(model="Llama-3.1-8B avg-3 synthetic", max_seq=max_seq, cached_keys=prompt, drafts=D, steps=steps,
                   legs={name: _med(t) for name, t in ts.items()})
        row["grouped_over_per_head"] = round(row["legs"]["grouped"]["us"] / row["legs"]["per_head"]["us"], 4)
        print(json.dumps(row), flush=True)
        res.append(row)
        del m, graphs
        torch.cuda.empty_cache()
    return res


def rows_gqa_from(launch):
    """the smallest measured cache length from which grouped wins beyond the spread at every (heads, R), there and at every longer length"""
    best = None
    for max_seq in sorted(CACHES, reverse=True):
        if all(r["grouped_wins_beyond_spread"] for r in launch if r["max_seq"] == max_seq):
            best = max_seq
        else:
            break
    return None if best is None else max(2048, best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="launch,step")
    ap.add_argument("--nbw2", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    from amq_amd import _lib
    from amq_amd.llama import QuantLlama
    res = dict(rounds=ROUNDS, replays_per_round=REPS, rows_gqa_from_in_tree=QuantLlama.ROWS_GQA_FROM)
    parts = a.part.split(",")
    if "launch" in parts:
        res["per_launch_us"] = per_launch(dev, _lib.open_twin(a.nbw2) if a.nbw2 else None)
        res["from"] = rows_gqa_from(res["per_launch_us"])
    if "step" in parts:
        res["whole_step_us"] = whole_step(dev)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
