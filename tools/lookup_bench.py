"""What a prompt-lookup verify step costs and gains: the captured step over R = D + 1 rows of one sequence (rows attention + verify-and-propose tail)
against the plain one-row step of the same process and the batched step at B = R (tools/decode_batch.py), on the 7B avg-3 synthetic model bench.py
uses, 64-token prompt.

    python tools/lookup_bench.py [--rows 2,3,4,5,6,7,8] [--steps 128] [--repeats 3] [--parent DIR] [--out profiles/lookup_decode.json]

Acceptance is PLANTED with external drafts.  Per R the lookup runner itself first records a never-accepting run (every draft a suppressed id): its
tokens are the greedy decode of the R-row arithmetic, the only sequence whose continuations this runner accepts.  Then, per step, the first ``a``
drafts are taken from that record and the rest are the suppressed id, for a = 0 .. R - 1: the table does not depend on what a random-weight model
happens to emit, and ``tokens_per_step`` (read from the device counters) must come out as a + 1.  The drafts of every step are staged on the device
beforehand; a timed step is the captured graph plus the one set_token launch and the small state copy that hand it the drafts (their cost is part
of the figure; the "lookup" leg, where the tail proposes on the device, has neither).  The plain one-row step is timed in the same process, the
legs alternate over ``--repeats`` rounds and the spread is recorded.  break_even_acceptance = t_R / t_1 - 1: the mean number of accepted drafts
per step from which the verify step wins.  The batched step at B = R is measured by tools/decode_batch.py in a child process.
``--parent DIR``: a built checkout of the parent commit; its plain step (bench.py --gpus 1 --steps 256 --warmup 16) and its batched steps
(tools/decode_batch.py) are run there as child processes, in the same session on the same box, and recorded under "parent".

    python tools/lookup_bench.py --sampled [--drafts 3,7] [--steps 128] [--repeats 5] [--out profiles/lookup_sample.json]

The SAMPLED verify step (QuantLlama(lookup=D, lookup_sampling=True) after set_sampling: the tail draws every row's token) against the greedy verify
step of the same runner -- two captured graphs of one process, replayed alternately, the tail proposing on the device in both -- on the 7B avg-3
synthetic models with vocabulary 32000 (Llama-2-7b-hf) and 152064 (Qwen2.5-7B), and, per model, the plain one-row sampled step against the plain
one-row greedy step in that process (the surcharge tools/sampling_bench.py measures).  The greedy verify step's launches are the parent commit's."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SUP = 5
PROMPT = 64


def _build(dev, max_seq, **kw):
    import bench
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = arch.MODEL_CONFIGS[bench.MODEL]
    a, _ = arch.synthesize_arch(cfg, bench.TARGET_BITS, seed=0, pinned=arch.PINNED_7B)
    return QuantLlama(cfg, a["linear"], device=dev, max_seq=max_seq, seed=0, **kw)


def _timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def _med(ts):
    return dict(ms=statistics.median(ts), runs=[round(t, 5) for t in ts], spread_pct=100.0 * (max(ts) - min(ts)) / statistics.median(ts))


def _child(args, cwd, limit):
    """a fresh child process (its own GPU context), output returned; a failure is an error of the tool"""
    r = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(args)} in {cwd} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def batched_steps(cwd, rows, steps):
    """ms per step at B = rows through tools/decode_batch.py (child process in ``cwd``)"""
    out = _child([os.path.join("tools", "decode_batch.py"), ",".join(str(r) for r in rows), str(steps)], cwd, 900)
    got = {int(b): float(ms) for b, ms in re.findall(r"batch (\d+): ([0-9.]+) ms/step", out)}
    assert sorted(got) == sorted(rows), out
    return got


def parent_plain(cwd):
    out = _child(["bench.py", "--gpus", "1", "--steps", "256", "--warmup", "16"], cwd, 900)
    line = [l for l in out.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def verify_rows(dev, R, plain, ids, steps, repeats):
    """the verify step at R rows for planted acceptance 0 .. R - 1 and with the tail's own proposals, the plain step alternating with every leg"""
    from amq_amd import ops
    D = R - 1
    m = _build(dev, PROMPT + 16 + steps * R + R, lookup=D)
    m.set_suppressed([SUP])
    tin = torch.zeros(R, dtype=torch.int64, device=dev)

    def run(dr, dr32, n_steps):
        def step(i):
            tin[:1].copy_(m.token[:1])
            tin[1:].copy_(dr[i])
            ops.set_token(tin, m.embed, m.token, m.pos, m.x, table=m.rope_tab, cur=m.rope_cur)
            m.lookup_state[ops.LOOKUP_DRAFT + 1:ops.LOOKUP_DRAFT + 1 + D].copy_(dr32[i])
            m.graph.replay()
        m.reset()
        m.set_lookup_mode(True)
        m.prefill(ids)
        m.capture()
        t = _timed(step, n_steps)
        count, st = m.lookup_sync()
        return t, (count - PROMPT - 1) / st

    def plain_leg():
        plain.prefill(ids)
        plain.capture()
        return _timed(lambda i: plain.graph.replay(), steps)

    # the record: never accepted = one token per step = the greedy decode of THIS runner's arithmetic
    never = torch.full((steps * R + R, D), SUP, dtype=torch.int64, device=dev)
    run(never, never.to(torch.int32), steps * R + R - 1)
    ref = m.lookup_tokens().cpu()
    res, plain_ts = {}, []
    for a in range(R):
        n_steps = min(steps, (ref.numel() - 1 - D) // (a + 1))
        dr = torch.full((n_steps, D), SUP, dtype=torch.int64)
        for i in range(n_steps):                        # row 0 of step i computes token index e = 1 + i (a + 1); rows 1 .. a run ref[e .. e + a - 1]
            e = 1 + i * (a + 1)
            dr[i, :a] = ref[e:e + a]
        dr = dr.to(dev)
        dr32 = dr.to(torch.int32)
        ts, emitted = [], None
        for rep in range(repeats + 1):                  # (the first round warms up: not kept)
            t, emitted = run(dr, dr32, n_steps)
            tp = plain_leg()
            if rep:
                ts.append(t)
                plain_ts.append(tp)
        r = _med(ts)
        r.update(steps=n_steps, planted=a, tokens_per_step=emitted, tokens_per_s=1e3 * emitted / r["ms"])
        res[str(a)] = r
    ts = []
    for rep in range(repeats + 1):                      # the tail proposing on the device (no host hand-over): the product path's step time
        m.reset()
        m.set_lookup_mode(False)
        m.prefill(ids)
        m.capture()
        t = _timed(lambda i: m.graph.replay(), steps)
        count, st = m.lookup_sync()
        tp = plain_leg()
        if rep:
            ts.append(t)
            plain_ts.append(tp)
    m.check()
    res["lookup"] = dict(_med(ts), tokens_per_step=(count - PROMPT - 1) / st)
    del m
    torch.cuda.empty_cache()
    return res, plain_ts


SAMPLED_MODELS = ("Llama-2-7b-hf", "Qwen2.5-7B")      # vocabulary 32000 / 152064
SAMPLER = dict(temperature=0.8, top_k=50, top_p=0.9, seed=1)


def _build_model(dev, model, max_seq, **kw):
    import bench
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = arch.MODEL_CONFIGS[model]
    a, _ = arch.synthesize_arch(cfg, bench.TARGET_BITS, seed=0, pinned=arch.PINNED_7B if model == bench.MODEL else ())
    return QuantLlama(cfg, a["linear"], device=dev, max_seq=max_seq, seed=0, **kw)


def _alternate(m, ids, steps, repeats):
    """greedy and sampled captured steps of runner ``m`` replayed alternately: -> {leg: median / runs / spread}, sampled_over_greedy_pct"""
    legs = {"greedy": [], "sampled": []}
    per_step = {}
    for rep in range(repeats + 1):                      # (the first round captures and warms up: not kept)
        for leg in legs:
            m.set_sampling(**SAMPLER) if leg == "sampled" else m.set_sampling(None)
            m.reset()
            m.prefill(ids)
            m.capture(leg == "sampled")
            g = m.sample_graph if leg == "sampled" else m.graph
            t = _timed(lambda i: g.replay(), steps)
            if m.lookup:
                count, st = m.lookup_sync()
                per_step[leg] = (count - ids.numel() - 1) / st
            if rep:
                legs[leg].append(t)
    m.set_sampling(None)
    m.check()
    res = {leg: _med(ts) for leg, ts in legs.items()}
    for leg, v in per_step.items():
        res[leg]["tokens_per_step"] = v
    res["sampled_over_greedy_pct"] = 100.0 * (res["sampled"]["ms"] / res["greedy"]["ms"] - 1.0)
    return res


def sampled_main(a):
    dev = torch.device("cuda:0")
    drafts = [int(d) for d in a.drafts.split(",") if d]
    res = {"sampler": SAMPLER, "prompt": PROMPT, "steps": a.steps, "repeats": a.repeats, "models": {}}
    for model in SAMPLED_MODELS:
        plain = _build_model(dev, model, PROMPT + 16 + a.steps)
        ids = torch.randint(8, plain.vocab, (PROMPT,), generator=torch.Generator().manual_seed(0)).to(dev)
        entry = {"vocab": plain.vocab, "plain_step": _alternate(plain, ids, a.steps, a.repeats), "verify": {}}
        del plain
        torch.cuda.empty_cache()
        for D in drafts:
            R = D + 1
            m = _build_model(dev, model, PROMPT + 16 + a.steps * R + R, lookup=D, lookup_sampling=True)
            v = _alternate(m, ids, a.steps, a.repeats)
            # the same sampler on R rows side by side instead of one: what the tail adds, beside what the one-row sampled step adds
            v["sampled_minus_greedy_us"] = 1e3 * (v["sampled"]["ms"] - v["greedy"]["ms"])
            v["plain_sampled_minus_greedy_us"] = 1e3 * (entry["plain_step"]["sampled"]["ms"] - entry["plain_step"]["greedy"]["ms"])
            entry["verify"][str(D)] = v
            del m
            torch.cuda.empty_cache()
        res["models"][model] = entry
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="2,3,4,5,6,7,8")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sampled", action="store_true", help="the sampled verify step against the greedy one (see the module docstring)")
    ap.add_argument("--drafts", default="3,7")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.sampled:
        return sampled_main(a)
    dev = torch.device("cuda:0")
    rows = [int(r) for r in a.rows.split(",") if r]
    ids = torch.randint(8, 32000, (PROMPT,), generator=torch.Generator().manual_seed(0)).to(dev)
    plain = _build(dev, PROMPT + 16 + a.steps)
    plain.set_suppressed([SUP])
    res = {"model": "Llama-2-7b-hf avg-3 synthetic", "prompt": PROMPT, "steps": a.steps, "repeats": a.repeats, "rows": {}}
    plain_all = []
    for R in rows:
        lk, pts = verify_rows(dev, R, plain, ids, a.steps, a.repeats)
        plain_all += pts
        res["rows"][str(R)] = dict(verify=lk)
    res["plain_step"] = _med(plain_all)
    del plain
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    batched = batched_steps(ROOT, rows, a.steps)
    for R in rows:
        e = res["rows"][str(R)]
        t_r = e["verify"]["lookup"]["ms"]
        e["batched_step_ms"] = batched[R]
        e["break_even_acceptance"] = t_r / res["plain_step"]["ms"] - 1.0
        e["overhead_over_batched_pct"] = 100.0 * (t_r / batched[R] - 1.0)
    if a.parent:
        pb = batched_steps(a.parent, [1] + rows, a.steps)
        pl = parent_plain(a.parent)
        res["parent"] = dict(batched_step_ms={str(k): v for k, v in pb.items()}, bench=pl)
        for R in rows:
            res["rows"][str(R)]["overhead_over_parent_batched_pct"] = 100.0 * (res["rows"][str(R)]["verify"]["lookup"]["ms"] / pb[R] - 1.0)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
