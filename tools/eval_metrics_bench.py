"""What scoring a window costs: perplexity / JSD rows of one 2048-token window on synthetic 7B avg-3-bit runners (Llama-2-7B shapes at vocab 32000,
Qwen2.5-7B shapes at vocab 152064), milliseconds and peak allocated bytes of

  (a) pass          the prompt pass alone (QuantLlama._rows_pass, no KV cache, no logits);
  (b) score_nll     QuantLlama.score_rows(ids): pass + per-piece lm_head + ops.logit_nll;
      score_jsd     QuantLlama.score_rows(ids, dense_logits): ... + ops.logit_jsd against dense logits already on the device;
  (c) torch_nll     the same metrics formed the way they are without this feature, on the same box: an all_logits prompt pass ([S, vocab] fp16),
      torch_jsd     .float(), and the reference's formulas as framework ops (CrossEntropyLoss; softmax / clamp / log / KLDivLoss with log_target).

(c) is the comparison point -- the reference's procedure, not the code under test.  Median of ``--repeats`` alternating repeats in one process (one
warm-up round before them), with the spread beside it.  With ``--bars`` the row kernels' accuracy is recorded as well: per quantity the largest
|kernel - fp64| / bar over the cases of tests/test_gpu_evalmetrics.py (bar = max(4 * e32, floor), tests/evalmetrics_ref.py).

    python tools/eval_metrics_bench.py [--models Llama-2-7b-hf,Qwen2.5-7B] [--seq 2048] [--repeats 5] [--bars] [--out profiles/eval_metrics.json]
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


def _timed(fn):
    """(ms, peak bytes allocated above the start) of fn(), ended by a device synchronise"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return ms, peak


def _torch_jsd(p, q, eps=1e-7):
    """the reference's JSD module, restated with the same framework ops"""
    kl = torch.nn.KLDivLoss(reduction="batchmean", log_target=True)
    m = (0.5 * (p.softmax(-1) + q.softmax(-1))).clamp_min(eps).log()
    return 0.5 * (kl(m, p.log_softmax(-1)) + kl(m, q.log_softmax(-1)))


def measure(model, S, repeats):
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    cfg = arch.MODEL_CONFIGS[model]
    arch_linear, usage = arch.synthesize_arch(cfg, 3.0, seed=0)
    m = QuantLlama(cfg, arch_linear["linear"], device=DEV, max_seq=S, seed=0)
    V = cfg["vocab_size"]
    ids = torch.randint(3, V, (1, S), generator=torch.Generator().manual_seed(0)).to(DEV)
    dense = (torch.randn(S, V, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 3.0).to(torch.float16)[None]

    def today(with_jsd):
        m.all_logits = True
        try:
            m.prefill(ids[0], use_graph=False)
        finally:
            m.all_logits = False
        lg = m.logits_rows.float()                                      # [1, S, V] fp32, as the reference's forward returns them
        shift = lg[:, :-1].reshape(-1, V).contiguous()
        out = torch.nn.functional.cross_entropy(shift, ids[:, 1:].reshape(-1))
        if with_jsd:
            out = out + _torch_jsd(shift, dense[0, :-1].float().reshape(-1, V).contiguous())
        m.logits_rows = None
        return out

    legs = {
        "pass": lambda: m._rows_pass(ids, 0, cache=False),
        "score_nll": lambda: m.score_rows(ids),
        "score_jsd": lambda: m.score_rows(ids, dense_logits=dense),
        "torch_nll": lambda: today(False),
        "torch_jsd": lambda: today(True),
    }
    runs = {k: [] for k in legs}
    peaks = {k: 0 for k in legs}
    for rep in range(repeats + 1):                      # (the first round warms up every shape: not kept)
        for name, fn in legs.items():
            ms, peak = _timed(fn)
            if rep:
                runs[name].append(ms)
                peaks[name] = max(peaks[name], peak)
    res = {"model": model, "bits_usage": round(usage, 4), "vocab": V, "window": S, "score_rows_chunk": m.SCORE_ROWS, "repeats": repeats,
           "window_logits_fp16_bytes": S * V * 2, "window_logits_fp16_plus_fp32_bytes": S * V * 6}
    for name, ts in runs.items():
        res[name + "_ms"] = round(statistics.median(ts), 3)
        res[name + "_ms_runs"] = [round(t, 3) for t in ts]
        res[name + "_spread_pct"] = round(100.0 * (max(ts) - min(ts)) / statistics.median(ts), 2)
        res[name + "_peak_bytes"] = int(peaks[name])
    del m, dense
    torch.cuda.empty_cache()
    return res


def bars():
    """largest |kernel - fp64| / bar per quantity over the row-kernel cases of the GPU tests"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import evalmetrics_ref as ref
    from amq_amd import ops
    worst = {"nll": 0.0, "lse": 0.0, "jsd_fp16_q": 0.0, "jsd_fp32_q": 0.0}
    per_case = []
    for V in (100, 1001, 32000, 152064):
        g = torch.Generator().manual_seed(1000 + V)
        p = (torch.randn(33, V, generator=g) * 3.0).to(torch.float16)
        q = (p.float() + 0.3 * torch.randn(33, V, generator=g)).to(torch.float16)
        labels = torch.randint(0, V, (33,), generator=g)
        q32 = (q.float() + 1e-3 * torch.randn(q.shape, generator=torch.Generator().manual_seed(V))).contiguous()
        en, e16, e32 = ref.nll_expected(p, labels), ref.jsd_expected(p, q), ref.jsd_expected(p, q32)
        nll, lse, amax = ops.logit_nll(p.to(DEV), labels.to(DEV))
        assert torch.equal(amax.cpu(), en["argmax"])
        case = {"vocab": V, "rows": 33,
                "nll": ref.worst_ratio(nll, en["nll"], en["nll_bar"]), "nll_bar": en["nll_bar"],
                "lse": ref.worst_ratio(lse, en["lse"], en["lse_bar"]), "lse_bar": en["lse_bar"],
                "jsd_fp16_q": ref.worst_ratio(ops.logit_jsd(p.to(DEV), q.to(DEV)), e16["jsd"], e16["jsd_bar"]), "jsd_fp16_q_bar": e16["jsd_bar"],
                "jsd_fp32_q": ref.worst_ratio(ops.logit_jsd(p.to(DEV), q32.to(DEV)), e32["jsd"], e32["jsd_bar"]), "jsd_fp32_q_bar": e32["jsd_bar"]}
        per_case.append(case)
        for k in worst:
            worst[k] = max(worst[k], case[k])
    return {"bar": "per row |kernel - fp64| <= max(4 * e32, floor); floors 2e-6 (nll, lse), 2.4e-7 (jsd); a ratio <= 1 is inside the bar",
            "largest_ratio": {k: round(v, 4) for k, v in worst.items()}, "cases": per_case}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="Llama-2-7b-hf,Qwen2.5-7B")
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bars", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0)}
    if a.bars:
        res["accuracy"] = bars()
        print(json.dumps(res["accuracy"]["largest_ratio"]), flush=True)
    res["timing"] = []
    for model in (v for v in a.models.split(",") if v):
        with torch.inference_mode():
            res["timing"].append(measure(model, a.seq, a.repeats))
        print(json.dumps(res["timing"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
