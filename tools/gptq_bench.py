"""What the GPTQ solve costs per layer shape of Llama-2-7B at 3 bit, group 128: ops.gptq_quantize (solve + flag + pack kernels and its one 4-byte
read-back) against the same solver run as framework passes on the same device:

  kernel   ops.gptq_quantize(W, U, 3, 128)
  torch    the reference's procedure (amq/quantization/gptq.py:255-292: blocks of 128 columns, about a dozen torch ops per column, the columns behind
           the block updated by one matmul per block) with the kernel's deployment rule (fp16 scale, fp16 weight), + hqq_format.pack_rows

The comparison leg is the reference's procedure, not the code under test; its trailing update is a GEMM, so its bits are not the kernel's.  The
two legs alternate in one process; median of ``--repeats`` after one warm-up round, spreads beside it.  Two further legs are timed on their own,
per K: ``hessian`` (ops.GPTQHessian.add_batch of one window of ``--tokens`` rows, torch ops) and ``factorise`` (ops.gptq_hinv: three torch.linalg
calls; where it ran is recorded).  The result is merged into ``--out`` under "timing" (tests/test_gpu_gptq_quantize.py keeps its observed parity
under "parity" there).

    python tools/gptq_bench.py [--repeats 5] [--tokens 2048] [--out profiles/gptq_quantize.json]

``--act-order``: the variant instead (activation order + static groups, ops.gptq_quantize(..., perm=, static_groups=True): parameters + solve +
flag + pack kernels) against the plain solve in the same session, at 2, 3 and 4 bit over the same three shapes.  The calibration gets hot channels
(every 64th column x 12), as real activations have and as an order by diag(H) needs to matter; both legs see the same W and the same H (the
variant's U is the factor of H[perm][:, perm]), alternate, and report the median of ``--repeats`` after a warm-up round, the proxy loss
tr(dW H dW^T) of each result and their ratio.  A synthetic calibration: nothing here says what the variant does to a real model's perplexity.

    python tools/gptq_bench.py --act-order [--repeats 5] [--tokens 2048] [--out profiles/gptq_actorder.json]
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
BITS, GROUP, BLOCK = 3, 128, 128


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    del out
    return ms


def torch_solve(W, U, bits, group):
    """fasterquant's loop as torch ops on W's device (no host read), with the deployment rule; returns (codes [R, group], scale, zero, loss)"""
    W = W.float().clone()
    N, K = W.shape
    maxq = float(2 ** bits - 1)
    Q = torch.empty_like(W)
    S = torch.empty(N, K // group, device=W.device)
    Z = torch.empty_like(S)
    loss = torch.zeros(N, device=W.device)
    zero = torch.zeros(N, device=W.device)
    for i1 in range(0, K, BLOCK):
        i2 = i1 + BLOCK
        W1 = W[:, i1:i2].clone()
        Err1 = torch.empty_like(W1)
        U1 = U[i1:i2, i1:i2]
        for g0 in range(i1, i2, group):
            x = W[:, g0:g0 + group]
            xmin = torch.minimum(x.min(1)[0], zero)
            xmax = torch.maximum(x.max(1)[0], zero)
            both = (xmin == 0) & (xmax == 0)
            xmin = torch.where(both, xmin - 1.0, xmin)
            xmax = torch.where(both, xmax + 1.0, xmax)
            s = ((xmax - xmin) / maxq).to(torch.float16).float().clamp(min=2.0 ** -24)
            S[:, g0 // group] = s
            Z[:, g0 // group] = torch.round(-xmin / s)
        for i in range(BLOCK):
            w = W1[:, i]
            d = U1[i, i]
            s, z = S[:, (i1 + i) // group], Z[:, (i1 + i) // group]
            q = torch.clamp(torch.round(w / s) + z, 0.0, maxq)
            wh = ((q - z) * s).to(torch.float16).float()
            Q[:, i1 + i] = q
            r = w - wh
            loss += (r * r) / (d * d) / 2.0
            e = r / d
            W1[:, i:] -= e.unsqueeze(1) * U1[i, i:].unsqueeze(0)
            Err1[:, i] = e
        W[:, i2:] -= Err1.matmul(U[i1:i2, i2:])
    return Q.reshape(-1, group).to(torch.int32), S.to(torch.float16).reshape(-1, 1), Z.to(torch.float16).reshape(-1, 1), loss


def _runs(row, leg, ts):
    row[leg + "_ms"] = round(statistics.median(ts), 3)
    row[leg + "_ms_runs"] = [round(t, 3) for t in ts]
    row[leg + "_spread_pct"] = round(100.0 * (max(ts) - min(ts)) / statistics.median(ts), 2)


def act_order_main(a):
    """the variant against the plain solve: one row per (shape, bits)"""
    from amq_amd import ops
    rows, calib = [], {}
    with torch.inference_mode():
        for K in sorted({k for _, _, k in SHAPES}):
            g = torch.Generator(device=DEV).manual_seed(K)
            r = K // 8
            X = (torch.randn(a.tokens, r, device=DEV, generator=g) @ (torch.randn(r, K, device=DEV, generator=g) / r ** 0.5)
                 + 0.3 * torch.randn(a.tokens, K, device=DEV, generator=g))
            X[:, ::64] *= 12.0
            acc = ops.GPTQHessian(K, DEV)
            acc.add_batch(X.to(torch.float16).unsqueeze(0))
            perm = ops.gptq_act_order(acc.H)
            calib[K] = (acc.H, perm, ops.gptq_hinv(acc.H, 0.01)[0], ops.gptq_hinv(acc.H[perm][:, perm], 0.01)[0])
            del X, acc
        for name, N, K in SHAPES:
            W = (torch.randn(N, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(N + K)) * 0.02).to(torch.float16)
            H, perm, U, U_p = calib[K]
            for bits in (2, 3, 4):
                legs = {"plain": lambda: ops.gptq_quantize(W, U, bits, GROUP),
                        "act_order_static": lambda: ops.gptq_quantize(W, U_p, bits, GROUP, perm=perm, static_groups=True)}
                runs = {k: [] for k in legs}
                for rep in range(a.repeats + 1):            # (the first round warms up: not kept)
                    for leg, fn in legs.items():
                        ms = _timed(fn)
                        if rep:
                            runs[leg].append(ms)
                row = {"layer": name, "N": N, "K": K, "bits": bits, "group": GROUP, "repeats": a.repeats, "tokens": a.tokens}
                for leg, fn in legs.items():
                    _runs(row, leg, runs[leg])
                    h = fn()
                    d = W.float() - ops.dequantize_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, N, K, GROUP).float()
                    row[leg + "_proxy_loss"] = float(((d @ H) * d).double().sum().item())
                    del h, d
                row["time_over_plain"] = round(row["act_order_static_ms"] / row["plain_ms"], 3)
                row["proxy_loss_over_plain"] = round(row["act_order_static_proxy_loss"] / row["plain_proxy_loss"], 4)
                rows.append(row)
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "layers": rows,
           "note": "synthetic calibration with hot channels; no real model or dataset was measured"}
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["timing"] = res
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--out", default=None)
    ap.add_argument("--act-order", action="store_true", help="time the act-order + static-groups variant against the plain solve")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.act_order:
        return act_order_main(a)
    from amq_amd import ops
    from amq_amd.hqq_format import pack_rows

    def torch_leg(W, U):
        q, s, z, loss = torch_solve(W, U, BITS, GROUP)
        return pack_rows(q, BITS), s, z, loss

    rows, prep, factors = [], [], {}
    with torch.inference_mode():
        for K in sorted({k for _, _, k in SHAPES}):
            g = torch.Generator(device=DEV).manual_seed(K)
            r = K // 8
            X = (torch.randn(a.tokens, r, device=DEV, generator=g) @ (torch.randn(r, K, device=DEV, generator=g) / r ** 0.5)
                 + 0.3 * torch.randn(a.tokens, K, device=DEV, generator=g)).to(torch.float16).unsqueeze(0)
            acc = ops.GPTQHessian(K, DEV)
            row = {"K": K, "tokens": a.tokens, "repeats": a.repeats}
            _runs(row, "hessian", [_timed(lambda: acc.add_batch(X)) for rep in range(a.repeats + 1)][1:])
            where = []
            _runs(row, "factorise", [_timed(lambda: where.append(ops.gptq_hinv(acc.H, 0.01, return_where=True)[2])) for rep in range(a.repeats + 1)][1:])
            row["factorise_ran_on"] = where[-1]
            factors[K] = ops.gptq_hinv(acc.H, 0.01)[0]
            prep.append(row)
            print(json.dumps(row), flush=True)
            del X, acc
        for name, N, K in SHAPES:
            W = (torch.randn(N, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(N + K)) * 0.02).to(torch.float16)
            U = factors[K]
            legs = {"kernel": lambda: ops.gptq_quantize(W, U, BITS, GROUP), "torch": lambda: torch_leg(W, U)}
            runs = {k: [] for k in legs}
            for rep in range(a.repeats + 1):            # (the first round warms up: not kept)
                for leg, fn in legs.items():
                    ms = _timed(fn)
                    if rep:
                        runs[leg].append(ms)
                torch.cuda.empty_cache()
            h, info = ops.gptq_quantize(W, U, BITS, GROUP, return_info=True)
            row = {"layer": name, "N": N, "K": K, "bits": BITS, "group": GROUP, "repeats": a.repeats, "kernel_solver_loss": info.loss,
                   "torch_solver_loss": float(torch_leg(W, U)[3].double().sum().item())}
            for leg, ts in runs.items():
                _runs(row, leg, ts)
            row["torch_over_kernel"] = round(row["torch_ms"] / row["kernel_ms"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "layers": rows, "per_K": prep}
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["timing"] = res
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
