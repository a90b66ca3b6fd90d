"""What OWQ costs per layer shape of Llama-2-7B at 3 bit, group 128, n_out by the reference's rule (patching.owq_n_out at 3.25 average bits): the
whole-row range pass and the solve, timed separately, each against the same step run as framework passes on the same device:

  range   kernel  ops.owq_range(W, 3): the range kernel + the column sums + its one 4-byte read-back
          torch   the reference's find_params (owq.py:435-513: 40 x 2^bits passes over W, about ten torch ops each) with the deployment rule,
                  then the column sums of (W - W^)^2
  solve   kernel  ops.owq_quantize(W_p, U_p, n_out, 3): solve + flag + pack kernels and its one 4-byte read-back
          torch   the reference's fasterquant (owq.py:348-385: blocks of 128 columns, find_params per group on the current values, about a dozen
                  torch ops per column, the columns behind the block updated by one matmul per block) with the deployment rule, +
                  hqq_format.pack_rows

The comparison legs are the reference's procedure, not the code under test: their scores are torch's fp32 pow and sums, their trailing update is a
GEMM, so their bits are not the kernels'.  The two legs of a step alternate in one process; median of ``--repeats`` after one warm-up round, spreads
beside it.  Also timed: the HIPOWQLinear forward at M = 1 and M = 2048 for 4096 x 4096 beside the plain HIPQuantLinear's (device events over
``--iters`` calls).  The result is merged into ``--out`` under "timing" (tests/test_gpu_owq_quantize.py keeps its observed parity under "parity").

    python tools/owq_bench.py [--repeats 5] [--tokens 2048] [--out profiles/owq_quantize.json]
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
SHAPES = [("attention q/k/v/o", "self_attn.q_proj", 4096, 4096), ("mlp gate/up", "mlp.up_proj", 11008, 4096),
          ("mlp down", "mlp.down_proj", 4096, 11008)]
BITS, GROUP, BLOCK, NUM, AVG_BITS = 3, 128, 128, 40, 3.25


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    del out
    return ms


def torch_find_params(x, bits, num=NUM):
    """find_params (mse, asymmetric, per channel) of the rows of x fp32 [N, L] as torch ops with the deployment rule: (d16, zp) fp32 [N]"""
    maxq = float(2 ** bits - 1)
    zero = torch.zeros(x.shape[0], device=x.device)
    xmin = torch.minimum(x.min(1)[0], zero)
    xmax = torch.maximum(x.max(1)[0], zero)
    xrange = xmax - xmin
    best = torch.full_like(xmin, 1e10)
    bd, bz = torch.zeros_like(xmin), torch.zeros_like(xmin)
    for i in range(1, num + 1):
        d = ((xrange / num * i) / maxq).clamp(min=1e-8).to(torch.float16).float().clamp(min=2.0 ** -24)
        d1 = d.unsqueeze(1)
        r = torch.round(x / d1)
        for zp in range(2 ** bits):
            wh = ((torch.clamp(r + zp, 0.0, maxq) - zp) * d1).to(torch.float16).float()
            score = (x - wh).abs().pow(2.4).mean(1)
            better = score < best
            bd = torch.where(better, d, bd)
            bz = torch.where(better, torch.full_like(bz, float(zp)), bz)
            best = torch.minimum(best, score)
    return bd, bz


def torch_range(W, bits):
    W = W.float()
    d, z = torch_find_params(W, bits)
    d1, z1 = d.unsqueeze(1), z.unsqueeze(1)
    wh = ((torch.clamp(torch.round(W / d1) + z1, 0.0, float(2 ** bits - 1)) - z1) * d1).to(torch.float16).float()
    return d, z, ((W - wh) ** 2).sum(0)


def torch_solve(Wp, U, n_out, bits):
    """fasterquant's loop over the permuted columns as torch ops on W's device (no host read), with the deployment rule"""
    W = Wp.float().clone()
    N, K = W.shape
    nq = K - n_out
    Kp = -(-nq // BLOCK) * BLOCK
    maxq = float(2 ** bits - 1)
    Q = torch.zeros(N, Kp, device=W.device)
    S = torch.empty(N, Kp // GROUP, device=W.device)
    Z = torch.empty_like(S)
    loss = torch.zeros(N, device=W.device)
    for i1 in range(0, nq, BLOCK):
        i2 = min(i1 + BLOCK, nq)
        W1 = W[:, i1:i2].clone()
        Err1 = torch.empty_like(W1)
        U1 = U[i1:i2, i1:i2]
        s, z = torch_find_params(W1, bits)
        S[:, i1 // GROUP], Z[:, i1 // GROUP] = s, z
        for i in range(i2 - i1):
            w = W1[:, i]
            d = U1[i, i]
            q = torch.clamp(torch.round(w / s) + z, 0.0, maxq)
            wh = ((q - z) * s).to(torch.float16).float()
            Q[:, i1 + i] = q
            r = w - wh
            loss += (r * r) / (d * d) / 2.0
            e = r / d
            W1[:, i:] -= e.unsqueeze(1) * U1[i, i:].unsqueeze(0)
            Err1[:, i] = e
        Q[:, i2:i1 + BLOCK] = z.unsqueeze(1)
        W[:, i2:] -= Err1.matmul(U[i1:i2, i2:])
    return Q.reshape(-1, GROUP).to(torch.int32), S.to(torch.float16).reshape(-1, 1), Z.to(torch.float16).reshape(-1, 1), W[:, nq:].half(), loss


def _runs(row, leg, ts):
    row[leg + "_ms"] = round(statistics.median(ts), 3)
    row[leg + "_ms_runs"] = [round(t, 3) for t in ts]
    row[leg + "_spread_pct"] = round(100.0 * (max(ts) - min(ts)) / statistics.median(ts), 2)


def _alternate(legs, repeats):
    runs = {k: [] for k in legs}
    for rep in range(repeats + 1):                      # (the first round warms up: not kept)
        for leg, fn in legs.items():
            ms = _timed(fn)
            if rep:
                runs[leg].append(ms)
        torch.cuda.empty_cache()
    return runs


def _forward_us(mod, x, iters):
    for _ in range(10):
        mod(x)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        mod(x)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from amq_amd import ops
    from amq_amd.hqq_format import pack_rows
    from amq_amd.patching import owq_n_out
    from amq_amd.quant_linear import HIPOWQLinear, HIPQuantLinear

    def torch_leg(Wp, U, n_out):
        q, s, z, W_out, loss = torch_solve(Wp, U, n_out, BITS)
        return pack_rows(q, BITS), s, z, W_out, loss

    rows, hess, forward = [], {}, []
    with torch.inference_mode():
        for K in sorted({k for _, _, _, k in SHAPES}):
            g = torch.Generator(device=DEV).manual_seed(K)
            r = K // 8
            X = (torch.randn(a.tokens, r, device=DEV, generator=g) @ (torch.randn(r, K, device=DEV, generator=g) / r ** 0.5)
                 + 0.3 * torch.randn(a.tokens, K, device=DEV, generator=g)).to(torch.float16).unsqueeze(0)
            X[..., ::97] *= 10.0
            acc = ops.GPTQHessian(K, DEV)
            acc.add_batch(X)
            hess[K] = acc.H
            del X, acc
        for name, linear, N, K in SHAPES:
            W = (torch.randn(N, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(N + K)) * 0.02).to(torch.float16)
            n_out = owq_n_out(K, AVG_BITS, linear, GROUP)
            row = {"layer": name, "N": N, "K": K, "bits": BITS, "group": GROUP, "n_out": n_out, "repeats": a.repeats}
            for leg, ts in _alternate({"range_kernel": lambda: ops.owq_range(W, BITS, return_info=True), "range_torch": lambda: torch_range(W, BITS)},
                                      a.repeats).items():
                _runs(row, leg, ts)
            ids, _ = ops.owq_select(W, hess[K], n_out, BITS)
            U, dead = ops.gptq_hinv(hess[K][ids][:, ids], 0.01)
            Wp = W[:, ids].contiguous()
            for leg, ts in _alternate({"solve_kernel": lambda: ops.owq_quantize(Wp, U, n_out, BITS), "solve_torch": lambda: torch_leg(Wp, U, n_out)},
                                      a.repeats).items():
                _runs(row, leg, ts)
            h, W_out, info = ops.owq_quantize(Wp, U, n_out, BITS, return_info=True)
            row["kernel_solver_loss"] = info.loss
            row["torch_solver_loss"] = float(torch_leg(Wp, U, n_out)[4].double().sum().item())
            row["range_torch_over_kernel"] = round(row["range_torch_ms"] / row["range_kernel_ms"], 2)
            row["solve_torch_over_kernel"] = round(row["solve_torch_ms"] / row["solve_kernel_ms"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if (N, K) == (4096, 4096):
                owq = HIPOWQLinear.from_owq(h, W_out, ids)
                plain = HIPQuantLinear.from_hqq(ops.hqq_quantize(W, BITS, GROUP))
                for M in (1, 2048):
                    x = torch.randn(M, K, device=DEV, dtype=torch.float16)
                    both = {"M": M, "iters": a.iters}
                    for rep in range(3):                # alternating, the median of three windows
                        for leg, mod in (("owq_us", owq), ("plain_us", plain)):
                            both.setdefault(leg + "_runs", []).append(round(_forward_us(mod, x, a.iters), 2))
                    for leg in ("owq_us", "plain_us"):
                        both[leg] = statistics.median(both[leg + "_runs"])
                    both["owq_over_plain"] = round(both["owq_us"] / both["plain_us"], 3)
                    forward.append(both)
                    print(json.dumps(both), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "layers": rows, "forward_4096x4096": forward}
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["timing"] = res
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
