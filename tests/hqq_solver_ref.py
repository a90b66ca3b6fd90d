"""HQQ's quantizer with its proximal solver, restated in torch fp32 with the summation orders of the device kernels (csrc/amq_quantize.hip;
DESIGN.md 3.9).  Written from the arithmetic, not from the reference's text; runs on any torch device (tools/quantize_bench.py times it on the GPU
as "the same loop as framework passes").

Every operation is its own fp32 rounding (torch does not contract), tensor / tensor is true division, rint is round-half-even.  The initial
s = maxv / den is the one exception the reference's text hides: ``float / tensor`` is ``tensor.reciprocal() * float`` in torch.

Summation orders (the only freedom the arithmetic leaves):
  * a group's sum: a binary tree over the element index, level by level over index bit 0, 1, ... (adjacent pairs first) -- in-lane pairs, DPP inside
    a 16-lane row, rows (0 + 1) + (2 + 3);
  * the tensor's sum of |W - W_r| per iteration: a wave's PASS (64 lanes: one group of >= 64, or two groups of 32) is the same tree; a wave adds
    its T passes serially in pass order, the workgroup its 4 waves in wave order, the stop kernel the workgroups in index order.
"""
import torch

ITERS = 20
WAVES = 4            # waves per workgroup of the solve kernel
MAX_WGS = 1024       # the solve grid is capped here: passes per wave T = ceil(passes / (WAVES * MAX_WGS))


def geometry(N, K, group):
    """(groups R, wave passes P, passes per wave T, workgroups) of the solve launch: a function of the shape only"""
    R = N * K // group
    P = R // 2 if group == 32 else R
    T = -(-P // (WAVES * MAX_WGS))
    return R, P, T, -(-P // (WAVES * T))


def workspace_bytes(N, K, group):
    """include/amq_hip.h amq_hqq_quantize_workspace_bytes: fp32 s[R], Z[20][R], Epart[20][wgs] and int32 nonfinite[wgs]"""
    R, _, _, wgs = geometry(N, K, group)
    return 4 * ((ITERS + 1) * R + (ITERS + 1) * wgs)


def tree_sum(x):
    """sum over the last axis (a power of two) as a binary tree over the index bits, lowest first"""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _tensor_sums(a_trace, N, K, group):
    """[ITERS, R, G] of |e| -> [ITERS] sums in the kernels' order"""
    R, P, T, wgs = geometry(N, K, group)
    s = tree_sum(a_trace.reshape(ITERS, P, -1))                         # per pass
    pad = torch.zeros(ITERS, wgs * WAVES * T - P, dtype=s.dtype, device=s.device)
    s = torch.cat([s, pad], 1).reshape(ITERS, wgs, WAVES, T)
    wave = torch.zeros(ITERS, wgs, WAVES, dtype=s.dtype, device=s.device)
    for t in range(T):
        wave = wave + s[..., t]
    part = torch.zeros(ITERS, wgs, dtype=s.dtype, device=s.device)
    for w in range(WAVES):
        part = part + wave[..., w]
    total = torch.zeros(ITERS, dtype=s.dtype, device=s.device)
    for g in range(wgs):
        total = total + part[:, g]
    return total, part


def solve(W, nbits, group_size=128, round_zero=None):
    """W fp16 / fp32 [N, K] -> dict(q [R, G] float codes, scale fp16 [R, 1], zero fp16 [R, 1], stop, mean_err [20] fp32, gap) and the
    kernels' workspace contents: s [R], Z [20, R] (the zero after each iteration), partials [20, workgroups] (the workgroups' sums of |e|).
    ``gap``: relative gap of the comparison that decided ``stop`` (of the closest comparison made, if the loop ran out)."""
    N, K = W.shape
    G = int(group_size)
    maxv = float(2 ** nbits - 1)
    if round_zero is None:
        round_zero = nbits == 4
    w = W.detach().float().reshape(-1, G)
    mn = w.min(dim=1, keepdim=True)[0]
    mx = w.max(dim=1, keepdim=True)[0]
    den = mx - mn
    s = den.reciprocal() * maxv          # (what torch makes of the reference's `max_v / tensor`: two roundings, not one division)
    s = torch.where(den.abs() <= 1e-4, torch.ones_like(s), s)
    s = torch.clamp(s, max=2e4)
    z = (-mn) * s
    if round_zero:
        z = torch.round(z)
    Z, A = [], []
    for _ in range(ITERS):
        q = torch.clamp(torch.round(w * s + z), 0.0, maxv)
        r = (q - z) / s
        e = w - r
        a = e.abs()
        A.append(a)
        sh = torch.clamp(a - 0.1 * torch.pow(a, -0.3), min=0.0) * torch.sign(e)
        z = (tree_sum(q - (w - sh) * s) / float(G)).unsqueeze(1)
        Z.append(z)
    sums, part = _tensor_sums(torch.stack(A), N, K, G)
    mean_err = sums / torch.tensor(float(N * K), dtype=torch.float32, device=sums.device)
    best, stop, gap = float("inf"), ITERS - 1, float("inf")
    errs = [float(v) for v in mean_err.cpu()]
    for i, m in enumerate(errs):
        if m < best:
            best = m
        else:
            stop, gap = i, (abs(m - best) / best if best > 0 else float("inf"))
            break
    if stop == ITERS - 1 and gap == float("inf") and ITERS > 1:
        # ran out: the closest call among the comparisons that were made
        run, g = float("inf"), float("inf")
        for m in errs:
            if run != float("inf") and run > 0:
                g = min(g, abs(m - run) / run)
            run = min(run, m)
        gap = g
    z = Z[stop]
    q = torch.clamp(torch.round(w * s + z), 0.0, maxv)
    return {"q": q, "scale": (1.0 / s).to(torch.float16), "zero": z.to(torch.float16), "stop": stop, "mean_err": mean_err, "gap": gap,
            "Z": torch.stack(Z).squeeze(-1), "s": s.squeeze(-1), "partials": part}
