"""AWQ's round-to-nearest and clip search as csrc/amq_awq.hip computes them (include/amq_hip.h), restated in torch fp32 on the CPU:
one torch op per rounding, all rows and groups at once.

``deploy=True`` is the kernels' rule: the scale is rounded to fp16 before it is used, ``w^ = fp16((q - z) * s16)`` is the weight the dequantize and
matmul kernels produce, scaled weights, bounds and the dense output are fp16, and the clip search's output error is the header's fmaf chain and
summation order.  ``deploy=False`` keeps an fp32 scale, fp32 bounds and ``w^ = (q - z) * s``, and takes the clip error as the difference of two fp32
output sums averaged over the rows: the reference's own rule (awq_utils/quantizer.py:61-105, auto_clip.py:27-87), used only to show that the algorithm
is the reference's.

``fmaf(a, b, c)`` is emulated as ``float32(float64(a) * float64(b) + float64(c))``.  The product of two fp32 numbers is exact in fp64; the sum is
rounded to fp64 and then to fp32, which differs from the single rounding of a true fmaf only when the fp64 sum lands exactly on the midpoint of two
fp32 neighbours after its own rounding moved it there (double rounding) -- it needs the exact sum's bits 25 .. 53 below the leading one to be
1000...0 or 0111...1 with a non-zero tail beyond, about one chain step in 2^29.
"""
import torch

GROUPS = (32, 64, 128)
STEPS = 10
ROWS = 8


def quantize_workspace_bytes(N, K, group):
    """include/amq_hip.h amq_awq_quantize_workspace_bytes: int32 flags [N * K / 512], byte codes [N, K]"""
    if group not in GROUPS or N <= 0 or K <= 0 or N % 16 or K % 128:
        return 0
    return N * K // 128 + N * K


def workspace_bytes(N, K, T, group):
    """include/amq_hip.h amq_awq_clip_workspace_bytes: int32 flags, one per (8 rows, group)"""
    if group not in GROUPS or N <= 0 or K <= 0 or N % 16 or K % 128 or T < 1:
        return 0
    return 4 * (N // ROWS) * (K // group)


def rtn(v, bits, deploy=True):
    """round to nearest of the groups v fp32 [..., G] (holding fp16 values): (q, s, z, w^) with s, z [..., 1]"""
    maxq = float(2 ** bits - 1)
    xmax = v.amax(dim=-1, keepdim=True)
    xmin = v.amin(dim=-1, keepdim=True)
    s = torch.clamp(xmax - xmin, min=1e-5) / maxq
    if deploy:
        s = s.to(torch.float16).float()
    z = torch.clamp(torch.round(-xmin / s), 0.0, maxq) + 0.0          # (+ 0: a -0 from rounding a small negative quotient becomes +0)
    q = torch.clamp(torch.round(v / s) + z, 0.0, maxq)
    t = (q - z) * s
    return q, s, z, (t.to(torch.float16).float() if deploy else t)


def quantize(W, bits, group=128, col_scale=None, hi=None, lo=None, deploy=True):
    """W fp16 (or fp32 holding the values) [N, K]; col_scale fp32 [K]; hi, lo [N, K / group].  Returns q int32 [R, group] (Format A's groups before
    packing), scale, zero fp16 [R, 1] (deploy) or fp32, W_hat fp32 [N, K] (the packed layer's weights), dense fp32 [N, K] (W_hat over the column
    scale, an fp16 value if deploy), nonfinite."""
    assert group in GROUPS and bits in (2, 3, 4)
    v = W.detach().float()
    N, K = v.shape
    if col_scale is not None:
        c = col_scale.detach().float().reshape(1, K)
        v = v * c
        if deploy:
            v = v.to(torch.float16).float()
    bad = not bool(torch.isfinite(v).all())
    v = v.reshape(N, K // group, group)
    if hi is not None:
        h, l = hi.detach().float().reshape(N, -1, 1), lo.detach().float().reshape(N, -1, 1)
        bad = bad or not bool(torch.isfinite(h).all() and torch.isfinite(l).all())
        v = torch.minimum(torch.maximum(v, l), h)
    q, s, z, wh = rtn(v, bits, deploy)
    wh = wh.reshape(N, K)
    dense = wh
    if col_scale is not None:
        dense = wh / c
        if deploy:
            dense = dense.to(torch.float16).float()
    bad = bad or not bool(torch.isfinite(dense).all())
    return {"q": q.reshape(-1, group).to(torch.int32), "scale": (s.to(torch.float16) if deploy else s).reshape(-1, 1),
            "zero": (z.to(torch.float16) if deploy else z).reshape(-1, 1), "W_hat": wh, "dense": dense, "nonfinite": int(bad)}


def _fmaf(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _shrink(i):
    return torch.tensor(1.0 - i / 20.0, dtype=torch.float32)          # the fp32 nearest to 1 - i / 20


def clip(W, X, bits, group=128, deploy=True):
    """W [N, K] (the layer's current weights), X [T, K] (the sampled rows), fp16 or fp32 holding fp16 values.  Returns hi, lo [N, K / group] (fp16 if
    deploy, else fp32), best int32 [N, K / group], err fp32 [N, K / group, 10] (deploy: the sums; else the reference's means)."""
    assert group in GROUPS and bits in (2, 3, 4)
    w = W.detach().float()
    x = X.detach().float()
    N, K = w.shape
    T = x.shape[0]
    kg = K // group
    w = w.reshape(N, kg, group)
    mx = w.amax(dim=-1, keepdim=True)
    mn = w.amin(dim=-1, keepdim=True)
    if deploy:
        Tp = -(-T // 16) * 16
        xp = torch.zeros(Tp, K)
        xp[:T] = x
        xg = xp.reshape(Tp, kg, group).permute(1, 0, 2).contiguous()      # [kg, Tp, G]
    else:
        xg = x.reshape(1, T, kg, group)
        org = (xg * w.unsqueeze(1)).sum(dim=-1)                           # [N, T, kg]
    errs, his, los = [], [], []
    for i in range(STEPS):
        f = _shrink(i)
        hi, lo = mx * f, mn * f
        if deploy:
            hi, lo = hi.to(torch.float16).float(), lo.to(torch.float16).float()
        wh = rtn(torch.minimum(torch.maximum(w, lo), hi), bits, deploy)[3]
        if deploy:
            d = wh - w                                                    # [N, kg, G]
            acc = torch.zeros(N, kg, Tp)
            for c in range(group):                                        # the fmaf chain, ascending columns
                acc = _fmaf(xg[:, :, c].unsqueeze(0), d[:, :, c].unsqueeze(2), acc)
            o2 = (acc * acc).reshape(N, kg, Tp // 16, 4, 4)               # t = 16 a + 4 h + r
            P = torch.zeros(N, kg, 4)
            for a in range(Tp // 16):
                for r in range(4):
                    P = P + o2[:, :, a, :, r]
            err = (P[..., 0] + P[..., 1]) + (P[..., 2] + P[..., 3])
        else:
            cur = (xg * wh.unsqueeze(1)).sum(dim=-1)
            err = (cur - org).pow(2).mean(dim=1)                          # [N, kg]
        errs.append(err)
        his.append(hi.squeeze(-1))
        los.append(lo.squeeze(-1))
    err = torch.stack(errs, dim=-1)
    best = torch.zeros(N, kg, dtype=torch.int64)
    m = err[..., 0].clone()
    for i in range(1, STEPS):
        better = err[..., i] < m                                          # strict: the least shrink wins a tie
        m = torch.where(better, err[..., i], m)
        best = torch.where(better, torch.full_like(best, i), best)
    hi = torch.stack(his, dim=-1).gather(-1, best.unsqueeze(-1)).squeeze(-1)
    lo = torch.stack(los, dim=-1).gather(-1, best.unsqueeze(-1)).squeeze(-1)
    if deploy:
        hi, lo = hi.to(torch.float16), lo.to(torch.float16)
    return {"hi": hi, "lo": lo, "best": best.to(torch.int32), "err": err}
