"""OWQ as csrc/amq_owq.hip computes it (include/amq_hip.h), restated in torch fp32 on the CPU from that specification: one torch op
per rounding, all rows at once.  The one thing the host does differently is the score of a range candidate: the device evaluates |d|^2.4 with the
hardware's log2 / exp2 in fp32 and a fixed sum order; here the score is formed in fp64 from the same fp32 values (``scores64``) -- the criterion
the tests hold the device's choice against.  ``solve(..., choices=...)`` therefore replays the solve with the device's (i, zp) per row and group:
everything else is basic IEEE fp32 arithmetic in a fixed order and must agree bit for bit.

``deploy=True`` is the kernel's rule (the candidate's step is rounded to fp16, floor 2^-24, before it is used; the score and the error feedback see
``w^ = fp16((q - zp) * d16)``); ``deploy=False`` keeps the fp32 step and ``w^ = (q - zp) * delta``: the reference's own rule, used only to show
that the algorithm is the reference's.
"""
import torch

BLOCK = 128
NUM = 40


def packed_columns(K, n_out):
    return -(-(K - n_out) // BLOCK) * BLOCK


def workspace_bytes(N, K, n_out, group=128):
    """include/amq_hip.h amq_owq_quantize_workspace_bytes: fp32 errors [N, Kp], int32 flags [N / 4], byte codes [N, Kp]"""
    if group != 128 or N <= 0 or K <= 0 or N % 16 or K % 128 or n_out < 0 or n_out % 2 or n_out >= K:
        return 0
    return 5 * N * packed_columns(K, n_out) + N


def n_out_rule(K, avg_bits, name, group=128):
    """owq.py:69-70, 146-153 from the specification: r = 12 / (16 - (avg_bits - 32 / group)) * 0.1 / 7, n_out = round(K r ratio), made even"""
    ratio = 1 if name.startswith("self_attn.") else 0.375
    r = (12 / (16 - (avg_bits - 32 / group))) * 0.1
    r /= 7
    n = round(K * r * ratio)
    return n + n % 2


def extremes(v):
    zero = torch.zeros(v.shape[0])
    return torch.minimum(v.min(1)[0], zero), torch.maximum(v.max(1)[0], zero)


def step(xrange, num, i, maxq, deploy=True):
    """candidate i's step [N] (i an int or an int tensor [N])"""
    i = i.float() if isinstance(i, torch.Tensor) else float(i)
    tmp_max = (xrange / float(num)) * i
    delta = torch.clamp(tmp_max / maxq, min=1e-8)
    return torch.clamp(delta.to(torch.float16).float(), min=2.0 ** -24) if deploy else delta


def deployed(v, d, zp, maxq, deploy=True):
    """(q, w^) of v [N, L] under the rows' step d [N] and zero-point zp (a number or a tensor [N])"""
    d = d.unsqueeze(1)
    zp = zp.float().unsqueeze(1) if isinstance(zp, torch.Tensor) else float(zp)
    q = torch.clamp(torch.round(v / d) + zp, 0.0, maxq)
    t = (q - zp) * d
    return q, (t.to(torch.float16).float() if deploy else t)


def scores64(v, bits, num=NUM, deploy=True):
    """(fp64 scores [N, num, 2^bits], fp32 steps [N, num]) of every candidate of the segments v fp32 [N, L]"""
    v = v.float()
    N, L = v.shape
    maxq = float(2 ** bits - 1)
    xmin, xmax = extremes(v)
    xrange = xmax - xmin
    S = torch.zeros(N, num, 2 ** bits, dtype=torch.float64)
    D = torch.zeros(N, num)
    for i in range(1, num + 1):
        d = step(xrange, num, i, maxq, deploy)
        D[:, i - 1] = d
        for zp in range(2 ** bits):
            _, wh = deployed(v, d, zp, maxq, deploy)
            S[:, i - 1, zp] = (v.double() - wh.double()).abs().pow(2.4).sum(1) / L
    return S, D


def range_search(v, bits, num=NUM, deploy=True):
    """the range search of the segments v [N, L] with the score in fp64: dict of scale (the winner's step, fp32 [N]), zero (fp32 [N]), choice
    (int32 [N, 2]: (i, zp)), score (fp64 [N])"""
    S, D = scores64(v, bits, num, deploy)
    N = S.shape[0]
    flat = S.reshape(N, -1)
    flat = torch.where(torch.isfinite(flat), flat, torch.full_like(flat, float("inf")))
    best = flat.argmin(1)                               # (the first of equal minima: i ascending, zp ascending)
    won = flat.gather(1, best.unsqueeze(1)).squeeze(1) < 1e10
    i = torch.where(won, best // 2 ** bits + 1, torch.zeros_like(best))
    zp = torch.where(won, best % 2 ** bits, torch.zeros_like(best))
    scale = torch.where(won, D.gather(1, (i - 1).clamp(min=0).unsqueeze(1)).squeeze(1), torch.zeros(N))
    return {"scale": scale, "zero": zp.float(), "choice": torch.stack([i, zp], 1).to(torch.int32),
            "score": torch.where(won, flat.gather(1, best.unsqueeze(1)).squeeze(1), torch.full((N,), 1e10, dtype=torch.float64))}


def criterion(v, bits, choice, num=NUM, deploy=True):
    """per row: (the fp64 score of the candidate ``choice`` [N, 2], the smallest fp64 score over all candidates, the candidate's fp32 step)"""
    S, D = scores64(v, bits, num, deploy)
    i, zp = choice[:, 0].long(), choice[:, 1].long()
    rows = torch.arange(S.shape[0])
    return S[rows, i - 1, zp], S.reshape(S.shape[0], -1).min(1)[0], D[rows, i - 1]


def select(W, H, n_out, bits, num=NUM, deploy=True):
    """the column choice: whole-row range search, frob_c = sum over rows of (w - w^)^2, sens = diag(H) * frob; (ids, out_ids ascending, frob, sens)"""
    W = W.float()
    K = W.shape[1]
    got = range_search(W, bits, num, deploy)
    _, wh = deployed(W, got["scale"], got["zero"], float(2 ** bits - 1), deploy)
    frob = ((W - wh) ** 2).sum(0)
    sens = torch.diag(H).float() * frob
    desc = torch.argsort(sens, descending=True, stable=True)
    keep = torch.ones(K, dtype=torch.bool)
    keep[desc[:n_out]] = False
    ids = torch.cat([torch.arange(K)[keep], desc[:n_out]])
    return ids, torch.sort(desc[:n_out])[0].to(torch.int32), frob, sens


def solve(W_p, U_p, n_out, bits, num=NUM, deploy=True, choices=None):
    """W_p fp16 (or fp32 holding the values) [N, K] permuted, U_p fp32 [K, K] upper.  ``choices`` int32 [N, Kp / 128, 2]: replay with these (i, zp)
    per row and group instead of searching.  Returns q int32 [N Kp / 128, 128], scale / zero ([., 1]; fp16 under deploy), W_hat fp32 [N, n_nonout]
    (what the error feedback saw), W_out (fp16 [N, n_out] under deploy, else fp32), dense_p fp32 [N, K] = [W_hat | W_out] in the permuted order,
    row_loss, loss, nonfinite, choice, and segments: the groups' current values at their block's start (the search's inputs)."""
    assert bits in (2, 3, 4)
    W = W_p.detach().float().clone()
    U = U_p.detach().float()
    N, K = W.shape
    assert K % BLOCK == 0 and U.shape == (K, K) and 0 <= n_out < K and n_out % 2 == 0
    nq, Kp = K - n_out, packed_columns(K, n_out)
    G = Kp // BLOCK
    maxq = float(2 ** bits - 1)
    Q = torch.zeros(N, Kp)
    What = torch.zeros(N, nq)
    S, Z = torch.zeros(N, G), torch.zeros(N, G)
    CH = torch.zeros(N, G, 2, dtype=torch.int32)
    loss = torch.zeros(N)
    segments = []
    bad = False
    for i1 in range(0, nq, BLOCK):
        i2, g = min(i1 + BLOCK, nq), i1 // BLOCK
        seg = W[:, i1:i2].clone()
        segments.append(seg)
        if choices is None:
            got = range_search(seg, bits, num, deploy)
            s, z, CH[:, g] = got["scale"], got["zero"], got["choice"]
        else:
            CH[:, g] = choices[:, g]
            xmin, xmax = extremes(seg)
            s = step(xmax - xmin, num, CH[:, g, 0], maxq, deploy)
            z = CH[:, g, 1].float()
        bad = bad or bool((CH[:, g, 0] == 0).any())
        S[:, g], Z[:, g] = s, z
        for i in range(i1, i2):
            w = W[:, i]
            d = U[i, i]
            q = torch.clamp(torch.round(w / s) + z, 0.0, maxq)
            t = (q - z) * s
            wh = t.to(torch.float16).float() if deploy else t
            r = w - wh
            e = r / d
            loss = loss + ((r * r) / (d * d)) / 2.0
            bad = bad or not bool(torch.isfinite(w).all()) or not bool(torch.isfinite(e).all()) or not bool(torch.isfinite(d) and d > 0)
            Q[:, i] = q
            What[:, i] = wh
            if i + 1 < K:
                p = e.unsqueeze(1) * U[i, i + 1:].unsqueeze(0)
                W[:, i + 1:] = W[:, i + 1:] - p
        Q[:, i2:i1 + BLOCK] = z.unsqueeze(1)            # the padding of a ragged last group: the code that dequantizes to 0
    W_out = W[:, nq:].to(torch.float16) if deploy else W[:, nq:].clone()
    bad = bad or not bool(torch.isfinite(W_out.float()).all())
    return {"q": None if bad else Q.reshape(-1, BLOCK).to(torch.int32), "scale": (S.to(torch.float16) if deploy else S).reshape(-1, 1),
            "zero": (Z.to(torch.float16) if deploy else Z).reshape(-1, 1), "W_hat": What, "W_out": W_out,
            "dense_p": torch.cat([What, W_out.float()], 1), "row_loss": loss, "loss": float(loss.double().sum()), "nonfinite": int(bad),
            "choice": CH, "segments": segments}


def unpermute(dense_p, ids):
    """[N, K] in the permuted order -> the original column order"""
    out = torch.empty_like(dense_p)
    out[:, ids] = dense_p
    return out
