"""GPTQ's solve with static groups and an activation order as csrc/amq_gptq_static.hip computes it (include/amq_hip.h), restated in
torch fp32 on the CPU: one torch op per rounding, all rows at once, the walk columns one after the other.  Every group's (s, z) comes from W's
original, consecutive columns before the solve (gptq_solver_ref._params: the plain solve's parameter arithmetic); walk column i is original column
``perm[i]`` and quantizes with the parameters of group ``perm[i] // group``; every later walk column receives ``w_j -= e * U[i, j]`` (one multiply,
one subtract) right after walk column i, so each element sees its subtractions in ascending walk index; the results leave in W's own column order.
``U`` is the factor of the permuted Hessian.  ``deploy`` as in gptq_solver_ref: True is the kernel's rule (fp16 scale with the 2^-24 floor, the
error feedback sees ``fp16((q - z) * s16)``), False the reference's own (amq/quantization/gptq.py:230-242, 270-277, 304-305).
"""
import torch

import gptq_solver_ref as plain

BLOCK, GROUPS = plain.BLOCK, plain.GROUPS
workspace_bytes = plain.workspace_bytes          # include/amq_hip.h amq_gptq_quantize_static_workspace_bytes: the plain solve's


def act_order(H):
    """gptq.py:226-227, 239 with a stable sort: the columns by descending diag(H), dead ones ranking as 1, ties to the lower column"""
    d = torch.diag(H).float().clone()
    d[d == 0] = 1
    return torch.sort(d, descending=True, stable=True)[1]


def static_params(W, bits, group, deploy=True):
    """(S, Z) fp32 [N, K / group] from W's original groups"""
    W = W.detach().float()
    N, K = W.shape
    maxq = float(2 ** bits - 1)
    S, Z = torch.zeros(N, K // group), torch.zeros(N, K // group)
    for g in range(K // group):
        s, z = plain._params(W[:, g * group:(g + 1) * group], maxq, deploy)
        S[:, g:g + 1], Z[:, g:g + 1] = s, z
    return S, Z


def solve(W, U, perm, bits, group=128, deploy=True):
    """W fp16 (or fp32 holding the values) [N, K] in its own column order, U fp32 [K, K] upper (of the permuted Hessian), perm integer [K].  Returns
    what gptq_solver_ref.solve returns, in W's own column order: q int32 [R, group], scale, zero fp16 [R, 1] (deploy) or fp32, W_hat fp32 [N, K],
    row_loss fp32 [N], loss, nonfinite."""
    assert group in GROUPS and bits in (2, 3, 4)
    W = W.detach().float()
    U = U.detach().float()
    N, K = W.shape
    perm = perm.to(torch.int64)
    assert K % BLOCK == 0 and U.shape == (K, K) and torch.equal(torch.sort(perm)[0], torch.arange(K))
    maxq = float(2 ** bits - 1)
    S, Z = static_params(W, bits, group, deploy)
    Wp = W[:, perm].clone()
    Q = torch.zeros(N, K)
    What = torch.zeros(N, K)
    loss = torch.zeros(N)
    bad = False
    for i in range(K):
        col = int(perm[i])
        w = Wp[:, i]
        s, z = S[:, col // group], Z[:, col // group]
        d = U[i, i]
        q = torch.clamp(torch.round(w / s) + z, 0.0, maxq)
        t = (q - z) * s
        wh = t.to(torch.float16).float() if deploy else t
        r = w - wh
        e = r / d
        loss = loss + ((r * r) / (d * d)) / 2.0
        bad = bad or not bool(torch.isfinite(w).all()) or not bool(torch.isfinite(e).all()) or not bool(torch.isfinite(d) and d > 0)
        Q[:, col] = q
        What[:, col] = wh
        if i + 1 < K:
            p = e.unsqueeze(1) * U[i, i + 1:].unsqueeze(0)
            Wp[:, i + 1:] = Wp[:, i + 1:] - p
    out = {"W_hat": What, "row_loss": loss, "loss": float(loss.double().sum()), "nonfinite": int(bad)}
    out["q"] = None if bad else Q.reshape(-1, group).to(torch.int32)
    out["scale"] = (S.to(torch.float16) if deploy else S).reshape(-1, 1)
    out["zero"] = (Z.to(torch.float16) if deploy else Z).reshape(-1, 1)
    return out
