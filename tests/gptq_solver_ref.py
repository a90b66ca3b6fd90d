"""GPTQ's error-feedback solve as csrc/amq_gptq.hip computes it (include/amq_hip.h), restated in torch fp32 on the CPU: one torch
op per rounding, all rows at once, the columns one after the other.  Every later column of the whole row receives ``w_j -= e * U[i, j]`` (one
multiply, one subtract) right after column i, so each element sees its subtractions in ascending i -- the order the kernel keeps whatever its
blocking.

``deploy=True`` is the kernel's rule: the scale is rounded to fp16 (floor 2^-24) before it is used and the error feedback sees
``w^ = fp16((q - z) * s16)``, the weight the dequantize and matmul kernels produce.  ``deploy=False`` keeps the fp32 scale and ``w^ = (q - z) * s``:
the reference's own rule (amq/quantization/gptq.py:12-16, 347-387), used only to show that the algorithm is the reference's.
"""
import torch

BLOCK = 128
GROUPS = (32, 64, 128)


def workspace_bytes(N, K, group):
    """include/amq_hip.h amq_gptq_quantize_workspace_bytes: fp32 errors [N, K], int32 flags [N / 4], byte codes [N, K]"""
    if group not in GROUPS or N <= 0 or K <= 0 or N % 16 or K % 128:
        return 0
    return 5 * N * K + N


def _params(x, maxq, deploy):
    """(s, z) [N, 1] of the groups x [N, G] (Quantizer.find_params, asymmetric, no grid search)"""
    zero = torch.zeros(x.shape[0])
    xmin = torch.minimum(x.min(1)[0], zero)
    xmax = torch.maximum(x.max(1)[0], zero)
    both = (xmin == 0) & (xmax == 0)
    xmin = torch.where(both, torch.full_like(xmin, -1.0), xmin)
    xmax = torch.where(both, torch.full_like(xmax, 1.0), xmax)
    s = (xmax - xmin) / maxq
    if deploy:
        s = torch.clamp(s.to(torch.float16).float(), min=2.0 ** -24)
    z = torch.round(-xmin / s)
    return s.unsqueeze(1), z.unsqueeze(1)


def solve(W, U, bits, group=128, deploy=True):
    """W fp16 (or fp32 holding the values) [N, K], U fp32 [K, K] upper.  Returns q int32 [R, group] (Format A's groups before packing), scale, zero
    fp16 [R, 1] (deploy) or fp32, W_hat fp32 [N, K] (the weights the error feedback saw), row_loss fp32 [N], loss (its fp64 sum), nonfinite."""
    assert group in GROUPS and bits in (2, 3, 4)
    W = W.detach().float().clone()
    U = U.detach().float()
    N, K = W.shape
    assert K % BLOCK == 0 and U.shape == (K, K)
    maxq = float(2 ** bits - 1)
    Q = torch.zeros(N, K)
    What = torch.zeros(N, K)
    S = torch.zeros(N, K // group)
    Z = torch.zeros(N, K // group)
    loss = torch.zeros(N)
    bad = False
    for i1 in range(0, K, BLOCK):
        for g0 in range(i1, i1 + BLOCK, group):        # every group of the block from the block-start values
            s, z = _params(W[:, g0:g0 + group], maxq, deploy)
            S[:, g0 // group:g0 // group + 1] = s
            Z[:, g0 // group:g0 // group + 1] = z
        for i in range(i1, i1 + BLOCK):
            w = W[:, i]
            s, z = S[:, i // group], Z[:, i // group]
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
    out = {"W_hat": What, "row_loss": loss, "loss": float(loss.double().sum()), "nonfinite": int(bad)}
    if bad:
        out["q"] = None
    else:
        out["q"] = Q.reshape(-1, group).to(torch.int32)
    out["scale"] = (S.to(torch.float16) if deploy else S).reshape(-1, 1)
    out["zero"] = (Z.to(torch.float16) if deploy else Z).reshape(-1, 1)
    return out


def hessian(X, window=64):
    """fp64 H = 2 / n * X^T X of the calibration rows X [T, K] delivered as n = ceil(T / window) sequences: what GPTQ_METHOD.add_batch
    accumulates in fp32 (it divides by the number of sequences, not of rows)"""
    X = X.double()
    return 2.0 / -(-X.shape[0] // window) * (X.t() @ X)


def proxy_loss(W, What, H):
    """tr(dW H dW^T) in fp64"""
    d = W.double() - What.double()
    return float(((d @ H) * d).sum())


def hinv_upper(H32, percdamp=0.01):
    """the reference's own three linalg calls (gptq.py:226-253) on an fp32 H: (U, dead)"""
    H = H32.clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    damp = percdamp * torch.mean(torch.diag(H))
    idx = torch.arange(H.shape[0])
    H[idx, idx] += damp
    H = torch.linalg.cholesky(H)
    H = torch.cholesky_inverse(H)
    return torch.linalg.cholesky(H, upper=True), dead
