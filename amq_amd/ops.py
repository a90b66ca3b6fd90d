"""Tensor-level wrappers over the C ABI: one function per operation.  Where the ABI has several entry points for one operation (the forms of
the decode-step attention and token tails, the `_qkn` twins), the function chooses among them by its arguments.

All tensors must live on a HIP device; inputs are validated on the host before
a kernel is launched (shape/dtype/contiguity), because an out-of-bounds access
in a hand-written kernel can take the GPU down.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import (MODE_HQQ, MODE_FMA, MODE_FMA1, PRO_NONE, PRO_RMSNORM, PRO_SILU_MUL, Segment, GemvOpts, EngineBlock, EngineLinear,  # noqa: F401
                   GEMM_AUTO, GEMM_TILED, GEMM_SKINNY, GEMM_RING, GEMM_RING128, GEMM_WS, GEMM_DEQ, MATH_DEFAULT, MATH_EXACT, MATH_LINEAR, MATH_GROUPSCALE)

GROUP = 128


def _need(t, dtype, name, numel=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a tensor on the GPU")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name}: expected {numel} elements, got {t.numel()}")


FINE_GROUPS = (64, 32)      # groups finer than the native tile: 128 / group (scale, zero) pairs per (row, tile) in the native meta


def native_group(group):
    """granularity of the NATIVE meta for a source-format group size: 128 for 128 and its multiples (pairs replicated), else the group"""
    return int(group) if int(group) in FINE_GROUPS else GROUP


def native_sizes(bits, N, K, group=GROUP):
    lib = _lib.load()
    return int(lib.amq_native_qweight_bytes(bits, N, K)), int(lib.amq_native_meta_bytes(N, K, native_group(group)))


def alloc_native(bits, N, K, device, group=GROUP, meta_dtype=torch.float16):
    qb, mb = native_sizes(bits, N, K, group)
    return (torch.empty(qb // 4, dtype=torch.int32, device=device),
            torch.empty(mb // 2, dtype=meta_dtype, device=device))


def _check_shape(bits, N, K):
    if bits not in (2, 3, 4):
        raise ValueError(f"bits must be 2, 3 or 4 (got {bits})")
    if N % 16 or K % 128 or N <= 0 or K <= 0:
        raise ValueError(f"need N % 16 == 0 and K % 128 == 0 (got N={N}, K={K})")


def _check_group(group, K):
    """source-format group sizes the repack kernels read: 128 or a multiple of it that divides K (each group's (scale, zero) is
    replicated into the native layout's per-128 pairs), or 64 / 32 (128 / group pairs per native tile row)"""
    group = int(group)
    if group in FINE_GROUPS:
        return group
    if group < GROUP or group % GROUP or K % group:
        raise ValueError(f"group size must be 32, 64 or a multiple of {GROUP} that divides K={K} (got {group})")
    return group


def repack_from_hqq(W_q, scale, zero, bits, N, K, group=GROUP):
    """HQQLinear.W_q + meta['scale'|'zero'] -> (qweight_native, meta_native), MODE_HQQ."""
    _check_shape(bits, N, K)
    group = _check_group(group, K)
    lib = _lib.load()
    R = N * K // group
    if bits == 3:
        _need(W_q, torch.int32, "W_q", ((R + 9) // 10) * group)
    else:
        _need(W_q, torch.uint8, "W_q", R * group * bits // 8)
    # compute_dtype = bfloat16 models (quantize.py:516): the repack copies 16-bit patterns, the native meta is then a bfloat16 tensor and only the
    # *_bf16 entry points take it (the tensor's dtype is the tag the C ABI does not carry)
    meta_dtype = torch.bfloat16 if isinstance(scale, torch.Tensor) and scale.dtype == torch.bfloat16 else torch.float16
    if meta_dtype == torch.bfloat16 and group in FINE_GROUPS:
        raise ValueError("bfloat16 meta: groups of 128 (and multiples) only")
    _need(scale, meta_dtype, "scale", R)
    _need(zero, meta_dtype, "zero", R)
    qn, mn = alloc_native(bits, N, K, W_q.device, group, meta_dtype)
    _lib.check(lib.amq_repack_from_hqq(bits, _lib.ptr(W_q), _lib.ptr(scale), _lib.ptr(zero), N, K, group,
                                       _lib.ptr(qn), _lib.ptr(mn), _lib.current_stream()))
    return qn, mn


def repack_from_gptq(qweight, scales, zeros, bits, N, K, group=GROUP):
    """GPTQLinear buffers -> native, MODE_FMA."""
    _check_shape(bits, N, K)
    group = _check_group(group, K)
    lib = _lib.load()
    _need(qweight, torch.int32, "qweight", K // 32 * bits * N)
    _need(scales, torch.float32, "scales", K // group * N)
    _need(zeros, torch.float32, "zeros", K // group * N)
    qn, mn = alloc_native(bits, N, K, qweight.device, group)
    _lib.check(lib.amq_repack_from_gptq(bits, _lib.ptr(qweight), _lib.ptr(scales), _lib.ptr(zeros), N, K, group,
                                        _lib.ptr(qn), _lib.ptr(mn), _lib.current_stream()))
    return qn, mn


def repack_from_awq(qweight, scales, scaled_zeros, N, K, group=GROUP):
    """FT_QuantLinear buffers (4 bit) -> native, MODE_FMA."""
    _check_shape(4, N, K)
    group = _check_group(group, K)
    if N % 4 or K % 64:
        raise ValueError("AWQ pack needs N % 4 == 0 and K % 64 == 0")
    lib = _lib.load()
    _need(qweight, torch.int16, "qweight", N // 4 * K)
    _need(scales, torch.float16, "scales", K // group * N)
    _need(scaled_zeros, torch.float16, "scaled_zeros", K // group * N)
    qn, mn = alloc_native(4, N, K, qweight.device, group)
    _lib.check(lib.amq_repack_from_awq(_lib.ptr(qweight), _lib.ptr(scales), _lib.ptr(scaled_zeros), N, K, group,
                                       _lib.ptr(qn), _lib.ptr(mn), _lib.current_stream()))
    return qn, mn


# ---------------------------------------------------------------------------------------------------------------- the device quantizers
QUANTIZE_GROUPS = (32, 64, 128, 256)      # group sizes the quantizer's solve kernel is built for
GPTQ_GROUPS = (32, 64, 128)      # group sizes the GPTQ solve kernel is built for: those that fit its 128-column block
AWQ_GROUPS = (32, 64, 128)       # group sizes the AWQ kernels are built for


def _format_a_buffers(N, K, nbits, group, device):
    """(W_q, scale, zero) of Format A for a layer [N, K]: R = N K / group rows of codes as int32 [(R + 9) // 10, group] (3 bit) or uint8
    [R nbits // 8, group], scale and zero fp16 [R, 1]"""
    R = N * K // group
    if nbits == 3:
        W_q = torch.empty((R + 9) // 10, group, dtype=torch.int32, device=device)
    else:
        W_q = torch.empty(R * nbits // 8, group, dtype=torch.uint8, device=device)
    return W_q, torch.empty(R, 1, dtype=torch.float16, device=device), torch.empty(R, 1, dtype=torch.float16, device=device)


def _dense_f16(t, who):
    """a dense 2-d operand at the boundary: on the GPU, fp16 (bf16 / fp32 are cast, as the reference's ``.half()`` does before it quantizes)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2:
        raise ValueError(f"{who}: expected a 2-d tensor on the GPU")
    if t.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"{who}: expected fp16 (or bf16 / fp32, cast to fp16), got {t.dtype}")
    return t.detach().to(torch.float16).contiguous()


def _quantize_shape(N, K, nbits, group_size, groups, serves):
    """a quantizer family's shape check: ``groups`` are what its kernels are built for, ``serves`` is how it says so; returns the group as int"""
    _check_shape(nbits, N, K)
    if int(group_size) not in groups or K % int(group_size):
        raise ValueError(f"{serves} (got {group_size})")
    return int(group_size)


def _workspace_words(query, who, **shape):
    """what the C ABI's workspace query answers for ``shape`` (its arguments, in order) in int32 words; 0 bytes is its refusal"""
    need = int(getattr(_lib.load(), query)(*shape.values()))
    if need <= 0:
        raise ValueError(f"{who} refuses " + ", ".join(f"{k}={v}" for k, v in shape.items()))
    return (need + 3) // 4


def _refuse_nonfinite(nonfinite, who, name, what):
    if nonfinite:
        raise ValueError(f"{who}: {'layer ' + name if name else 'W'}{what}")


def _info_block(nbytes, device):
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device)


def _nbytes(t):
    return t.numel() * t.element_size()


class HQQQuantizeInfo:
    """the info block of one ``hqq_quantize`` call, read back: ``stop`` (the iteration whose zero was kept, 0 .. 19), ``nonfinite`` and
    ``mean_err`` (the tensor's mean |W - W_r| at the start of each of the 20 iterations, fp32)"""

    def __init__(self, block):
        self.stop = int(block[0].item())
        self.nonfinite = int(block[1].item())
        self.mean_err = block[2:].view(torch.float32).clone()

    def __repr__(self):
        return f"HQQQuantizeInfo(stop={self.stop}, nonfinite={self.nonfinite}, mean_err[0]={float(self.mean_err[0]):.6g})"


def hqq_quantize_launch(W, nbits, group_size, round_zero, W_q, scale, zero, info, workspace):
    """the bare entry point over caller-owned buffers (three launches on the current stream; no allocation, no read-back: capturable)"""
    N, K = W.shape
    _lib.check(_lib.load().amq_hqq_quantize_f16(_lib.ptr(W), N, K, int(nbits), int(group_size), int(bool(round_zero)), _lib.ptr(W_q), _lib.ptr(scale),
                                                _lib.ptr(zero), _lib.ptr(info), _lib.ptr(workspace), _nbytes(workspace), _lib.current_stream()))


def hqq_quantize_buffers(N, K, nbits, group_size, device):
    """(W_q, scale, zero, info, workspace) of the right sizes for ``hqq_quantize_launch``"""
    group_size = _quantize_shape(N, K, nbits, group_size, QUANTIZE_GROUPS, f"the quantizer serves groups of 32, 64, 128 and 256 that divide K={K}")
    words = _workspace_words("amq_hqq_quantize_workspace_bytes", "the quantizer", N=N, K=K, group=group_size)
    return (*_format_a_buffers(N, K, nbits, group_size, device), _info_block(_lib.HQQ_INFO_BYTES, device), _quantize_scratch.get(device, words))


def hqq_quantize(W, nbits, group_size=GROUP, round_zero=None, return_info=False, bias=None, name=None):
    """Dense W [N, K] on the GPU -> HQQWeights (Format A) on the same device: the reference's ``Quantizer.quantize`` with its proximal solver
    (axis 1, lp_norm 0.7, beta 10, 20 iterations, early stop) in the fp32 arithmetic of its CPU path, as HIP kernels.  W is fp16 (bf16 / fp32 weights
    are cast at this boundary, as the reference's ``.half()`` does before it quantizes).  ``round_zero`` defaults to ``nbits == 4`` (the reference's
    hqq_base_quant_config).  Raises ValueError if W holds an inf or NaN.  One synchronising read of the 88-byte info block per call.
    ``return_info``: also return the :class:`HQQQuantizeInfo`."""
    from .hqq_format import HQQWeights
    W = _dense_f16(W, "W")
    N, K = W.shape
    nbits = int(nbits)
    if round_zero is None:
        round_zero = nbits == 4
    W_q, scale, zero, info, workspace = hqq_quantize_buffers(N, K, nbits, group_size, W.device)
    hqq_quantize_launch(W, nbits, group_size, round_zero, W_q, scale, zero, info, workspace)
    got = HQQQuantizeInfo(info.cpu())
    _refuse_nonfinite(got.nonfinite, "hqq_quantize", name, " holds inf or NaN values")
    h = HQQWeights(W_q, scale, zero, nbits, (N, K), int(group_size), bias, name)
    return (h, got) if return_info else h


class GPTQHessian:
    """The running Hessian of one linear's inputs, the reference's form (amq/quantization/gptq.py:199-204) as torch fp32 ops on ``device``:
    ``H <- H * n / (n + b); n += b; H += (sqrt(2 / n) x)^T (sqrt(2 / n) x)`` per batch of b sequences, x the batch's rows [b * seqlen, K]."""

    def __init__(self, K, device):
        self.H = torch.zeros(int(K), int(K), dtype=torch.float32, device=device)
        self.nsamples = 0

    def add_batch(self, x):
        if x.dim() == 2:
            x = x.unsqueeze(0)
        b = x.shape[0]
        x = x.reshape(-1, x.shape[-1]).t()
        self.H *= self.nsamples / (self.nsamples + b)
        self.nsamples += b
        x = (2.0 / self.nsamples) ** 0.5 * x.float()
        self.H += x.matmul(x.t())


def gptq_hinv(H, percdamp=0.01, name=None, return_where=False):
    """(U, dead): the upper Cholesky factor of the damped inverse of H (gptq.py:224-253: dead columns get a unit diagonal, the diagonal is damped
    by ``percdamp`` of its mean, then cholesky, cholesky_inverse, cholesky(upper)) and the bool mask of the dead columns.  H is not modified.
    ``torch.linalg`` runs on H's device; a build that lacks the factorisation there runs it on the host and brings U back
    (``return_where``: also return ``'device'`` or ``'host'``).  A failed factorisation raises ValueError naming the layer."""
    H = H.detach().to(torch.float32).clone()
    dead = torch.diag(H) == 0
    idx = torch.arange(H.shape[0], device=H.device)
    H[idx, idx] = torch.where(dead, torch.ones_like(H[idx, idx]), H[idx, idx])
    H[idx, idx] += percdamp * torch.mean(torch.diag(H))

    def factor(A):
        A = torch.linalg.cholesky(A)
        A = torch.cholesky_inverse(A)
        return torch.linalg.cholesky(A, upper=True)

    where = "device" if H.is_cuda else "host"
    try:
        try:
            U = factor(H)
        except RuntimeError as e:
            if isinstance(e, torch.linalg.LinAlgError) or not H.is_cuda:
                raise
            where = "host"                      # (a build without the device solver library)
            U = factor(H.cpu()).to(H.device)
    except torch.linalg.LinAlgError as e:
        raise ValueError(f"gptq_hinv: the damped Hessian of {'layer ' + name if name else 'the layer'} is not positive definite ({e})") from None
    U = U.contiguous()
    return (U, dead, where) if return_where else (U, dead)


class GPTQQuantizeInfo:
    """what one ``gptq_quantize`` call reports: ``nonfinite`` (the info block), ``row_loss`` (fp32 [N], on the device) and ``loss``, its fp64 sum
    (the reference's printed ``error``)"""

    def __init__(self, nonfinite, row_loss):
        self.nonfinite = int(nonfinite)
        self.row_loss = row_loss
        self.loss = float(row_loss.double().sum().item())

    def __repr__(self):
        return f"GPTQQuantizeInfo(nonfinite={self.nonfinite}, loss={self.loss:.6g})"


def gptq_quantize_launch(W, U, nbits, group_size, W_q, scale, zero, row_loss, info, workspace):
    """the bare entry point over caller-owned buffers (three launches on the current stream; no allocation, no read-back: capturable)"""
    N, K = W.shape
    _lib.check(_lib.load().amq_gptq_quantize_f16(_lib.ptr(W), _lib.ptr(U), N, K, int(nbits), int(group_size), _lib.ptr(W_q), _lib.ptr(scale),
                                                 _lib.ptr(zero), _lib.ptr(row_loss), _lib.ptr(info), _lib.ptr(workspace), _nbytes(workspace),
                                                 _lib.current_stream()))


def gptq_quantize_buffers(N, K, nbits, group_size, device, query="amq_gptq_quantize_workspace_bytes"):
    """(W_q, scale, zero, row_loss, info, workspace) of the right sizes for ``gptq_quantize_launch``"""
    serves = "the GPTQ solve serves groups of 32, 64 and 128"
    if int(group_size) == 256:
        serves += ": a group of 256 would span two of its 128-column blocks"
    group_size = _quantize_shape(N, K, nbits, group_size, GPTQ_GROUPS, serves)
    words = _workspace_words(query, "the GPTQ solve", N=N, K=K, group=group_size)
    return (*_format_a_buffers(N, K, nbits, group_size, device), torch.empty(N, dtype=torch.float32, device=device),
            _info_block(_lib.GPTQ_INFO_BYTES, device), _gptq_scratch.get(device, words))


def gptq_act_order(H):
    """The reference's activation order of a Hessian H [K, K] (gptq.py:226-227, 239): ``perm`` (int64 [K], on H's device) = the columns by
    descending ``diag(H)``, a dead column (diagonal 0) ranking as 1.  The sort is stable, so ties go to the lower column: the reference's ``perm``
    wherever the diagonal has no ties.  Walk column i of ``gptq_quantize(..., perm=perm, static_groups=True)`` is column ``perm[i]``, and its
    ``U`` is ``gptq_hinv(H[perm][:, perm])``."""
    d = torch.diag(H.detach()).to(torch.float32)
    d = torch.where(d == 0, torch.ones_like(d), d)
    return torch.sort(d, descending=True, stable=True)[1]


def _gptq_perm(perm, K, device):
    """``gptq_quantize``'s ``perm`` as the entry point takes it (int32 [K], contiguous, on ``device``), validated on the host before any launch"""
    if not isinstance(perm, torch.Tensor) or perm.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"perm: expected an int32 or int64 tensor, got {getattr(perm, 'dtype', type(perm).__name__)}")
    if perm.device != device:
        raise ValueError(f"perm: expected a tensor on W's GPU ({device}), got {perm.device}")
    if tuple(perm.shape) != (K,):
        raise ValueError(f"perm: expected shape ({K},), got {tuple(perm.shape)}")
    if not torch.equal(torch.sort(perm.to(torch.int64))[0], torch.arange(K, dtype=torch.int64, device=device)):
        raise ValueError(f"perm: not a permutation of 0 .. {K - 1}")
    return perm.to(torch.int32).contiguous()


def gptq_quantize_static_launch(W, U, perm, nbits, group_size, W_q, scale, zero, row_loss, info, workspace):
    """the bare entry point of the static-groups solve over caller-owned buffers (four launches on the current stream; no allocation, no
    read-back: capturable).  ``perm``: int32 [K], a permutation -- the entry point cannot check it (``gptq_quantize`` does)."""
    N, K = W.shape
    _lib.check(_lib.load().amq_gptq_quantize_static_f16(_lib.ptr(W), _lib.ptr(U), _lib.ptr(perm), N, K, int(nbits), int(group_size),
                                                        _lib.ptr(W_q), _lib.ptr(scale), _lib.ptr(zero), _lib.ptr(row_loss), _lib.ptr(info),
                                                        _lib.ptr(workspace), _nbytes(workspace), _lib.current_stream()))


def gptq_quantize_static_buffers(N, K, nbits, group_size, device):
    """(W_q, scale, zero, row_loss, info, workspace) of the right sizes for ``gptq_quantize_static_launch`` (the plain solve's sizes)"""
    return gptq_quantize_buffers(N, K, nbits, group_size, device, query="amq_gptq_quantize_static_workspace_bytes")


def gptq_quantize(W, U, nbits, group_size=GROUP, return_info=False, bias=None, name=None, perm=None, static_groups=False):
    """Dense W [N, K] and U [K, K] (``gptq_hinv``: fp32, the upper Cholesky factor of the damped inverse Hessian) on the GPU -> HQQWeights (Format
    A) on the same device by GPTQ's error-feedback solve (gptq.py:206-311: asymmetric, grouped, blocks of 128 columns) as HIP kernels, in the
    arithmetic include/amq_hip.h states: the scale is rounded to fp16 before it is used and the error feedback sees the weight the packed layer
    will dequantize to.  W is fp16 (bf16 / fp32 weights are cast at this boundary); the caller has zeroed its dead columns.  Raises ValueError if a
    weight, an error or U's diagonal was not finite (or the diagonal not positive).  One synchronising read of the 4-byte info block per call.
    ``return_info``: also return the :class:`GPTQQuantizeInfo`.

    ``static_groups=True``: every group's (scale, zero) is fixed from W's original columns before the solve (gptq.py:230-236).  With it,
    ``perm`` (an integer tensor [K] on W's device, a permutation of 0 .. K - 1, e.g. ``gptq_act_order(H)``) makes the solve walk the columns in
    that order -- the reference's ``actorder=True, static_groups=True`` -- and U must be the factor of the equally permuted Hessian,
    ``gptq_hinv(H[perm][:, perm])``.  W stays in its own order and so does the packed result: an ordinary Format A layer.  ``perm`` is validated
    before any launch (ValueError).  ``perm`` without ``static_groups`` raises NotImplementedError: groups formed over the permuted columns are not
    a Format A layer (it would need a gather at run time)."""
    from .hqq_format import HQQWeights
    if perm is not None and not static_groups:
        raise NotImplementedError("gptq_quantize: an activation order without static groups forms its groups over the permuted columns, which is "
                                  "not a Format A layer (it would need a gather of x at run time); pass static_groups=True")
    W = _dense_f16(W, "W")
    N, K = W.shape
    if not isinstance(U, torch.Tensor) or U.device != W.device:
        raise ValueError("U: expected a tensor on W's GPU")
    U = U.detach().contiguous()                # (cholesky(upper=True) hands out a transposed view)
    _need(U, torch.float32, "U", K * K)
    nbits = int(nbits)
    if static_groups:
        perm = torch.arange(K, dtype=torch.int32, device=W.device) if perm is None else _gptq_perm(perm, K, W.device)
        W_q, scale, zero, row_loss, info, workspace = gptq_quantize_static_buffers(N, K, nbits, group_size, W.device)
        gptq_quantize_static_launch(W, U, perm, nbits, group_size, W_q, scale, zero, row_loss, info, workspace)
    else:
        W_q, scale, zero, row_loss, info, workspace = gptq_quantize_buffers(N, K, nbits, group_size, W.device)
        gptq_quantize_launch(W, U, nbits, group_size, W_q, scale, zero, row_loss, info, workspace)
    got = GPTQQuantizeInfo(info.cpu()[0].item(), row_loss)
    _refuse_nonfinite(got.nonfinite, "gptq_quantize", name, ": a weight, an error or U's diagonal was not finite (or the diagonal not positive)")
    h = HQQWeights(W_q, scale, zero, nbits, (N, K), int(group_size), bias, name)
    return (h, got) if return_info else h


OWQ_NUM = 40                     # delta candidates of OWQ's range search (owq.py:202, 364)
_OWQ_SERVES = "the OWQ kernels serve groups of 128 only"


class OWQRangeInfo:
    """what one ``owq_range`` call reports: ``choice`` (int32 [N, 2]: the winner's (i, zp) per row), ``score`` (fp32 [N]), ``wq_err`` (fp32 [K]: the
    column sums of (w - w^)^2, whole-row calls only, else None) and ``nonfinite`` (some row ended without a winner)"""

    def __init__(self, nonfinite, choice, score, wq_err):
        self.nonfinite, self.choice, self.score, self.wq_err = int(nonfinite), choice, score, wq_err

    def __repr__(self):
        return f"OWQRangeInfo(nonfinite={self.nonfinite}, rows={self.score.numel()})"


def owq_range_launch(W, col0, L, nbits, num, scale, zero, choice, score, wq_err, info):
    """the bare entry point over caller-owned buffers (``wq_err`` may be None; up to three launches on the current stream; no allocation, no
    read-back: capturable)"""
    N, K = W.shape
    _lib.check(_lib.load().amq_owq_range_f16(_lib.ptr(W), N, K, int(col0), int(L), int(nbits), int(num), _lib.ptr(scale), _lib.ptr(zero),
                                             _lib.ptr(choice), _lib.ptr(score), _lib.ptr(wq_err), _lib.ptr(info), _lib.current_stream()))


def owq_range_buffers(N, K, device, wq_err=False):
    """(scale, zero, choice, score, wq_err, info) of the right sizes for ``owq_range_launch``"""
    return (torch.empty(N, dtype=torch.float16, device=device), torch.empty(N, dtype=torch.float16, device=device),
            torch.empty(N, 2, dtype=torch.int32, device=device), torch.empty(N, dtype=torch.float32, device=device),
            torch.empty(K, dtype=torch.float32, device=device) if wq_err else None, _info_block(_lib.OWQ_INFO_BYTES, device))


def owq_range(W, nbits, col0=0, L=None, num=OWQ_NUM, return_info=False):
    """OWQ's range search (owq.py Quantizer.find_params with mse, asymmetric, per channel) of the segment ``W[n, col0 : col0 + L]`` of every row of
    the dense W [N, K] on the GPU, as a HIP kernel in the arithmetic include/amq_hip.h states: ``num`` x 2^nbits (delta, zero-point) candidates
    under the lp-2.4 loss of the deployed weight.  Returns (scale, zero) fp16 [N] -- with ``return_info`` also the :class:`OWQRangeInfo`, whose
    ``wq_err`` a whole-row call (col0 = 0, L = K) fills.  Raises ValueError if a row holds an inf or NaN.  One synchronising read per call."""
    W = _dense_f16(W, "W")
    N, K = W.shape
    _check_shape(int(nbits), N, K)
    L = K - int(col0) if L is None else int(L)
    if not 1 <= int(num) <= 100:
        raise ValueError(f"owq_range: num must be 1..100 (got {num})")
    if col0 < 0 or L < 1 or col0 + L > K:
        raise ValueError(f"owq_range: the segment col0={col0}, L={L} does not lie inside K={K}")
    scale, zero, choice, score, wq_err, info = owq_range_buffers(N, K, W.device, wq_err=(col0 == 0 and L == K))
    owq_range_launch(W, col0, L, nbits, num, scale, zero, choice, score, wq_err, info)
    got = OWQRangeInfo(info.cpu()[0].item(), choice, score, wq_err)
    _refuse_nonfinite(got.nonfinite, "owq_range", None, " holds inf or NaN values")
    return (scale, zero, got) if return_info else (scale, zero)


def owq_select(W, H, n_out, nbits, num=OWQ_NUM):
    """OWQ's column choice (owq.py:197-207, hessian_sorting with frob_norm, actorder=False): the whole-row range pass gives frob_c = the column sums
    of (w - w^)^2, sens_c = diag(H)_c * frob_c, the ``n_out`` columns of largest sens are the outliers.  Returns (ids int64 [K]: the kept columns
    ascending, then the outliers in descending sens; out_ids int32 [n_out]: the outliers ascending), on W's device."""
    W = _dense_f16(W, "W")
    N, K = W.shape
    n_out = int(n_out)
    if n_out < 0 or n_out % 2 or n_out >= K:
        raise ValueError(f"owq_select: n_out must be even and in 0 .. K - 2 (got {n_out}, K={K})")
    if not isinstance(H, torch.Tensor) or H.device != W.device or tuple(H.shape) != (K, K):
        raise ValueError("H: expected a [K, K] tensor on W's GPU")
    every = torch.arange(K, device=W.device)
    if n_out == 0:
        return every, torch.empty(0, dtype=torch.int32, device=W.device)
    _, _, info = owq_range(W, nbits, num=num, return_info=True)
    sens = torch.diag(H).to(torch.float32) * info.wq_err
    desc = torch.argsort(sens, descending=True, stable=True)
    keep = torch.ones(K, dtype=torch.bool, device=W.device)
    keep[desc[:n_out]] = False
    return torch.cat([every[keep], desc[:n_out]]), torch.sort(desc[:n_out])[0].to(torch.int32)


class OWQQuantizeInfo:
    """what one ``owq_quantize`` call reports: ``nonfinite`` (the info block), ``choice`` (int32 [N, Kp / 128, 2]: the winner's (i, zp) per row and
    group), ``row_loss`` (fp32 [N], on the device) and ``loss``, its fp64 sum"""

    def __init__(self, nonfinite, choice, row_loss):
        self.nonfinite, self.choice, self.row_loss = int(nonfinite), choice, row_loss
        self.loss = float(row_loss.double().sum().item())

    def __repr__(self):
        return f"OWQQuantizeInfo(nonfinite={self.nonfinite}, loss={self.loss:.6g})"


def owq_packed_columns(K, n_out):
    """Kp: the quantized columns K - n_out padded to whole groups of 128"""
    return -(-(K - n_out) // GROUP) * GROUP


def owq_quantize_launch(W_p, U_p, n_out, nbits, group_size, num, W_q, scale, zero, W_out, choice, row_loss, info, workspace):
    """the bare entry point over caller-owned buffers (three launches on the current stream; no allocation, no read-back: capturable)"""
    N, K = W_p.shape
    _lib.check(_lib.load().amq_owq_quantize_f16(_lib.ptr(W_p), _lib.ptr(U_p), N, K, int(n_out), int(nbits), int(group_size), int(num),
                                                _lib.ptr(W_q), _lib.ptr(scale), _lib.ptr(zero), _lib.ptr(W_out) if n_out else None,
                                                _lib.ptr(choice), _lib.ptr(row_loss), _lib.ptr(info), _lib.ptr(workspace), _nbytes(workspace),
                                                _lib.current_stream()))


def owq_quantize_buffers(N, K, n_out, nbits, group_size, device):
    """(W_q, scale, zero, W_out, choice, row_loss, info, workspace) of the right sizes for ``owq_quantize_launch``"""
    group_size = _quantize_shape(N, K, nbits, group_size, (GROUP,), _OWQ_SERVES)
    n_out = int(n_out)
    if n_out < 0 or n_out % 2 or n_out >= K:
        raise ValueError(f"owq_quantize: n_out must be even and in 0 .. K - 2 (got {n_out}, K={K})")
    Kp = owq_packed_columns(K, n_out)
    words = _workspace_words("amq_owq_quantize_workspace_bytes", "the OWQ solve", N=N, K=K, n_out=n_out, group=group_size)
    return (*_format_a_buffers(N, Kp, nbits, group_size, device), torch.empty(N, n_out, dtype=torch.float16, device=device),
            torch.empty(N, Kp // GROUP, 2, dtype=torch.int32, device=device), torch.empty(N, dtype=torch.float32, device=device),
            _info_block(_lib.OWQ_INFO_BYTES, device), _owq_scratch.get(device, words))


def owq_quantize(W_p, U_p, n_out, nbits, group_size=GROUP, num=OWQ_NUM, return_info=False, bias=None, name=None):
    """OWQ's solve (owq.py:312-391 with grouping, actorder=False) as HIP kernels in the arithmetic include/amq_hip.h states.  ``W_p`` [N, K] is the
    dense matrix with its columns permuted (``owq_select``'s ids: the ``n_out`` outliers last) and its dead columns zeroed, ``U_p`` [K, K] is
    ``gptq_hinv`` of the equally permuted Hessian, both on the GPU.  Returns (HQQWeights of shape (N, Kp) -- the first K - n_out columns quantized
    in groups of 128 with searched ranges, padded with columns that dequantize to 0 --, W_out fp16 [N, n_out]: the outlier columns after the error
    feedback, in W_p's order); with ``return_info`` also the :class:`OWQQuantizeInfo`.  Raises ValueError on non-finite values.  One
    synchronising read of the 4-byte info block per call."""
    from .hqq_format import HQQWeights
    W_p = _dense_f16(W_p, "W_p")
    N, K = W_p.shape
    if not isinstance(U_p, torch.Tensor) or U_p.device != W_p.device:
        raise ValueError("U_p: expected a tensor on W_p's GPU")
    U_p = U_p.detach().contiguous()
    _need(U_p, torch.float32, "U_p", K * K)
    nbits, n_out = int(nbits), int(n_out)
    if not 1 <= int(num) <= 100:
        raise ValueError(f"owq_quantize: num must be 1..100 (got {num})")
    W_q, scale, zero, W_out, choice, row_loss, info, workspace = owq_quantize_buffers(N, K, n_out, nbits, group_size, W_p.device)
    owq_quantize_launch(W_p, U_p, n_out, nbits, group_size, num, W_q, scale, zero, W_out, choice, row_loss, info, workspace)
    got = OWQQuantizeInfo(info.cpu()[0].item(), choice, row_loss)
    _refuse_nonfinite(got.nonfinite, "owq_quantize", name, ": a weight, an error or U's diagonal was not finite (or the diagonal not positive)")
    h = HQQWeights(W_q, scale, zero, nbits, (N, owq_packed_columns(K, n_out)), int(group_size), bias, name)
    return (h, W_out, got) if return_info else (h, W_out)


def owq_gather(x, perm):
    """xg [M, Kp] = x[:, perm] with 0 where perm < 0 (HIPOWQLinear's first launch); x fp16 [M, K] contiguous, perm int32 [Kp]"""
    M, K = x.shape
    Kp = perm.numel()
    xg = torch.empty(M, Kp, dtype=torch.float16, device=x.device)
    _lib.check(_lib.load().amq_owq_gather_f16(_lib.ptr(x), M, K, _lib.ptr(perm), Kp, _lib.ptr(xg), _lib.current_stream()))
    return xg


def owq_outlier_add(x, out_ids, W_out, y):
    """y [M, N] += x[:, out_ids] . W_out^T in place (HIPOWQLinear's last launch: an fp32 fmaf chain per output, one rounding back to fp16)"""
    M, K = x.shape
    N, n_out = W_out.shape
    for lo in range(0, M, 65535):           # (the entry point takes 65535 rows a call: its grid's second dimension)
        rows = min(65535, M - lo)
        _lib.check(_lib.load().amq_owq_outlier_add_f16(_lib.ptr(x[lo:]), rows, K, _lib.ptr(out_ids), n_out, _lib.ptr(W_out), _lib.ptr(y[lo:]), N,
                                                       _lib.current_stream()))
    return y


OWQ_ACT_NONE, OWQ_ACT_RMSNORM, OWQ_ACT_SILU_MUL = _lib.OWQ_ACT_NONE, _lib.OWQ_ACT_RMSNORM, _lib.OWQ_ACT_SILU_MUL
OWQ_STAGE_ROWS = 8


def owq_stage_parts(parts, R, K):
    """the host array of ``owq_stage_launch`` from a list of dicts, one per sibling linear reading the staged activation: an OWQ linear
    {perm int32 [Kp], out_ids int32 [n_out], W_out fp16 [N, n_out], xg fp16 [R, Kp], y fp16 [R, N], residual=None | fp16 [R, N] (may be y)}, a
    plain sibling {xg fp16 [R, K]} alone.  Every shape is checked here: the kernel trusts them."""
    if not 1 <= len(parts) <= _lib.OWQ_MAX_PARTS:
        raise ValueError(f"owq_stage: 1..{_lib.OWQ_MAX_PARTS} parts a launch (got {len(parts)})")
    arr = (_lib.OwqPart * len(parts))()
    for i, p in enumerate(parts):
        W_out = p.get("W_out")
        if W_out is None:
            _need(p["xg"], torch.float16, f"part {i}: xg", R * K)
            arr[i] = _lib.OwqPart(None, None, None, _lib.ptr(p["xg"]), None, None, 0, 0, K)
            continue
        N, n_out = W_out.shape
        Kp = p["perm"].numel()
        _need(W_out, torch.float16, f"part {i}: W_out")
        _need(p["perm"], torch.int32, f"part {i}: perm")
        _need(p["out_ids"], torch.int32, f"part {i}: out_ids", n_out)
        _need(p["xg"], torch.float16, f"part {i}: xg", R * Kp)
        _need(p["y"], torch.float16, f"part {i}: y", R * N)
        res = p.get("residual")
        if res is not None:
            _need(res, torch.float16, f"part {i}: residual", R * N)
        arr[i] = _lib.OwqPart(_lib.ptr(p["perm"]), _lib.ptr(p["out_ids"]), _lib.ptr(W_out), _lib.ptr(p["xg"]), _lib.ptr(p["y"]), _lib.ptr(res),
                              N, n_out, Kp)
    return arr


def owq_stage_launch(x, R, K, act, gamma, eps, x2, arr):
    """the bare entry point over caller-owned buffers and an ``owq_stage_parts`` array (one launch on the current stream; capturable)"""
    _lib.check(_lib.load().amq_owq_stage_f16(_lib.ptr(x), R, K, act, _lib.ptr(gamma), ctypes.c_float(eps), _lib.ptr(x2), arr, len(arr),
                                             _lib.current_stream()))


def owq_stage(x, parts, act=OWQ_ACT_NONE, gamma=None, eps=0.0, x2=None):
    """The token step's stage of OWQ layers (include/amq_hip.h amq_owq_stage_f16): for R = 1 .. 8 rows x [R, K] and a = x (OWQ_ACT_NONE),
    rmsnorm(x, gamma, eps) (OWQ_ACT_RMSNORM) or silu_mul(x, x2) (OWQ_ACT_SILU_MUL), ONE launch leaves per part xg = owq_gather(a, perm) and
    y = the outlier product of a (+ residual), bit for bit what those ops give in composition; ``gemv_grouped(xg, [seg(y, residual=y)], Kp)``
    completes the layer.  ``parts``: see :func:`owq_stage_parts`."""
    x = _prep_x(x, x.shape[-1])
    R, K = x.shape
    if not 1 <= R <= OWQ_STAGE_ROWS:
        raise ValueError(f"owq_stage: 1..{OWQ_STAGE_ROWS} rows (got {R})")
    if act == OWQ_ACT_RMSNORM:
        _need(gamma, torch.float16, "gamma", K)
    elif act == OWQ_ACT_SILU_MUL:
        _need(x2, torch.float16, "x2", R * K)
    elif act != OWQ_ACT_NONE:
        raise ValueError(f"owq_stage: unknown activation {act}")
    owq_stage_launch(x, R, K, act, gamma if act == OWQ_ACT_RMSNORM else None, eps, x2 if act == OWQ_ACT_SILU_MUL else None,
                     owq_stage_parts(parts, R, K))


def _awq_check(N, K, nbits, group_size):
    return _quantize_shape(N, K, nbits, group_size, AWQ_GROUPS, "the AWQ kernels serve groups of 32, 64 and 128")


def awq_quantize_launch(W, nbits, group_size, col_scale, hi, lo, W_q, scale, zero, dense, info, workspace):
    """the bare entry point over caller-owned buffers (``col_scale``, ``hi`` / ``lo``, ``W_q`` / ``scale`` / ``zero`` and ``dense`` may be None; at
    most three launches on the current stream; no allocation, no read-back: capturable)"""
    N, K = W.shape
    _lib.check(_lib.load().amq_awq_quantize_f16(_lib.ptr(W), _lib.ptr(col_scale), _lib.ptr(hi), _lib.ptr(lo), N, K, int(nbits), int(group_size),
                                                _lib.ptr(W_q), _lib.ptr(scale), _lib.ptr(zero), _lib.ptr(dense), _lib.ptr(info),
                                                _lib.ptr(workspace), _nbytes(workspace), _lib.current_stream()))


def awq_quantize_buffers(N, K, nbits, group_size, device, dense=False):
    """(W_q, scale, zero, dense, info, workspace) of the right sizes for ``awq_quantize_launch``: Format A buffers and ``dense`` None, or -- with
    ``dense`` -- the fp16 [N, K] matrix and W_q / scale / zero None"""
    group_size = _awq_check(N, K, nbits, group_size)
    if dense:
        out = (None, None, None, torch.empty(N, K, dtype=torch.float16, device=device))
    else:
        out = (*_format_a_buffers(N, K, nbits, group_size, device), None)
    words = _workspace_words("amq_awq_quantize_workspace_bytes", "the AWQ quantizer", N=N, K=K, group=group_size)
    return (*out, _info_block(_lib.AWQ_INFO_BYTES, device), _awq_scratch.get(device, words))


def awq_quantize(W, nbits, group_size=GROUP, col_scale=None, hi=None, lo=None, dense=False, bias=None, name=None):
    """Dense W [N, K] on the GPU -> HQQWeights (Format A) on the same device by AWQ's round-to-nearest (awq_utils/quantizer.py
    pseudo_quantize_tensor, zero_point=True) in the arithmetic include/amq_hip.h states, as HIP kernels: ``col_scale`` (fp32 [K]) multiplies the
    columns first, ``hi`` / ``lo`` (fp16 [N, K / group], ``awq_clip``) clamp each group before its range is taken.  ``dense``: return instead the
    fp16 [N, K] fake-quantized matrix divided by ``col_scale`` again -- the scale search's ``w_quantize_func(W * s) / s``.  W is fp16 (bf16 / fp32
    weights are cast at this boundary).  Raises ValueError on non-finite input.  One synchronising read of the 4-byte info block per call."""
    from .hqq_format import HQQWeights
    W = _dense_f16(W, "W")
    N, K = W.shape
    nbits = int(nbits)
    group_size = _awq_check(N, K, nbits, group_size)
    if (hi is None) != (lo is None):
        raise ValueError("hi and lo come together or not at all")
    if col_scale is not None:
        col_scale = col_scale.detach().to(W.device, torch.float32).contiguous()
        _need(col_scale, torch.float32, "col_scale", K)
    if hi is not None:
        hi, lo = hi.detach().contiguous(), lo.detach().contiguous()
        _need(hi, torch.float16, "hi", N * K // group_size)
        _need(lo, torch.float16, "lo", N * K // group_size)
    W_q, scale, zero, out, info, workspace = awq_quantize_buffers(N, K, nbits, group_size, W.device, dense=dense)
    awq_quantize_launch(W, nbits, group_size, col_scale, hi, lo, W_q, scale, zero, out, info, workspace)
    _refuse_nonfinite(info.cpu()[0].item(), "awq_quantize", name, ": a (scaled) weight, a bound or an output was not finite")
    if dense:
        return out
    return HQQWeights(W_q, scale, zero, nbits, (N, K), group_size, bias, name)


class AWQClipInfo:
    """what one ``awq_clip`` call reports: ``nonfinite`` (the info block), ``best`` (int32 [N, K / group]: the chosen shrink step, 0 = none) and
    ``err`` (fp32 [N, K / group, 10]: every step's summed squared output error over the sampled rows), both on the device"""

    def __init__(self, nonfinite, best, err):
        self.nonfinite = int(nonfinite)
        self.best = best
        self.err = err

    def __repr__(self):
        return f"AWQClipInfo(nonfinite={self.nonfinite}, best={tuple(self.best.shape)}, err={tuple(self.err.shape)})"


def awq_clip_launch(W, X, nbits, group_size, hi, lo, best, err, info, workspace):
    """the bare entry point over caller-owned buffers (two launches on the current stream; no allocation, no read-back: capturable)"""
    N, K = W.shape
    _lib.check(_lib.load().amq_awq_clip_f16(_lib.ptr(W), _lib.ptr(X), N, K, int(X.shape[0]), int(nbits), int(group_size), _lib.ptr(hi), _lib.ptr(lo),
                                            _lib.ptr(best), _lib.ptr(err), _lib.ptr(info), _lib.ptr(workspace), _nbytes(workspace),
                                            _lib.current_stream()))


def awq_clip_buffers(N, K, T, nbits, group_size, device):
    """(hi, lo, best, err, info, workspace) of the right sizes for ``awq_clip_launch``"""
    group_size = _awq_check(N, K, nbits, group_size)
    kg = K // group_size
    hi = torch.empty(N, kg, dtype=torch.float16, device=device)
    lo = torch.empty(N, kg, dtype=torch.float16, device=device)
    best = torch.empty(N, kg, dtype=torch.int32, device=device)
    err = torch.empty(N, kg, _lib.AWQ_STEPS, dtype=torch.float32, device=device)
    words = _workspace_words("amq_awq_clip_workspace_bytes", "the AWQ clip search", N=N, K=K, T=int(T), group=group_size)
    return hi, lo, best, err, _info_block(_lib.AWQ_INFO_BYTES, device), _awq_scratch.get(device, words)


def awq_clip(W, X, nbits, group_size=GROUP, return_info=False):
    """AWQ's clip search (auto_clip.py auto_clip_layer_asym: 10 shrink steps of 5 %, asymmetric) for dense W [N, K] (the layer's current, already
    column-scaled weights) against the sampled activation rows X [T, K], on the matrix cores in the arithmetic include/amq_hip.h states: (hi, lo),
    fp16 [N, K / group], the bounds ``awq_quantize`` takes.  W and X are fp16 (bf16 / fp32 are cast at this boundary).  Raises ValueError on
    non-finite input.  One synchronising read of the 4-byte info block per call.  ``return_info``: also return the :class:`AWQClipInfo`."""
    W = _dense_f16(W, "W")
    X = _dense_f16(X, "X")
    N, K = W.shape
    if X.device != W.device or X.shape[1] != K or X.shape[0] < 1:
        raise ValueError(f"X: expected at least one row of {K} values on W's GPU")
    nbits = int(nbits)
    hi, lo, best, err, info, workspace = awq_clip_buffers(N, K, X.shape[0], nbits, group_size, W.device)
    awq_clip_launch(W, X, nbits, group_size, hi, lo, best, err, info, workspace)
    got = AWQClipInfo(info.cpu()[0].item(), best, err)
    _refuse_nonfinite(got.nonfinite, "awq_clip", None, ": a weight or an error sum was not finite")
    return (hi, lo, got) if return_info else (hi, lo)


def fma_mode_for(mn, bits):
    """AMQ_MODE_FMA1 for a native meta buffer whose scales allow the GEMV kernel's one-op unpack (|scale| <= amq_fma1_scale_bound(bits); the same
    weights bit for bit, ~5 % faster decode launches), else AMQ_MODE_FMA.  One device -> host read: call at load time, not per forward."""
    bound = float(_lib.load().amq_fma1_scale_bound(int(bits)))
    smax = float(mn.view(-1, 2)[:, 0].abs().max().item()) if mn.numel() else 0.0
    return MODE_FMA1 if smax <= bound else MODE_FMA


_SD_E = {4: -3, 3: -5, 2: -5}      # csrc/amq_common.cuh SdCfg<BITS>::E


def scale_limit(bits):
    """largest |scale| the matmul kernels' scaled-subnormal unpack takes: it multiplies by the fp16 constant s * 2^-E (amq_common.cuh sd_meta;
    E = -3 at 4 bit, -5 at 3 / 2 bit), which must be finite -- 8188 / 2047 / 2047"""
    if bits not in _SD_E:
        raise ValueError(f"bits must be 2, 3 or 4 (got {bits})")
    return 65504.0 * 2.0 ** _SD_E[bits]


def check_scale_range(mn, bits, mode, name=None):
    """Refuse a native meta buffer with a scale beyond :func:`scale_limit` (ValueError naming the layer, the scale and the limit): past it the
    matmul kernels' weights are inf / NaN while ``dequantize`` -- the other unpack -- still returns finite ones.  The limit is the same for
    MODE_HQQ and the MODE_FMA forms (both multiply by s * 2^-E).  Pure torch (CPU or GPU tensors); one device -> host read: called where a module
    takes its buffers (constructors, to_kernel_arithmetic, load_state_dict), never per forward.  bfloat16 meta is exempt: the bf16 kernels
    do not use this unpack (their scale stays an fp32 factor)."""
    limit = scale_limit(int(bits))
    if mode not in (MODE_HQQ, MODE_FMA, MODE_FMA1):
        raise ValueError(f"unknown dequant mode {mode}")
    if mn.dtype == torch.bfloat16 or mn.numel() == 0 or mn.is_meta:
        return
    s = mn.detach().view(-1, 2)[:, 0].float().abs()
    worst = float(s.max().item())                  # (max propagates NaN)
    who = f"layer {name}" if name else "layer"
    if worst != worst:
        raise ValueError(f"{who}: a scale is NaN")
    if worst > limit:
        raise ValueError(f"{who}: |scale| = {worst} exceeds {limit}, the largest the {int(bits)}-bit matmul kernels' unpack takes "
                         f"(scale * 2^{-_SD_E[int(bits)]} must be a finite fp16 number)")


def _check_native(qn, mn, bits, N, K, fine=False):
    """validates a native (payload, meta) pair and returns its group granularity: 128, or -- where the caller serves them (``fine``) --
    64 / 32, recognised by the meta tensor's size (128 / group pairs per tile row)"""
    qb, mb = native_sizes(bits, N, K)
    _need(qn, torch.int32, "qweight_native", qb // 4)
    if isinstance(mn, torch.Tensor) and mn.numel() != mb // 2 and mn.numel() in (mb, 2 * mb):
        group = GROUP * (mb // 2) // mn.numel()
        if not fine:
            raise ValueError(f"meta_native holds groups of {group}: this entry point serves groups of 128 (and multiples); "
                             f"groups of 64 / 32 run through gemv / gemv_grouped (<= 16 rows), gemm and dequantize")
        _need(mn, torch.float16, "meta_native", mn.numel())
        return group
    _need(mn, torch.float16, "meta_native", mb // 2)
    return GROUP


def dequantize(qn, mn, bits, mode, N, K, out=None):
    _check_shape(bits, N, K)
    group = _check_native(qn, mn, bits, N, K, fine=True)
    if out is None:
        out = torch.empty(N, K, dtype=torch.float16, device=qn.device)
    _need(out, torch.float16, "out", N * K)
    _lib.check(_lib.load().amq_dequantize_f16(bits, mode, _lib.ptr(qn), _lib.ptr(mn), N, K, group,
                                              _lib.ptr(out), _lib.current_stream()))
    return out


def dequantize_hqq(W_q, scale, zero, bits, N, K, group=GROUP):
    _check_shape(bits, N, K)
    group = _check_group(group, K)
    R = N * K // group
    if bits == 3:
        _need(W_q, torch.int32, "W_q", ((R + 9) // 10) * group)
    else:
        _need(W_q, torch.uint8, "W_q", R * group * bits // 8)
    if isinstance(scale, torch.Tensor) and scale.dtype == torch.bfloat16:      # a compute_dtype = bfloat16 layer: dequantized in bf16, as the reference does
        _need(scale, torch.bfloat16, "scale", R)
        _need(zero, torch.bfloat16, "zero", R)
        out = torch.empty(N, K, dtype=torch.bfloat16, device=W_q.device)
        _lib.check(_lib.load().amq_dequantize_hqq_bf16(bits, _lib.ptr(W_q), _lib.ptr(scale), _lib.ptr(zero), N, K, group,
                                                       _lib.ptr(out), _lib.current_stream()))
        return out
    _need(scale, torch.float16, "scale", R)
    _need(zero, torch.float16, "zero", R)
    out = torch.empty(N, K, dtype=torch.float16, device=W_q.device)
    _lib.check(_lib.load().amq_dequantize_hqq_f16(bits, _lib.ptr(W_q), _lib.ptr(scale), _lib.ptr(zero), N, K, group,
                                                  _lib.ptr(out), _lib.current_stream()))
    return out


def _prep_x(x, K):
    if x.dtype != torch.float16:
        raise ValueError(f"x: expected float16, got {x.dtype}")
    if x.shape[-1] != K:
        raise ValueError(f"x: last dim {x.shape[-1]} != K={K}")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    return x2


def _linear_operands(x, qn, mn, bits, N, K, bias, residual, out, fine, M=None):
    """what the single-layer matmuls check before they call the library -> (x as [M, K] rows, M, the layer's group size, y [M, N]: ``out`` or new).
    ``fine``: the call serves groups of 64 / 32 too; ``M`` given: x is already in fragment order (:func:`xfrag`)"""
    _check_shape(bits, N, K)
    group = _check_native(qn, mn, bits, N, K, fine=fine)
    if M is None:
        x = _prep_x(x, K)
        M = x.shape[0]
    else:
        _need(x, torch.float16, "xf", _lib.load().amq_xfrag_bytes(M, K) // 2)
    if bias is not None:
        _need(bias, torch.float16, "bias", N)
    if residual is not None:
        _need(residual, torch.float16, "residual", M * N)
    y = out if out is not None else torch.empty(M, N, dtype=torch.float16, device=x.device)
    _need(y, torch.float16, "y", M * N)
    return x, M, group, y


def _segment_array(segments, M, K, fine):
    """the amq_segment array of a grouped call over M rows and the group size its segments share (``fine``: the call serves groups of 64 / 32 too)"""
    if not 1 <= len(segments) <= _lib.MAX_SEGMENTS:
        raise ValueError(f"1..{_lib.MAX_SEGMENTS} segments")
    arr = (Segment * len(segments))()
    group = None
    for i, s in enumerate(segments):
        _check_shape(s["bits"], s["N"], K)
        g = _check_native(s["qn"], s["mn"], s["bits"], s["N"], K, fine=fine)
        if group is not None and g != group:
            raise ValueError(f"segments of one launch must share their group size (got {group} and {g})")
        group = g
        _need(s["y"], torch.float16, "y", M * s["N"])
        if s.get("bias") is not None:
            _need(s["bias"], torch.float16, "bias", s["N"])
        if s.get("residual") is not None:
            _need(s["residual"], torch.float16, "residual", M * s["N"])
        arr[i] = Segment(_lib.ptr(s["qn"]), _lib.ptr(s["mn"]), _lib.ptr(s.get("bias")), _lib.ptr(s.get("residual")),
                         _lib.ptr(s["y"]), s["N"], s["bits"], s["mode"], 0)
    return arr, group


def gemv(x, qn, mn, bits, mode, N, K, bias=None, out=None, opts=None):
    """y = x . W^T for few rows (weight-streaming kernels).  ``opts``: a :class:`GemvOpts` (per-call A/B / math options)."""
    if opts is None:
        opts = DEFAULT_GEMV_OPTS
    if opts is not None:
        x2 = _prep_x(x, K)
        y = out if out is not None else torch.empty(x2.shape[0], N, dtype=torch.float16, device=x.device)
        gemv_grouped(x2, [dict(qn=qn, mn=mn, bits=bits, mode=mode, N=N, y=y, bias=bias)], K, opts=opts)
        return y.reshape(*x.shape[:-1], N)
    x2, M, group, y = _linear_operands(x, qn, mn, bits, N, K, bias, None, out, True)
    _lib.check(_lib.load().amq_gemv_f16(bits, mode, _lib.ptr(x2), _lib.ptr(qn), _lib.ptr(mn), _lib.ptr(bias),
                                        _lib.ptr(y), M, N, K, group, 0, 0, _lib.current_stream()))
    return y.reshape(*x.shape[:-1], N)


class _ScratchPool:
    """Grow-only device scratch, one buffer per (device, stream).  A buffer that has been handed out is NEVER freed:
    a captured hipGraph (QuantLlama.prefill keeps one per prompt length) has the raw pointer baked in, so when a larger
    request arrives the old block is retired into ``_keep`` instead of being dropped -- replaying an older graph then
    still writes memory this pool owns.  Keyed by stream so that launches on different streams never share partials."""

    def __init__(self, dtype):
        self.dtype = dtype
        self._cur = {}
        self._keep = []

    def get(self, device, numel):
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream)
        t = self._cur.get(key)
        if t is None or t.numel() < numel:
            if t is not None:
                self._keep.append(t)
            t = self._cur[key] = torch.empty(numel, dtype=self.dtype, device=device)
        return t


_SPLITK_WS = _ScratchPool(torch.float32)
_quantize_scratch = _ScratchPool(torch.int32)      # hqq_quantize's workspace (s, the zero trace, the partial errors)
_gptq_scratch = _ScratchPool(torch.int32)          # gptq_quantize's workspace (the columns' errors, the flags, the byte codes)
_awq_scratch = _ScratchPool(torch.int32)           # awq_quantize's / awq_clip's workspace (the flags, the byte codes)
_owq_scratch = _ScratchPool(torch.int32)           # owq_quantize's workspace (the quantized columns' errors, the flags, the byte codes)


def _splitk_workspace(device, nbytes):
    """scratch for split-K partials (see _ScratchPool)"""
    return _SPLITK_WS.get(device, (nbytes + 3) // 4)


# OPT-IN comparison leg for many rows: from LIB_GEMM_ROWS rows on (0 = never, the default) `gemm` runs the bit-exact dequantize
# kernel into a scratch and hands the plain fp16 GEMM to the library (torch.matmul -> hipBLASLt) -- what the reference itself
# does from 128 rows on (GPTQLinear.forward: torch unpack + matmul, hqq/backends/autogptq.py:245-283).  The product path is
# hand-written at every size: the fused kernels below ~6k rows, and from there the same split as the reference's with BOTH halves
# hand-written (GEMM_DEQ: dequantize kernel + amq_gemm_f16.hip; profiles/r04_gemm_f16pp.txt: 1.33-1.45 PFLOP/s at BASELINE configs[3]
# sizes against 1.27-1.32 for the fused ring kernel and 1.42-1.52 for dequantize + hipBLASLt, faster than the library up to 8192 rows);
# bench.py reports the library route next to it.
LIB_GEMM_ROWS = 0
_DEQ_SCRATCH = _ScratchPool(torch.float16)


def _dequant_scratch(device, numel):
    """fp16 scratch for one dequantized weight matrix (see _ScratchPool)"""
    return _DEQ_SCRATCH.get(device, numel)[:numel]


def _route_workspace(lib, device, route, M, N, K, group=GROUP):
    """(tensor or None, bytes) for ``amq_gemm_route_f16`` / ``amq_gemm_gated_f16``: split-K partials for few rows, the dequantized
    fp16 weights for the dequantize-once route (GEMM_DEQ, GEMM_AUTO on MFMA-bound launches, and launches of more than 256 rows over groups of 64 / 32)."""
    need = lib.amq_gemm_route_workspace_bytes_g(route, M, N, K, group)
    if not need:
        return None, 0
    if need == N * K * 2 and (route == GEMM_DEQ or route == GEMM_AUTO):
        return _dequant_scratch(device, N * K), need
    ws = _splitk_workspace(device, need)
    return ws, ws.numel() * 4


def gemm_route_name(M, N=13824, K=5120):
    """what :func:`gemm` runs for an M-row launch under the current settings (for result files)"""
    if LIB_GEMM_ROWS and M >= LIB_GEMM_ROWS:
        return "amq::dequant_kernel + library GEMM (torch.matmul -> hipBLASLt)"
    if _lib.load().amq_gemm_route_workspace_bytes(GEMM_AUTO, M, N, K) == N * K * 2:
        return ("amq::dequant_native_kernel + amq::gemm_f16_pp_kernel (dequantize once into a scratch, then a hand-written fp16 MFMA GEMM: "
                "256x256 tiles, two wave groups in ping-pong, persistent tiles, no unpack in the K loop)")
    return ("amq::gemm_ring_kernel / amq::gemm_ws_kernel / amq::gemm_kernel (fused unpack + MFMA, hand-written; 256x256 ring tiles when they "
            "fill the chip, 256x128 wave-specialised tiles where those fill it better)")


def gemm(x, qn, mn, bits, mode, N, K, bias=None, out=None, residual=None, route=GEMM_AUTO, gate=None):
    """y = x . W^T for any number of rows: few-row kernel, tiled MFMA kernel (split-K when few rows would leave the chip
    idle), or -- from LIB_GEMM_ROWS rows -- dequantize kernel + library GEMM.
    ``residual`` (fp16 [M, N], may be ``out``) is added in the epilogue: y = residual + fp16(x . W^T (+ bias))
    (the library path rounds the sum once).  ``gate`` (fp16 [M, N] contiguous, may be ``out``; not with ``residual``):
    y = fp16(silu(gate)) * fp16(x . W^T (+ bias)), i.e. :func:`silu_mul` of the two projections with this one as ``up``.
    ``route`` != GEMM_AUTO forces one hand-written kernel family (tests, tools)."""
    x2, M, group, y = _linear_operands(x, qn, mn, bits, N, K, bias, residual, out, True)
    lib = _lib.load()
    if gate is not None:
        if residual is not None:
            raise ValueError("gate and residual are exclusive")
        _need(gate, torch.float16, "gate", M * N)
        ws, ws_bytes = _route_workspace(lib, x.device, route, M, N, K, group)
        if y.data_ptr() == gate.data_ptr() and not lib.amq_gemm_gated_fused_g(route, M, N, K, 1 if ws_bytes else 0, group):
            # the tiled kernel cannot apply the gate itself: in place on the gate needs the projection somewhere else first
            up = gemm(x, qn, mn, bits, mode, N, K, bias=bias, route=route)
            silu_mul(gate, up.view(-1), out=y)
            return y.reshape(*x.shape[:-1], N)
        _lib.check(lib.amq_gemm_gated_f16(route, bits, mode, _lib.ptr(x2), _lib.ptr(qn), _lib.ptr(mn), _lib.ptr(bias),
                                          _lib.ptr(gate), _lib.ptr(y), M, N, K, group, 0, _lib.ptr(ws),
                                          ws_bytes, _lib.current_stream()))
        return y.reshape(*x.shape[:-1], N)
    if route == GEMM_AUTO and LIB_GEMM_ROWS and M >= LIB_GEMM_ROWS:
        w = dequantize(qn, mn, bits, mode, N, K, out=_dequant_scratch(x.device, N * K).view(N, K))
        y2 = y.view(M, N)
        if residual is not None:
            r2 = residual.view(M, N)
            if r2.data_ptr() == y2.data_ptr():
                y2.addmm_(x2, w.t())
            else:
                torch.addmm(r2, x2, w.t(), out=y2)
            if bias is not None:
                y2.add_(bias)
        elif bias is not None:
            torch.addmm(bias, x2, w.t(), out=y2)
        else:
            torch.matmul(x2, w.t(), out=y2)
        return y.reshape(*x.shape[:-1], N)
    ws, ws_bytes = _route_workspace(lib, x.device, route, M, N, K, group)
    _lib.check(lib.amq_gemm_route_f16(route, bits, mode, _lib.ptr(x2), _lib.ptr(qn), _lib.ptr(mn), _lib.ptr(bias),
                                      _lib.ptr(residual), _lib.ptr(y), M, N, K, group, 0, 0, _lib.ptr(ws),
                                      ws_bytes, _lib.current_stream()))
    return y.reshape(*x.shape[:-1], N)


def gemm_res_norm_xfrag(x, qn, mn, bits, mode, N, K, gamma, eps, bias=None, residual=None, out=None, xf_out=None):
    """:func:`gemm` (``residual`` fused, dense result rows) followed by :func:`rmsnorm_xfrag` of the result, as one call: returns (y, xf).  Where the
    GEMM runs split-K -- a short prompt's down_proj -- the sum over the splits and the norm are one launch (include/amq_hip.h:
    amq_gemm_res_norm_xfrag_f16); same bits as the two calls."""
    x2, M, group, y = _linear_operands(x, qn, mn, bits, N, K, bias, residual, out, True)
    _need(gamma, torch.float16, "gamma", N)
    lib = _lib.load()
    nbytes = lib.amq_xfrag_bytes(M, N)
    if nbytes == 0:
        raise ValueError(f"N = {N}: the normed rows are handed on in fragment order (N % 128 == 0)")
    xf = xf_out if xf_out is not None else torch.empty(nbytes // 2, dtype=torch.float16, device=x.device)
    _need(xf, torch.float16, "xf", nbytes // 2)
    ws, ws_bytes = _route_workspace(lib, x.device, GEMM_AUTO, M, N, K, group)
    _lib.check(lib.amq_gemm_res_norm_xfrag_f16(bits, mode, _lib.ptr(x2), _lib.ptr(qn), _lib.ptr(mn), _lib.ptr(bias), _lib.ptr(residual),
                                               _lib.ptr(y), M, N, K, group, 0, _lib.ptr(ws), ws_bytes, _lib.ptr(gamma), float(eps),
                                               _lib.ptr(xf), _lib.current_stream()))
    return y.reshape(*x.shape[:-1], N), xf


def gemm_f16w(x, w, bias=None, out=None, residual=None, gate=None):
    """y = x . w^T for DENSE fp16 weights w [N, K] (hand-written ping-pong MFMA kernel, amq_gemm_f16.hip): what GEMM_DEQ runs behind
    :func:`dequantize`; ``residual`` / ``gate`` as in :func:`gemm`.  ``out`` may be a column slice [M, N] of a wider row-major matrix (rows
    ``out.stride(0)`` elements apart, a multiple of 4; no residual / gate then): the C entry point's y_stride."""
    _need(w, torch.float16, "w")
    N, K = w.shape
    x2 = _prep_x(x, K)
    M = x2.shape[0]
    y = out if out is not None else torch.empty(M, N, dtype=torch.float16, device=x.device)
    if y.dim() == 2 and not y.is_contiguous():
        if not y.is_cuda or y.dtype != torch.float16 or tuple(y.shape) != (M, N) or y.stride(1) != 1 or y.stride(0) < N or y.stride(0) % 4 \
                or y.data_ptr() % 8 or residual is not None or gate is not None:
            raise ValueError("y: a strided out must be an fp16 [M, N] column slice of a row-major matrix, rows a multiple of 4 elements apart, "
                             "8-byte aligned, without residual / gate")
        if bias is not None:
            _need(bias, torch.float16, "bias", N)
        _lib.check(_lib.load().amq_gemm_f16w_f16(_lib.ptr(x2), _lib.ptr(w), _lib.ptr(bias), None, None, _lib.ptr(y), M, N, K, 0, y.stride(0),
                                                 _lib.current_stream()))
        return y
    _need(y, torch.float16, "y", M * N)
    for t, nm, n in ((bias, "bias", N), (residual, "residual", M * N), (gate, "gate", M * N)):
        if t is not None:
            _need(t, torch.float16, nm, n)
    _lib.check(_lib.load().amq_gemm_f16w_f16(_lib.ptr(x2), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(residual), _lib.ptr(gate),
                                             _lib.ptr(y), M, N, K, 0, 0, _lib.current_stream()))
    return y.reshape(*x.shape[:-1], N)


def xfrag(src, M, K, stride_m=None, stride_kt=128, out=None):
    """Fragment-ordered copy of M x K activations (see include/amq_hip.h: amq_xfrag_f16).  ``src`` is any fp16 tensor whose
    element (m, k) sits at m*stride_m + (k // 128)*stride_kt + k % 128 (default: row-major [M, K])."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.float16:
        raise ValueError("src: expected an fp16 tensor on the GPU")
    lib = _lib.load()
    nbytes = lib.amq_xfrag_bytes(M, K)
    xf = out if out is not None else torch.empty(nbytes // 2, dtype=torch.float16, device=src.device)
    _need(xf, torch.float16, "xf", nbytes // 2)
    _lib.check(lib.amq_xfrag_f16(_lib.ptr(src), _lib.ptr(xf), M, K, K if stride_m is None else int(stride_m), int(stride_kt),
                                 _lib.current_stream()))
    return xf


def rmsnorm_xfrag(x, gamma, eps, out=None):
    """:func:`rmsnorm` of x [M, K] with the result in fragment order (input of :func:`gemm_xfrag`)."""
    M, K = x.shape
    _need(x, torch.float16, "x")
    _need(gamma, torch.float16, "gamma", K)
    lib = _lib.load()
    nbytes = lib.amq_xfrag_bytes(M, K)
    xf = out if out is not None else torch.empty(nbytes // 2, dtype=torch.float16, device=x.device)
    _need(xf, torch.float16, "xf", nbytes // 2)
    _lib.check(lib.amq_rmsnorm_xfrag_f16(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(xf), M, K, float(eps), _lib.current_stream()))
    return xf


def gemm_xfrag(xf, M, qn, mn, bits, mode, N, K, bias=None, out=None, residual=None, gate=None):
    """y[M, N] = x . W^T with x given in fragment order (:func:`xfrag`); ``residual`` as in :func:`gemm`;
    ``gate`` (fp16 [M, N], may be ``out``): y = fp16(silu(gate)) * fp16(x . W^T (+ bias)), i.e. :func:`silu_mul` fused."""
    xf, M, _, y = _linear_operands(xf, qn, mn, bits, N, K, bias, residual, out, False, M=M)
    if gate is not None:
        _need(gate, torch.float16, "gate", M * N)
    _lib.check(_lib.load().amq_gemm_xfrag_f16(bits, mode, _lib.ptr(xf), _lib.ptr(qn), _lib.ptr(mn), _lib.ptr(bias),
                                              _lib.ptr(gate), _lib.ptr(residual), _lib.ptr(y), M, N, K, GROUP, 0,
                                              _lib.current_stream()))
    return y


def gemm_xfrag_grouped(xf, M, segments, K, form=0, blocks_per_wg=0):
    """One few-row launch for several linears over the same fragment-ordered x (q/k/v, gate/up of a prompt pass).
    segments: list of dicts {qn, mn, bits, mode, N, y, bias=None, residual=None} (y / residual: fp16 [M, N] contiguous).
    Per segment the result is :func:`gemm_xfrag`'s, bit for bit -- whatever the kernel form (``form``: _lib.FEWROW_AUTO / _TILE / _STREAM,
    ``blocks_per_wg`` with _STREAM: tests and A/B tools)."""
    arr, group = _segment_array(segments, M, K, False)
    lib = _lib.load()
    _need(xf, torch.float16, "xf", lib.amq_xfrag_bytes(M, K) // 2)
    _lib.check(lib.amq_gemm_xfrag_grouped_form_f16(arr, len(segments), _lib.ptr(xf), M, K, group, int(form), int(blocks_per_wg), _lib.current_stream()))


def linear(x, qn, mn, bits, mode, N, K, bias=None):
    """Reference-style dispatch: few rows -> gemv family, otherwise gemm."""
    x2, M, group, y = _linear_operands(x, qn, mn, bits, N, K, bias, None, None, True)
    if group != GROUP and M > 0:    # groups of 64 / 32: the GEMV kernel as far as it reaches (16 rows), then gemm (few-row kernel up to 256 rows, dequantize once + the fp16 GEMM beyond)
        if M <= gemv_max_rows(K):
            return gemv(x, qn, mn, bits, mode, N, K, bias=bias, out=y)
        return gemm(x, qn, mn, bits, mode, N, K, bias=bias, out=y)
    if M > 8:                       # tiled MFMA GEMM (split-K for few rows); amq_linear_f16 makes the same cut at 8 rows
        return gemm(x, qn, mn, bits, mode, N, K, bias=bias, out=y)
    if M == 0:
        return y.reshape(*x.shape[:-1], N)
    _lib.check(_lib.load().amq_linear_f16(bits, mode, _lib.ptr(x2), _lib.ptr(qn), _lib.ptr(mn), _lib.ptr(bias),
                                          _lib.ptr(y), M, N, K, GROUP, _lib.current_stream()))
    return y.reshape(*x.shape[:-1], N)


# ---- bfloat16 variants (include/amq_hip.h "bfloat16 variants"; csrc/amq_bf16.hip): models quantized with compute_dtype = torch.bfloat16
_DEQ_SCRATCH_BF16 = _ScratchPool(torch.bfloat16)


def _check_native_bf16(qn, mn, bits, N, K):
    qb, mb = native_sizes(bits, N, K)
    _need(qn, torch.int32, "qweight_native", qb // 4)
    if isinstance(mn, torch.Tensor) and mn.dtype == torch.float16:
        raise ValueError("meta_native is float16: this buffer was repacked from an fp16 model -- use the fp16 entry points")
    _need(mn, torch.bfloat16, "meta_native", mb // 2)


def dequantize_bf16(qn, mn, bits, N, K, out=None):
    """native (bf16 meta) -> W[N, K] bfloat16, bit-identical to Quantizer.dequantize under compute_dtype = bfloat16"""
    _check_shape(bits, N, K)
    _check_native_bf16(qn, mn, bits, N, K)
    if out is None:
        out = torch.empty(N, K, dtype=torch.bfloat16, device=qn.device)
    _need(out, torch.bfloat16, "out", N * K)
    _lib.check(_lib.load().amq_dequantize_bf16(bits, _lib.ptr(qn), _lib.ptr(mn), N, K, GROUP, _lib.ptr(out), _lib.current_stream()))
    return out


def linear_bf16(x, qn, mn, bits, N, K, bias=None, residual=None, out=None):
    """y = x . W^T (+ bias) (+ residual) in bfloat16: up to 16 rows the weight-streaming kernel, beyond dequantize once + the bf16 MFMA GEMM"""
    _check_shape(bits, N, K)
    _check_native_bf16(qn, mn, bits, N, K)
    if x.dtype != torch.bfloat16:
        raise ValueError(f"x: expected bfloat16, got {x.dtype}")
    if x.shape[-1] != K:
        raise ValueError(f"x: last dim {x.shape[-1]} != K={K}")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    if bias is not None:
        _need(bias, torch.bfloat16, "bias", N)
    if residual is not None:
        _need(residual, torch.bfloat16, "residual", M * N)
    y = out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    _need(y, torch.bfloat16, "y", M * N)
    if M == 0:
        return y.reshape(*x.shape[:-1], N)
    lib = _lib.load()
    need = int(lib.amq_gemm_bf16_workspace_bytes(M, N, K))
    ws = _DEQ_SCRATCH_BF16.get(x.device, need // 2) if need else None
    _lib.check(lib.amq_gemm_bf16(bits, _lib.ptr(x2), _lib.ptr(qn), _lib.ptr(mn), _lib.ptr(bias), _lib.ptr(residual), _lib.ptr(y),
                                 M, N, K, GROUP, 0, 0, _lib.ptr(ws), need, _lib.current_stream()))
    return y.reshape(*x.shape[:-1], N)


# Default launch options of the grouped GEMV (None = the library's defaults: exact math, auto geometry).  Only tools/
# set this (explicitly, from their own command lines) to run whole-model A/B experiments; no environment variable does.
DEFAULT_GEMV_OPTS = None


def default_gemv_math():
    """the arithmetic an ``opts=None`` GEMV launch runs in this build of the library (MATH_EXACT or MATH_GROUPSCALE)"""
    return int(_lib.load().amq_default_gemv_math())


def gemv_max_rows(K, plain=False, norm=True):
    """largest number of x rows the weight-streaming GEMV stages in LDS for this K (amq_query); ``plain``: with default options over groups of
    128 (launches of 2 .. 8 rows then run kernels with a smaller cross-wave sum buffer: one row more at K = 11008); ``norm=False``: and without
    an RMSNorm prologue (x may then be staged in two K phases: 8 rows at K = 11008, the 7B down_proj)"""
    out = (ctypes.c_int * 6)()
    _lib.load().amq_query(int(K), out, 6)
    return int((out[4] if norm else out[5]) if plain else out[0])


def gemv_grouped(x, segments, K, prologue=PRO_NONE, x2=None, gamma=None, eps=0.0, opts=None, x_activated=False):
    """One launch for several linears sharing x.

    segments: list of dicts {qn, mn, bits, mode, N, y, bias=None, residual=None, act=False}
    (y / residual: fp16 [M, N] contiguous).  ``act``: the segment stores fp16(silu(y)) -- a gate_proj whose down_proj launch then passes
    ``x_activated=True`` with ``prologue=PRO_SILU_MUL``: x already holds fp16(silu(gate)), the prologue only multiplies (AMQ_PRO_MUL; the same bits
    as SiLU*mul over the plain gate).  Groups of 128; ``act`` takes no residual."""
    xx = _prep_x(x, K)
    M = xx.shape[0]
    arr, group = _segment_array(segments, M, K, True)
    if prologue == PRO_RMSNORM:
        _need(gamma, torch.float16, "gamma", K)
    if x_activated and prologue != PRO_SILU_MUL:
        raise ValueError("x_activated goes with prologue=PRO_SILU_MUL")
    if prologue == PRO_SILU_MUL:
        x2 = _prep_x(x2, K)
        if x2.shape[0] != M:
            raise ValueError("x2 rows != x rows")
        if x_activated:
            prologue = _lib.PRO_MUL
    if opts is None:
        opts = DEFAULT_GEMV_OPTS
    act_mask = sum(1 << i for i, s in enumerate(segments) if s.get("act"))
    if act_mask:                                # a per-call copy: the caller's (or the default) options stay as they are
        o = opts
        opts = GemvOpts(act_mask=act_mask) if o is None else GemvOpts(math=o.math, waves=o.waves, depth=o.depth, rpt=o.rpt, dot=o.dot, act_mask=act_mask)
    _lib.check(_lib.load().amq_gemv_grouped_f16(arr, len(segments), _lib.ptr(xx), _lib.ptr(x2), _lib.ptr(gamma),
                                                ctypes.c_float(eps), prologue, M, K, group, 0,
                                                ctypes.byref(opts) if opts is not None else None, _lib.current_stream()))


def gemv_route(prologue, M, K, bits, modes=None, group=GROUP, opts=None):
    """which kernel :func:`gemv_grouped` launches for these arguments (host logic, no device): ``_lib.GEMV_ROUTE_KEYED`` -- the segments' bit-widths
    fixed at compile time, the one-row launches of a 7B-class decode step -- or ``_lib.GEMV_ROUTE_GENERIC`` (include/amq_hip.h amq_gemv_route).
    ``bits`` / ``modes``: per segment (modes default to MODE_HQQ); ``prologue`` as the library sees it (``_lib.PRO_MUL`` for an activated x)."""
    n = len(bits)
    modes = [MODE_HQQ] * n if modes is None else list(modes)
    rc = _lib.load().amq_gemv_route(prologue, M, K, group, n, (ctypes.c_int * n)(*bits), (ctypes.c_int * n)(*modes),
                                    ctypes.byref(opts) if opts is not None else None)
    _lib.check(min(rc, 0))
    return rc


def gemv_segment_order(bits, act_mask=0):
    """launch order of the segments of a keyed-geometry launch (ascending bit-width, stable) and ``act_mask`` with its bits moved along:
    ``(order, act_mask)``, ``order[i]`` = index of the segment launched i-th (amq_gemv_segment_order)"""
    n = len(bits)
    order, mask = (ctypes.c_int * n)(), ctypes.c_int(0)
    _lib.check(_lib.load().amq_gemv_segment_order(n, (ctypes.c_int * n)(*bits), act_mask, order, ctypes.byref(mask)))
    return list(order), mask.value


# ---------------------------------------------------------------- decode-step surroundings
def gemv_grouped_sums(x, segments, K, gamma=None, eps=0.0, sums_in=None, sums_out=None):
    """5 .. 8 rows: :func:`gemv_grouped` whose RMSNorm takes the rows' sums of squares as per-16-column partials (``sums_in`` fp32 [M, K / 16], with
    ``gamma``) from the launch that produced x, and / or that leaves such partials of ITS output rows in ``sums_out`` (fp32 [M, N / 16]; one segment):
    include/amq_hip.h amq_gemv_grouped_sums_f16.  No pass over x for the statistic, no separate rmsnorm launch."""
    xx = _prep_x(x, K)
    M = xx.shape[0]
    if any(s.get("act") for s in segments):
        raise ValueError("an activated segment (act) is a gate, not a hidden state: the partial-sum launches take none (gemv_grouped)")
    arr, group = _segment_array(segments, M, K, False)
    if sums_in is not None:
        _need(gamma, torch.float16, "gamma", K)
        _need(sums_in, torch.float32, "sums_in", M * (K // 16))
    if sums_out is not None:
        _need(sums_out, torch.float32, "sums_out", M * (segments[0]["N"] // 16))
    _lib.check(_lib.load().amq_gemv_grouped_sums_f16(arr, len(segments), _lib.ptr(xx), _lib.ptr(gamma) if sums_in is not None else None,
                                                     ctypes.c_float(eps), _lib.ptr(sums_in), _lib.ptr(sums_out), M, K, group, _lib.current_stream()))


def rmsnorm(x, gamma, eps, out=None):
    K = x.shape[-1]
    x2 = _prep_x(x, K)
    _need(gamma, torch.float16, "gamma", K)
    y = out if out is not None else torch.empty_like(x2)
    _need(y, torch.float16, "y", x2.numel())
    _lib.check(_lib.load().amq_rmsnorm_f16(_lib.ptr(x2), _lib.ptr(gamma), _lib.ptr(y), x2.shape[0], K,
                                           ctypes.c_float(eps), _lib.current_stream()))
    return y.reshape(x.shape)


def gemv_f16w(x, W, bias=None, gamma=None, eps=0.0, out=None):
    """y[N] = (RMSNorm'ed if gamma) x[K] . W[N,K]^T, fp16 weights (lm_head).  x [M, K] with 2 <= M <= 8 (batched decode):
    y [M, N], W streamed once for all rows."""
    N, K = W.shape
    _need(W, torch.float16, "W", N * K)
    M = x.shape[0] if x.dim() == 2 else 1
    _need(x, torch.float16, "x", M * K)
    if gamma is not None:
        _need(gamma, torch.float16, "gamma", K)
    if bias is not None:
        _need(bias, torch.float16, "bias", N)
    shape = (M, N) if x.dim() == 2 else (N,)
    y = out if out is not None else torch.empty(shape, dtype=torch.float16, device=x.device)
    _need(y, torch.float16, "y", M * N)
    if M == 1:
        _lib.check(_lib.load().amq_gemv_f16w(_lib.ptr(x), _lib.ptr(W), _lib.ptr(bias), _lib.ptr(y), _lib.ptr(gamma),
                                             ctypes.c_float(eps), N, K, _lib.current_stream()))
    else:
        if M > 8:
            raise ValueError("at most 8 rows")
        _lib.check(_lib.load().amq_gemv_f16w_rows(_lib.ptr(x), _lib.ptr(W), _lib.ptr(bias), _lib.ptr(y), _lib.ptr(gamma),
                                                  ctypes.c_float(eps), M, N, K, _lib.current_stream()))
    return y


def _lm8_layer(w8):
    """checks of an hqq_format.LM8Weights on the GPU -> (N, K)"""
    N, K = w8.shape
    if w8.group_size != GROUP or K < GROUP or K % GROUP or N < 1:
        raise ValueError(f"an LM8 layer has groups of {GROUP} along K (got N={N}, K={K}, group {w8.group_size})")
    _need(w8.codes, torch.uint8, "codes", N * K)
    _need(w8.meta, torch.float16, "meta", N * (K // GROUP) * 2)
    return N, K


def lm8_gemv(x, w8, gamma=None, eps=0.0, out=None):
    """y = (RMSNorm'ed if gamma) x . W^T over the 8-bit lm_head ``w8`` (hqq_format.LM8Weights): x [K] -> y [N], or x [M, K] with 1 <= M <= 8 ->
    y [M, N], W streamed once for all rows (include/amq_hip.h amq_lm8_gemv_f16)."""
    N, K = _lm8_layer(w8)
    M = x.shape[0] if x.dim() == 2 else 1
    if M > 8:
        raise ValueError("at most 8 rows")
    _need(x, torch.float16, "x", M * K)
    if gamma is not None:
        _need(gamma, torch.float16, "gamma", K)
    shape = (M, N) if x.dim() == 2 else (N,)
    y = out if out is not None else torch.empty(shape, dtype=torch.float16, device=x.device)
    _need(y, torch.float16, "y", M * N)
    _lib.check(_lib.load().amq_lm8_gemv_f16(_lib.ptr(x), _lib.ptr(w8.codes), _lib.ptr(w8.meta), _lib.ptr(y), _lib.ptr(gamma), ctypes.c_float(eps),
                                            M, N, K, GROUP, _lib.current_stream()))
    return y


def lm8_dequantize(w8, row0=0, rows=None, out=None):
    """rows row0 .. row0 + rows - 1 (default: to the last) of the 8-bit lm_head's weights as fp16 [rows, K]: w = fp16(fp16(fp16(c) - zero) * scale)"""
    N, K = _lm8_layer(w8)
    row0 = int(row0)
    rows = N - row0 if rows is None else int(rows)
    if row0 < 0 or rows < 1 or row0 + rows > N:
        raise ValueError(f"rows {row0} .. {row0 + rows - 1} outside the layer's {N} rows")
    y = out if out is not None else torch.empty(rows, K, dtype=torch.float16, device=w8.codes.device)
    _need(y, torch.float16, "out", rows * K)
    if y.data_ptr() % 16:
        raise ValueError("out: must be 16-byte aligned")
    with torch.cuda.device(w8.codes.device):    # (the layer is no tensor argument: _on_tensor_device cannot name its device)
        _lib.check(_lib.load().amq_lm8_dequantize_f16(_lib.ptr(w8.codes), _lib.ptr(w8.meta), _lib.ptr(y), row0, rows, N, K, GROUP,
                                                      _lib.current_stream()))
    return y


def _tail_args(embed, token, pos, x, table, cur):
    """the checks the token tails and set_token share, and the arguments of their C calls from ``token`` to ``rope_rows``:
    -> (per-sequence step state?, B, (token, step states | pos, x, rope_table[, rope_cur], rope_rows))"""
    vocab, hidden = embed.shape
    B = token.numel()
    _need(embed, torch.float16, "embed", vocab * hidden)
    _need(token, torch.int64, "token", B)
    _need(x, torch.float16, "x", B * hidden)
    states, nseq = _seq_state(cur, pos)
    if states is not None:                      # every sequence advances its own position and cos/sin row
        if nseq != B:
            raise ValueError(f"a step state of {nseq} sequences for {B} tokens")
        _need(table, torch.float16, "rope table")
        return True, B, (_lib.ptr(token), states, _lib.ptr(x), _lib.ptr(table), table.numel() // 128)
    _need(pos, torch.int32, "pos", 1)
    if cur is None:
        return False, B, (_lib.ptr(token), _lib.ptr(pos), _lib.ptr(x), None, None, 0)
    _need(cur, torch.float16, "rope_cur", 128)
    _need(table, torch.float16, "rope table")
    return False, B, (_lib.ptr(token), _lib.ptr(pos), _lib.ptr(x), _lib.ptr(table), _lib.ptr(cur), table.numel() // 128)


def decode_tail(logits, embed, token, pos, x, table=None, cur=None, suppress=None):
    """token = argmax(logits), pos += 1, x = embed[token] (and cur = table[pos], the next step's cos/sin row) -- one
    launch (graph-capturable).  Batched decode: logits [B, vocab], token [B], x [B, hidden]; pos / cur advance once.
    suppress: int32 [8] device tensor of token ids never chosen (-1 = unused slot): HF's min_new_tokens treatment of the EOS ids."""
    vocab, hidden = embed.shape
    _need(logits, torch.float16, "logits", token.numel() * vocab)
    seq, B, mid = _tail_args(embed, token, pos, x, table, cur)
    if suppress is not None:
        _need(suppress, torch.int32, "suppress", 8)
    lib, head = _lib.load(), (_lib.ptr(logits), vocab, _lib.ptr(embed), hidden) + mid
    if seq:
        _lib.check(lib.amq_decode_tail_seq_f16(*head, B, _lib.ptr(suppress), _lib.current_stream()))
    elif suppress is not None:
        _lib.check(lib.amq_decode_tail_suppress_f16(*head, B, _lib.ptr(suppress), _lib.current_stream()))
    elif B == 1:
        _lib.check(lib.amq_decode_tail_f16(*head, _lib.current_stream()))
    else:
        _lib.check(lib.amq_decode_tail_batch_f16(*head, B, _lib.current_stream()))


# ---- sampled decoding (include/amq_hip.h: "sampled decoding"; amq_sample.hip)
SAMPLE_ADVANCE, SAMPLE_EOS = 1, 2
_SMP_WORDS, _SMP_DRAW, _SMP_EOS, _SMP_FINISHED, _SMP_UNFINISHED = 32, 6, 8, 16, 24


def new_sampling_state(device):
    """-> int32 [32] device block of sampling parameters (the layout include/amq_hip.h documents), set to temperature 1, no top-k / top-p, seed 0,
    no EOS ids.  The captured sampled step reads it on every replay: :func:`set_sampling_state` changes what the next replay does."""
    state = torch.zeros(_SMP_WORDS, dtype=torch.int32, device=device)
    set_sampling_state(state)
    return state


def set_sampling_state(state, temperature=1.0, top_k=0, top_p=1.0, seed=0, eos_ids=(), pad_id=0, first_kept=False):
    """write the parameters, reset the draw counter and the finished flags (one 128-byte copy; nothing is re-captured).  ``first_kept``: no draw,
    the first kept token in token order is taken -- with top_k = 1 the greedy arg-max (first maximum) with the sampled tail's EOS bookkeeping."""
    temperature, top_k, top_p, seed, pad_id = float(temperature), int(top_k), float(top_p), int(seed), int(pad_id)
    eos_ids = [int(e) for e in eos_ids]
    if not temperature > 0.0 or temperature == float("inf"):
        raise ValueError(f"temperature must be a positive finite number (got {temperature})")
    if not 0 <= top_k < 2 ** 31:
        raise ValueError(f"top_k must be >= 0 (0 = off), got {top_k}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if len(eos_ids) > 8 or any(e < 0 for e in eos_ids):
        raise ValueError("at most 8 EOS ids, each >= 0")
    if not 0 <= pad_id < 2 ** 31:
        raise ValueError(f"pad_id must be a token id, got {pad_id}")
    _need(state, torch.int32, "state", _SMP_WORDS)
    seed &= (1 << 64) - 1
    host = torch.zeros(_SMP_WORDS, dtype=torch.int32)
    host[0:1].view(torch.float32)[0] = temperature
    host[1] = top_k
    host[2:3].view(torch.float32)[0] = top_p
    host[3] = pad_id
    host[4:6].view(torch.int64)[0] = seed - (1 << 64) if seed >= 1 << 63 else seed
    host[26] = 1 if first_kept else 0
    host[_SMP_EOS:_SMP_EOS + 8] = torch.tensor(eos_ids + [-1] * (8 - len(eos_ids)), dtype=torch.int32)
    state.copy_(host)
    return state


def set_draw_counter(state, draw):
    """the generator's draw counter (advanced by the sampled tail itself; a sequence starts at 0)"""
    state[_SMP_DRAW:_SMP_DRAW + 2].copy_(torch.tensor([int(draw)], dtype=torch.int64).view(torch.int32))


def sample(logits, state, u=None, kept_out=None, suppress=None, out=None, seq0=0, flags=0):
    """tokens int64 [rows] drawn from fp16 logits [rows, vocab] (or [vocab]) with the parameters in ``state``: amq_sample_f16.  ``u``: float32 [rows]
    uniform numbers used instead of the generator (tests); ``kept_out``: uint8 [rows, vocab] receives the kept-set mask; ``flags``: SAMPLE_ADVANCE
    (the draw counter moves on), SAMPLE_EOS (finished flags / pad filling, at most 8 rows)."""
    vocab = logits.shape[-1]
    rows = logits.numel() // vocab
    _need(logits, torch.float16, "logits", rows * vocab)
    _need(state, torch.int32, "state", _SMP_WORDS)
    if u is not None:
        _need(u, torch.float32, "u", rows)
    if kept_out is not None:
        _need(kept_out, torch.uint8, "kept_out", rows * vocab)
    if suppress is not None:
        _need(suppress, torch.int32, "suppress", 8)
    tok = out if out is not None else torch.empty(rows, dtype=torch.int64, device=logits.device)
    _need(tok, torch.int64, "token", rows)
    _lib.check(_lib.load().amq_sample_f16(_lib.ptr(logits), rows, vocab, _lib.ptr(state), _lib.ptr(suppress), _lib.ptr(u), _lib.ptr(tok),
                                          _lib.ptr(kept_out), int(seq0), int(flags), _lib.current_stream()))
    return tok


def _need_rows(t, dtypes, name):
    """a 2-D GPU tensor [M, V] whose rows are dense (any row stride >= V) -> (M, V, row stride in elements)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a tensor on the GPU")
    if t.dtype not in dtypes:
        raise ValueError(f"{name}: expected {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name}: expected [rows, vocab] with at least one row and one column, got {tuple(t.shape)}")
    M, V = t.shape
    if (V > 1 and t.stride(1) != 1) or (M > 1 and t.stride(0) < V):
        raise ValueError(f"{name}: rows must be dense and at least a row apart (strides {tuple(t.stride())})")
    return M, V, (t.stride(0) if M > 1 else V)


def logit_nll(logits, labels=None, out=None):
    """(nll, lse, argmax) per row of fp16 logits [M, V] (any row stride): amq_logit_nll_f16.  ``labels``: int64 [M] on the same device; -100 (HF's
    ignore_index) gives nll = 0, any other label outside the vocabulary NaN; None: every nll is 0.  nll / lse are float32 [M], argmax int32 [M]
    (the first maximum).  ``out``: a (nll, lse, argmax) triple to write into.  No synchronisation."""
    M, V, stride = _need_rows(logits, (torch.float16,), "logits")
    if labels is not None:
        _need(labels, torch.int64, "labels", M)
        if labels.device != logits.device:
            raise ValueError("labels: must be on the device of logits")
    if out is None:
        out = (torch.empty(M, dtype=torch.float32, device=logits.device), torch.empty(M, dtype=torch.float32, device=logits.device),
               torch.empty(M, dtype=torch.int32, device=logits.device))
    nll, lse, amax = out
    for t, dt, nm in ((nll, torch.float32, "nll"), (lse, torch.float32, "lse"), (amax, torch.int32, "argmax")):
        _need(t, dt, nm, M)
        if t.device != logits.device:
            raise ValueError(f"{nm}: must be on the device of logits")
    _lib.check(_lib.load().amq_logit_nll_f16(_lib.ptr(logits), stride, _lib.ptr(labels), M, V, _lib.ptr(nll), _lib.ptr(lse), _lib.ptr(amax),
                                             _lib.current_stream()))
    return nll, lse, amax


def logit_jsd(p, q, eps=1e-7, out=None):
    """Jensen-Shannon divergence per row between fp16 logits ``p`` [M, V] and ``q`` [M, V] (fp16 or fp32), the reference's ``JSD`` (mixture clamped
    at ``eps`` before its log: identical rows score slightly negative) -> float32 [M]: amq_logit_jsd_f16.  Any row strides.  No synchronisation."""
    M, V, ps = _need_rows(p, (torch.float16,), "p")
    Mq, Vq, qs = _need_rows(q, (torch.float16, torch.float32), "q")
    if (Mq, Vq) != (M, V) or q.device != p.device:
        raise ValueError(f"q: expected [{M}, {V}] on {p.device}, got {tuple(q.shape)} on {q.device}")
    y = out if out is not None else torch.empty(M, dtype=torch.float32, device=p.device)
    _need(y, torch.float32, "out", M)
    if y.device != p.device:
        raise ValueError("out: must be on the device of p")
    _lib.check(_lib.load().amq_logit_jsd_f16(_lib.ptr(p), ps, _lib.ptr(q), qs, 1 if q.dtype is torch.float32 else 0, M, V, ctypes.c_float(eps),
                                             _lib.ptr(y), _lib.current_stream()))
    return y


def decode_tail_sample(logits, embed, token, pos, x, state, table=None, cur=None, suppress=None):
    """:func:`decode_tail` with the token drawn by :func:`sample` (draw counter advanced, EOS bookkeeping) instead of the arg-max -- one launch"""
    vocab, hidden = embed.shape
    _need(logits, torch.float16, "logits", token.numel() * vocab)
    _need(state, torch.int32, "state", _SMP_WORDS)
    if suppress is not None:
        _need(suppress, torch.int32, "suppress", 8)
    seq, B, mid = _tail_args(embed, token, pos, x, table, cur)
    fn = _lib.load().amq_decode_tail_sample_seq_f16 if seq else _lib.load().amq_decode_tail_sample_f16
    _lib.check(fn(_lib.ptr(logits), vocab, _lib.ptr(embed), hidden, *mid, B, _lib.ptr(suppress), _lib.ptr(state), _lib.current_stream()))


def set_token(token_in, embed, token, pos, x, table=None, cur=None):
    """token = token_in (int64 CUDA tensor: one id, or one per sequence), x = embed[token], cur = table[pos] -- one launch (amq_set_token_f16); pos unchanged"""
    vocab, hidden = embed.shape
    n_in = token_in.numel()
    _need(token_in, torch.int64, "token_in", n_in)
    seq, B, mid = _tail_args(embed, token, pos, x, table, cur)
    fn = _lib.load().amq_set_token_seq_f16 if seq else _lib.load().amq_set_token_f16
    _lib.check(fn(_lib.ptr(token_in), n_in, _lib.ptr(embed), vocab, hidden, *mid, B, _lib.current_stream()))


QK_NORM_EPS = 1e-6         # Qwen3Config.rms_norm_eps: the default of the wrappers' ``norm_eps``


def _qk_norm(q_norm, k_norm, norm_eps, device):
    """the `amq_qk_norm` argument of the amq_*_qkn_f16 entry points (include/amq_hip.h) for Qwen3's per-head q / k RMSNorm weights, or None when
    neither is given (the entry points without the suffix).  Both or neither; each fp16 [128], contiguous, on ``device``."""
    if q_norm is None and k_norm is None:
        return None
    if q_norm is None or k_norm is None:
        raise ValueError("q_norm and k_norm go together: the kernels normalise both q and k per head (got only "
                         f"{'q_norm' if k_norm is None else 'k_norm'})")
    for name, g in (("q_norm", q_norm), ("k_norm", k_norm)):
        if not isinstance(g, torch.Tensor) or g.dtype is not torch.float16 or tuple(g.shape) != (128,) or not g.is_contiguous():
            raise ValueError(f"{name} must be a contiguous fp16 tensor of 128 elements (one weight per element of a head), got "
                             f"{tuple(g.shape) if isinstance(g, torch.Tensor) else type(g).__name__}"
                             f"{' ' + str(g.dtype) if isinstance(g, torch.Tensor) else ''}")
        if not g.is_cuda:
            raise ValueError(f"{name} must be in GPU memory, which the kernels read (it is on {g.device})")
        if g.device != device:
            raise ValueError(f"{name} must be on {device}, where q is (it is on {g.device})")
    return _lib.QkNorm(q_norm.data_ptr(), k_norm.data_ptr(), float(norm_eps))


def _qkn_fn(lib, name, norm, qkn=None):
    """the entry point ``name`` (norm None) or its `_qkn` variant bound to ``norm``: same arguments behind it.  ``qkn``: the variant's name where
    it is not ``name`` with the suffix"""
    if norm is None:
        return getattr(lib, name)
    fn = getattr(lib, qkn or name[:-len("_f16")] + "_qkn_f16")
    return lambda *args: fn(ctypes.byref(norm), *args)


def rope_cache(q, k, v, kcache, vcache, table, pos0, n_heads, n_kv_heads, q_norm=None, k_norm=None, norm_eps=QK_NORM_EPS):
    """Prefill glue: rotate q [S, n_heads*128] in place, rotate k [S, n_kv_heads*128] into kcache[h, pos0+s], copy v into
    vcache (both [n_kv_heads, max_seq, 128]); ``table`` from :func:`rope_table`.
    Caches [B, n_kv_heads, max_seq, 128] (4-D): q / k / v hold B sequences of S = rows / B rows each, one launch for all.
    ``q_norm`` / ``k_norm`` (both, fp16 [128]): every head of q and k is RMS-normalised with these weights before the rotation (Qwen3), in the
    same launch."""
    norm = _qk_norm(q_norm, k_norm, norm_eps, q.device)
    if kcache.dim() == 4 or norm is not None:
        if kcache.dim() == 3:                   # with norms there is ONE entry point, the batched one: a 3-D cache goes through it as a batch of 1
            if kcache.shape[0] != n_kv_heads:
                raise ValueError("caches must be [n_kv_heads, max_seq, 128]")
            kcache, vcache = kcache.unsqueeze(0), vcache.unsqueeze(0)
        B = kcache.shape[0]
        rows = q.shape[0]
        if rows % B or kcache.shape[1] != n_kv_heads or kcache.shape[3] != 128 or vcache.shape != kcache.shape:
            raise ValueError("caches must be [B, n_kv_heads, max_seq, 128] and q rows a multiple of B")
        S = rows // B
        _need(q, torch.float16, "q", rows * n_heads * 128)
        _need(k, torch.float16, "k", rows * n_kv_heads * 128)
        _need(v, torch.float16, "v", rows * n_kv_heads * 128)
        _need(kcache, torch.float16, "kcache")
        _need(vcache, torch.float16, "vcache")
        _need(table, torch.float16, "rope table")
        _lib.check(_qkn_fn(_lib.load(), "amq_rope_cache_batch_f16", norm, qkn="amq_rope_cache_qkn_f16")(
            _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(kcache), _lib.ptr(vcache), _lib.ptr(table), table.numel() // 128, int(pos0), S, B,
            n_heads, n_kv_heads, 128, kcache.shape[2], _lib.current_stream()))
        return
    S = q.shape[0]
    _need(q, torch.float16, "q", S * n_heads * 128)
    _need(k, torch.float16, "k", S * n_kv_heads * 128)
    _need(v, torch.float16, "v", S * n_kv_heads * 128)
    if kcache.dim() != 3 or kcache.shape[0] != n_kv_heads or kcache.shape[2] != 128 or vcache.shape != kcache.shape:
        raise ValueError("caches must be [n_kv_heads, max_seq, 128]")
    _need(kcache, torch.float16, "kcache")
    _need(vcache, torch.float16, "vcache")
    _need(table, torch.float16, "rope table")
    _lib.check(_lib.load().amq_rope_cache_f16(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(kcache), _lib.ptr(vcache),
                                              _lib.ptr(table), table.numel() // 128, int(pos0), S, n_heads, n_kv_heads, 128,
                                              kcache.shape[1], _lib.current_stream()))


def attn_prefill(q, k, v, out, S, n_heads, n_kv_heads, batch=1, pos0=0, kv_cache=False, out_xfrag=False):
    """Causal attention over a prompt (amq_attn_prefill_f16).  q / out: fp16 [batch*S, n_heads*128] (q rotated).
    kv_cache=False: k / v are projection outputs [batch*S, n_kv_heads*128] (rotated keys); kv_cache=True: k / v are cache
    tensors [batch, n_kv_heads, max_seq, 128] whose rows 0 .. pos0+S-1 are valid.
    out_xfrag (batch 1): ``out`` is an :func:`xfrag` buffer of the result (None: allocated) -- what :func:`gemm_xfrag` reads."""
    H = n_heads * 128
    _need(q, torch.float16, "q", batch * S * H)
    if out_xfrag:
        if batch != 1:
            raise ValueError("out_xfrag needs batch == 1")
        nb = _lib.load().amq_xfrag_bytes(S, H)
        if out is None:
            out = torch.empty(nb // 2, dtype=torch.float16, device=q.device)
        _need(out, torch.float16, "out_xf", nb // 2)
    else:
        _need(out, torch.float16, "out", batch * S * H)
    if kv_cache:
        if k.dim() != 4 or k.shape[0] != batch or k.shape[1] != n_kv_heads or k.shape[3] != 128 or v.shape != k.shape:
            raise ValueError("caches must be [batch, n_kv_heads, max_seq, 128]")
        max_seq = k.shape[2]
        if pos0 + S > max_seq:
            raise ValueError(f"keys 0..{pos0 + S - 1} do not fit the cache (max_seq={max_seq})")
        _need(k, torch.float16, "kcache")
        _need(v, torch.float16, "vcache")
        kr, kb, kh = 128, n_kv_heads * max_seq * 128, max_seq * 128
    else:
        if pos0 != 0:
            raise ValueError("pos0 needs a cache")
        _need(k, torch.float16, "k", batch * S * n_kv_heads * 128)
        _need(v, torch.float16, "v", batch * S * n_kv_heads * 128)
        kr, kb, kh = n_kv_heads * 128, S * n_kv_heads * 128, 128
    if out_xfrag:
        _lib.check(_lib.load().amq_attn_prefill_xfrag_f16(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), S, int(pos0), n_heads,
                                                          n_kv_heads, 128, H, kr, kh, kr, kh, _lib.current_stream()))
        return out
    _lib.check(_lib.load().amq_attn_prefill_f16(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), batch, S, int(pos0), n_heads,
                                                n_kv_heads, 128, H, S * H, kr, kb, kh, kr, kb, kh, H, S * H, _lib.current_stream()))
    return out


def rope_rows(q, k, table, seq_len, n_heads, n_kv_heads, pos0=0, q_norm=None, k_norm=None, norm_eps=QK_NORM_EPS):
    """RoPE in place on q [rows, n_heads*128] and k [rows, n_kv_heads*128], rows = batch * seq_len (no cache).
    ``q_norm`` / ``k_norm``: as :func:`rope_cache`."""
    norm = _qk_norm(q_norm, k_norm, norm_eps, q.device)
    rows = q.shape[0]
    _need(q, torch.float16, "q", rows * n_heads * 128)
    _need(k, torch.float16, "k", rows * n_kv_heads * 128)
    _need(table, torch.float16, "rope table")
    _lib.check(_qkn_fn(_lib.load(), "amq_rope_rows_f16", norm)(_lib.ptr(q), _lib.ptr(k), _lib.ptr(table), table.numel() // 128, int(pos0), rows,
                                                               int(seq_len), n_heads, n_kv_heads, 128, _lib.current_stream()))


def silu_mul(gate, up, out=None):
    """fp16(silu(gate)) * up (LlamaMLP activation), the same expression as the GEMV SiLU prologue."""
    _need(gate, torch.float16, "gate")
    _need(up, torch.float16, "up", gate.numel())
    y = out if out is not None else torch.empty_like(gate)
    _need(y, torch.float16, "out", gate.numel())
    _lib.check(_lib.load().amq_silu_mul_f16(_lib.ptr(gate), _lib.ptr(up), _lib.ptr(y), gate.numel(), _lib.current_stream()))
    return y


STEP_STATE_STRIDE = _lib.STEP_STATE_STRIDE       # bytes between the blocks of a per-sequence step state
_STEP_WORDS = STEP_STATE_STRIDE // 4


def new_step_state(device, batch=None):
    """-> (rope_cur fp16 [128], pos int32 [1], err int32 [1]): three views of one 264-byte block, the layout
    amq_attn_decode_cur_f16 reads.  ``err`` is the sticky error word the attention kernel raises when the device-side
    position is outside the cache (see :func:`check_step_state`).
    ``batch``: the per-sequence form (sequences at positions of their own, include/amq_hip.h: amq_*_seq_f16) -- (rope_cur fp16 [batch, 128],
    pos int32 [batch], err int32 [batch]), strided views of ``batch`` such blocks STEP_STATE_STRIDE bytes apart."""
    if batch is None:
        block = torch.zeros(66, dtype=torch.int32, device=device)
        return block[:64].view(torch.float16), block[64:65], block[65:66]
    blocks = torch.zeros(int(batch), _STEP_WORDS, dtype=torch.int32, device=device)
    return blocks[:, :64].view(torch.float16), blocks[:, 64], blocks[:, 65]


def _seq_state(cur, pos):
    """the base pointer and sequence count of a per-sequence step state, after checking that ``cur`` [B, 128] and ``pos`` [B] are the views
    :func:`new_step_state` made of ONE array of blocks (None, 0 when ``cur`` is not the per-sequence form)"""
    if not isinstance(cur, torch.Tensor) or cur.dim() != 2:
        return None, 0
    B = cur.shape[0]
    ok = (cur.is_cuda and cur.dtype is torch.float16 and cur.shape[1] == 128 and cur.stride(1) == 1 and isinstance(pos, torch.Tensor)
          and pos.dtype is torch.int32 and pos.device == cur.device and tuple(pos.shape) == (B,) and pos.data_ptr() == cur.data_ptr() + 256
          and (B == 1 or (cur.stride(0) == STEP_STATE_STRIDE // 2 and pos.stride(0) == _STEP_WORDS)))
    if not ok:
        raise ValueError("cur [B, 128] / pos [B] must be the views of one per-sequence step state (ops.new_step_state(device, batch=B))")
    return ctypes.c_void_p(cur.data_ptr()), B


def check_step_state(err):
    """raise if a decode step ran with its device-side position outside the KV cache (synchronises); per-sequence state: ANY sequence's"""
    if err.numel() == 1:
        bad = int(err.item()) != 0
    else:
        bad = bool((err != 0).any().item())
    if bad:
        raise _lib.AmqError("a decode step ran with its position outside the KV cache (step skipped on the device)")


def gemv_qkv_attn(x, segments, K, gamma, eps, kcache, vcache, out, cur, n_heads, n_kv_heads, tickets):
    """q / k / v GEMV (RMSNorm prologue) + decode attention of one block as ONE launch (include/amq_hip_ab.h: amq_gemv_qkv_attn_f16; an A/B route in libamq_hip_ab.so).
    segments: three dicts {qn, mn, bits, mode, N, y} (q, k, v; y fp16 [N]); caches [1, n_kv_heads, max_seq, 128]; ``cur``: the
    fp16 [128] view of a step-state block; ``tickets``: int32 [>= n_heads], zero (left zero)."""
    xx = _prep_x(x, K)
    if xx.shape[0] != 1 or len(segments) != 3:
        raise ValueError("one row, three segments (q, k, v)")
    arr = (Segment * 3)()
    for i, s in enumerate(segments):
        _check_shape(s["bits"], s["N"], K)
        _check_native(s["qn"], s["mn"], s["bits"], s["N"], K)
        _need(s["y"], torch.float16, "y", s["N"])
        arr[i] = Segment(_lib.ptr(s["qn"]), _lib.ptr(s["mn"]), None, None, _lib.ptr(s["y"]), s["N"], s["bits"], s["mode"], 0)
    max_seq = kcache.shape[2]
    _need(gamma, torch.float16, "gamma", K)
    _need(kcache, torch.float16, "kcache", n_kv_heads * max_seq * 128)
    _need(vcache, torch.float16, "vcache", n_kv_heads * max_seq * 128)
    _need(out, torch.float16, "out", n_heads * 128)
    _need(cur, torch.float16, "rope_cur", 128)
    if tickets.dtype != torch.int32 or tickets.numel() < n_heads or not tickets.is_cuda:
        raise ValueError("tickets: int32 [n_heads] on the GPU")
    _lib.check_ab(_lib.load_ab().amq_gemv_qkv_attn_f16(arr, _lib.ptr(xx), _lib.ptr(gamma), ctypes.c_float(eps), K, GROUP, _lib.ptr(kcache),
                                                 _lib.ptr(vcache), _lib.ptr(out), _lib.ptr(cur), n_heads, n_kv_heads, 128, max_seq,
                                                 _lib.ptr(tickets), _lib.current_stream()))


ENGINE_LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                  "mlp.down_proj")


class DecodeEngine:
    """One decode token of a whole model as ONE persistent launch (include/amq_hip_ab.h: amq_decode_engine_f16, an A/B route in libamq_hip_ab.so; counterpart of
    the per-token loop of amq/kernel/monkeypatch/ftllama_modeling.py:167-230).

    blocks: list of dicts, one per decoder block: the seven linears under ENGINE_LINEARS as dicts {qn, mn, bits, mode, N}
    (native buffers), "ln1" / "ln2" fp16 [hidden], "kc" / "vc" fp16 [1, n_kv_heads, max_seq, 128] (batch 1).
    x: fp16 [hidden] residual stream (in / out); step_cur: the fp16 [128] view of a step-state block (new_step_state()).
    The device table, scratch and barrier words are owned by this object; step() only enqueues (graph-capturable)."""

    def __init__(self, blocks, hidden, inter, n_heads, n_kv_heads, max_seq, eps, x, step_cur, grid=0):
        lib = _lib.load_ab()
        dev = x.device
        nb = len(blocks)
        _need(x, torch.float16, "x", hidden)
        _need(step_cur, torch.float16, "rope_cur", 128)
        arr = (EngineBlock * nb)()
        keep = []
        for b, blk in enumerate(blocks):
            for i, name in enumerate(ENGINE_LINEARS):
                l = blk[name]
                K = inter if name == "mlp.down_proj" else hidden
                _check_shape(l["bits"], l["N"], K)
                _check_native(l["qn"], l["mn"], l["bits"], l["N"], K)
                if l["qn"].device != dev:
                    raise ValueError("all engine buffers must live on x's device")
                arr[b].lin[i] = EngineLinear(_lib.ptr(l["qn"]), _lib.ptr(l["mn"]), l["N"], l["bits"], l["mode"], 0)
                keep += [l["qn"], l["mn"]]
            _need(blk["ln1"], torch.float16, "ln1", hidden)
            _need(blk["ln2"], torch.float16, "ln2", hidden)
            for c in ("kc", "vc"):
                _need(blk[c], torch.float16, c, n_kv_heads * max_seq * 128)
            arr[b].ln1, arr[b].ln2 = _lib.ptr(blk["ln1"]), _lib.ptr(blk["ln2"])
            arr[b].kcache, arr[b].vcache = _lib.ptr(blk["kc"]), _lib.ptr(blk["vc"])
            keep += [blk["ln1"], blk["ln2"], blk["kc"], blk["vc"]]
        nbytes = int(lib.amq_decode_engine_image_bytes(nb))
        host = (ctypes.c_ubyte * nbytes)()
        _lib.check_ab(lib.amq_decode_engine_image(arr, nb, hidden, inter, n_heads, n_kv_heads, 128, GROUP, host))
        self.image = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev)
        self.scratch = torch.zeros(int(lib.amq_decode_engine_scratch_bytes(hidden, inter, n_kv_heads)), dtype=torch.uint8, device=dev)
        self.sync = torch.zeros(int(lib.amq_decode_engine_sync_bytes()) // 4, dtype=torch.int32, device=dev)
        self._keep = keep
        self.x, self.cur = x, step_cur
        self.args = (nb, hidden, inter, n_heads, n_kv_heads, 128, int(max_seq), ctypes.c_float(eps))
        self.grid = int(grid)
        self._grid_used = None

    def step(self):
        if self._grid_used != self.grid:         # the barrier words count arrivals of ONE grid size across launches
            self.sync.zero_()
            self._grid_used = self.grid
        _lib.check_ab(_lib.load_ab().amq_decode_engine_f16(_lib.ptr(self.image), *self.args, _lib.ptr(self.x), _lib.ptr(self.scratch),
                                                     self.scratch.numel(), _lib.ptr(self.cur), _lib.ptr(self.sync),
                                                     self.sync.numel() * 4, self.grid, _lib.current_stream()))

    def check(self):
        """raise if a barrier poll of an earlier step ran into its bound (synchronises)"""
        word = int(self.sync[(2 + 2 * 32 - 1) * 64].item())
        if word != 0:
            who = int(self.sync[(2 + 2 * 32 - 1) * 64 + 1].item())
            # recover here, not only in step(): a runner replays a captured hipGraph and never comes through step(), and the sticky error
            # word / the un-advanced epoch base would fail every later replay.  The caller drops its graph (QuantLlama.check).
            self.sync.zero_()
            self._grid_used = None
            raise _lib.AmqError("decode engine: a device-wide barrier timed out (barrier %d of the launch, first seen by workgroup %d)"
                                % (word & 0xFFFF, who))

    def vector(self, name):
        """fp16 view of one hand-off vector of the scratch buffer ('q', 'k', 'v', 'att', 'gate', 'up'): tests only"""
        nb, H, I, nh, nkv = self.args[0], self.args[1], self.args[2], self.args[3], self.args[4]
        sizes = [("q", H), ("k", nkv * 128), ("v", nkv * 128), ("att", H), ("gate", I), ("up", I)]
        off = 0
        for n, sz in sizes:
            if n == name:
                return self.scratch[off:off + 2 * sz].view(torch.float16)
            off += (2 * sz + 255) // 256 * 256
        raise KeyError(name)


def rope_table(max_seq, rope_theta, device, inv_freq=None, scale=1.0):
    """fp16 [max_seq, 64, 2] (cos, sin) rows.  ``inv_freq`` (fp32 [64]: HF's ``rotary_emb.inv_freq`` after a static rope_scaling -- Llama-3.1's
    "llama3" factors, arch.rope_inv_freq) and ``scale`` (its attention_scaling) replace the plain ``rope_theta`` frequencies."""
    tab = torch.empty(max_seq, 64, 2, dtype=torch.float16, device=device)
    if inv_freq is None:
        _lib.check(_lib.load().amq_rope_table_f16(_lib.ptr(tab), max_seq, ctypes.c_float(rope_theta), _lib.current_stream()))
    else:
        f = inv_freq.detach().to(device=device, dtype=torch.float32).contiguous()
        if f.numel() != 64:
            raise ValueError("inv_freq must hold 64 frequencies (head_dim 128)")
        _lib.check(_lib.load().amq_rope_table_freqs_f16(_lib.ptr(tab), max_seq, _lib.ptr(f), ctypes.c_float(scale), _lib.current_stream()))
    return tab


class _ZeroedPool:
    """Zeroed int32 ticket arrays (split decode attention), one per (device, stream), grow-only like :class:`_ScratchPool`:
    every launch leaves its tickets zero, so one array serves all launches of a stream."""

    def __init__(self):
        self._cur = {}
        self._keep = []

    def get(self, device, n):
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream)
        t = self._cur.get(key)
        if t is None or t.numel() < n:
            if t is not None:
                self._keep.append(t)
            t = self._cur[key] = torch.zeros(max(n, 1024), dtype=torch.int32, device=device)
        return t


_ATTN_WS = _ScratchPool(torch.float32)
_ATTN_TICKETS = _ZeroedPool()
ATTN_SPLIT_FROM = 512      # caches longer than this use the split kernel (n_splits = 0 / auto)
ATTN_CHUNK = 272           # keys per workgroup aimed at for a full cache (the kernel holds up to 384 in registers; its smallest chunk is 256)
ATTN_CUS = 256             # workgroups per round of the chip (MI355X: 256 CUs)
ATTN_PREFETCH_KEYS = 384   # keys of a chunk the split kernel requests ahead into registers (amq_decode.hip); longer chunks take its remainder loop


ATTN_GQA_KEYS = 0          # keys per workgroup of the grouped-query kernel (0: by cache length, attn_decode_splits; a multiple of 128: A/B tools)


def attn_decode_splits(max_seq, n_heads=32, batch=1, n_kv_heads=None):
    """workgroups per head the auto policy gives a cache of ``max_seq`` rows (1: the single-workgroup kernel): about ATTN_CHUNK keys each, and --
    where the heads divide the CU count -- a whole number of rounds of the chip (7B at 2048 keys: 8 x 32 = 256 workgroups of 264 keys run the launch
    in 11.9 us, 6 x 32 of 352 keys in 11.8; at 4000 keys 16 x 32 in 18.1 against 11 x 32 in 19.6: profiles/r05_attn_decode_long.txt).
    Grouped-query models (``n_kv_heads`` given, 2 .. 16 query heads per kv head): workgroups per KV head of the grouped kernel (amq_attn_prefill.hip:
    attn_decode_gqa_kernel), chunks of 64 / 128 / 256 keys -- the longest that still gives the chip a round of workgroups."""
    if max_seq <= ATTN_SPLIT_FROM:
        return 1
    g = n_heads // n_kv_heads if n_kv_heads else 1
    if 2 <= g <= 16:
        # a round of the chip (workgroups = kv heads x sequences x splits), chunks of whole 128-key stages: 128 keys up to 2048 cached keys, at least 256
        # beyond (more, smaller chunks cost more in partial results than they gain: profiles/r06_attn_gqa.txt); ATTN_GQA_KEYS: A/B tools
        want = max(1, ATTN_CUS // (n_kv_heads * batch))
        if want > 32 and 32 * n_kv_heads * batch >= ATTN_CUS // 2:
            want = 32           # the combine launch takes 32 chunks in one round trip: 28 / 4 heads at 16384 keys 20.2 us with 64 chunks, 17.4 with 32
        per = ATTN_GQA_KEYS or max(128 if max_seq <= 2048 else 256, -(-max_seq // want))
        per = -(-per // 128) * 128
        return max(2, -(-max_seq // per))
    s = max(1, round(max_seq / ATTN_CHUNK))
    wg = max(1, n_heads * batch)
    if ATTN_CUS % wg == 0:
        step = ATTN_CUS // wg              # splits per round of the chip
        s = max(step, round(s / step) * step) if s >= step else s
        # rounding DOWN to a whole round may leave chunks beyond the kernel's 384-key register prefetch (32 heads at ~3000 - 3128 keys: 11 -> 8
        # splits of 416 keys, the slower remainder loop): go up a round instead
        while s >= step and (-(-max_seq // s) + 31) // 32 * 32 > ATTN_PREFETCH_KEYS:
            s += step
    return s


def _split_scratch(lib, device, rows, n_heads, n_splits):
    """-> (workspace pointer, its bytes, tickets pointer) of a decode-attention call over ``n_splits`` > 1 workgroups per head; (None, 0, None) for one"""
    if n_splits <= 1:
        return None, 0, None
    wsb = lib.amq_attn_decode_split_workspace_bytes(rows, n_heads, n_splits)
    return _lib.ptr(_ATTN_WS.get(device, wsb // 4)), wsb, _lib.ptr(_ATTN_TICKETS.get(device, rows * n_heads))


def _attn_call(lib, name, norm, tensors, where, heads, rest=()):
    """one decode-attention call: entry point ``name`` (its `_qkn` twin under ``norm``) over ``tensors`` = (q, k, v, kcache, vcache, out); ``where``: its
    position arguments; ``heads`` = (rows, n_heads, n_kv_heads, max_seq); ``rest``: what follows max_seq in front of the stream.  -> out"""
    rows, n_heads, n_kv_heads, max_seq = heads
    _lib.check(_qkn_fn(lib, name, norm)(*map(_lib.ptr, tensors), *where, rows, n_heads, n_kv_heads, 128, max_seq, *rest, _lib.current_stream()))
    return tensors[5]


def attn_decode(q, k, v, kcache, vcache, out, pos, n_heads, n_kv_heads, rope_theta=10000.0, table=None, cur=None, n_splits=0,
                q_norm=None, k_norm=None, norm_eps=QK_NORM_EPS):
    """One new token per sequence.  q [B, n_heads*128], k/v [B, n_kv_heads*128],
    caches [B, n_kv_heads, max_seq, 128]; ``pos`` is an int or a device int32 tensor.  ``cur``: fp16 [128] cos/sin row
    of the current position (maintained by decode_tail) -- needs ``pos`` as a device tensor.
    ``n_splits``: workgroups per head (include/amq_hip.h: amq_attn_decode_split_f16); 0 = by cache length, 1 = the
    single-workgroup kernel.
    ``cur`` [B, 128] with ``pos`` [B] (ops.new_step_state(device, batch=B)): every sequence at its own position (amq_attn_decode_seq_f16).
    ``q_norm`` / ``k_norm`` (both, fp16 [128]) with ``norm_eps``: Qwen3's per-head RMSNorm of q and of the new k, applied inside the same kernels
    in front of the rotation (the amq_*_qkn_f16 entry points); neither: the kernels as they are for every other model."""
    norm = _qk_norm(q_norm, k_norm, norm_eps, q.device)
    B = kcache.shape[0]
    max_seq = kcache.shape[2]
    if n_splits == 0:
        n_splits = attn_decode_splits(max_seq, n_heads, B, n_kv_heads)
    _need(q, torch.float16, "q", B * n_heads * 128)
    _need(k, torch.float16, "k", B * n_kv_heads * 128)
    _need(v, torch.float16, "v", B * n_kv_heads * 128)
    _need(kcache, torch.float16, "kcache", B * n_kv_heads * max_seq * 128)
    _need(vcache, torch.float16, "vcache", B * n_kv_heads * max_seq * 128)
    _need(out, torch.float16, "out", B * n_heads * 128)
    lib, tensors, heads = _lib.load(), (q, k, v, kcache, vcache, out), (B, n_heads, n_kv_heads, max_seq)
    states, nseq = _seq_state(cur, pos)
    if states is not None:                      # per-sequence step state: sequence b appends at ITS pos[b] and attends rows 0 .. pos[b]
        if nseq != B:
            raise ValueError(f"a step state of {nseq} sequences for caches of {B}")
        return _attn_call(lib, "amq_attn_decode_seq_f16", norm, tensors, (states,), heads,
                          (n_splits if n_splits > 1 else 0,) + _split_scratch(lib, q.device, B, n_heads, n_splits))
    if isinstance(pos, torch.Tensor):
        _need(pos, torch.int32, "pos", 1)
        pos_dev, pos_i = ctypes.cast(pos.data_ptr(), ctypes.c_void_p), 0
    else:
        pos_dev, pos_i = None, int(pos)
        if not 0 <= pos_i < max_seq:
            raise ValueError(f"pos {pos_i} outside the cache (max_seq={max_seq})")
    if cur is not None:
        # step-state block: cos/sin row (256 bytes) immediately followed by the int32 position and the error word (new_step_state())
        _need(cur, torch.float16, "rope_cur", 128)
        if pos_dev is None or pos.data_ptr() != cur.data_ptr() + 256:
            raise ValueError("cur / pos must be the two views of one step-state block (ops.new_step_state)")
    if table is not None:
        _need(table, torch.float16, "rope table", max_seq * 128)
    if n_splits > 1:
        return _attn_call(lib, "amq_attn_decode_split_f16", norm, tensors, (_lib.ptr(cur), pos_dev, pos_i), heads,
                          (ctypes.c_float(rope_theta), _lib.ptr(table), n_splits) + _split_scratch(lib, q.device, B, n_heads, n_splits))
    if cur is not None:
        return _attn_call(lib, "amq_attn_decode_cur_f16", norm, tensors, (_lib.ptr(cur),), heads)
    return _attn_call(lib, "amq_attn_decode_f16", norm, tensors, (pos_dev, pos_i), heads, (ctypes.c_float(rope_theta), _lib.ptr(table)))


# ---- 8-bit KV cache (include/amq_hip.h: "8-bit KV cache"; amq_attn_kv8.hip)
KV8_ROW_BYTES = 132        # 128 int8 codes + one fp32 scale (the fp16 cache: 256)
KV8_CHUNK_MIN = 256        # fewest keys the policy gives a workgroup: one tile of the kernel's online softmax
KV8_HEADS_PER_WG = 8       # query heads of a kv head one workgroup serves (amq_attn_kv8.hip: kv8_head_blocks)
KV8_WGS = 2 * ATTN_CUS     # workgroups a launch aims at: two of its 256-thread workgroups fit a CU's registers and LDS


def kv8_alloc(B, n_kv_heads, max_seq, device):
    """-> (kc8, ks, vc8, vs): int8 [B, n_kv_heads, max_seq, 128] codes and fp32 [B, n_kv_heads, max_seq] scales of K and of V, zeroed (a zero
    scale with zero codes stands for a zero row)"""
    mk = lambda: (torch.zeros(B, n_kv_heads, max_seq, 128, dtype=torch.int8, device=device),
                  torch.zeros(B, n_kv_heads, max_seq, dtype=torch.float32, device=device))
    (kc8, ks), (vc8, vs) = mk(), mk()
    return kc8, ks, vc8, vs


def _need_kv8(kc8, ks, vc8, vs):
    if kc8.dim() != 4 or kc8.shape[3] != 128:
        raise ValueError("kc8 must be int8 [B, n_kv_heads, max_seq, 128]")
    B, nkv, max_seq = kc8.shape[:3]
    for t, name in ((kc8, "kc8"), (vc8, "vc8")):
        _need(t, torch.int8, name, B * nkv * max_seq * 128)
    for t, name in ((ks, "ks"), (vs, "vs")):
        _need(t, torch.float32, name, B * nkv * max_seq)
    return B, nkv, max_seq


def kv8_store(k, v, kc8, ks, vc8, vs, pos0, n_kv_heads):
    """the prompt pass' glue: ROTATED k and v, fp16 [B * S, n_kv_heads * 128], quantized into rows pos0 .. pos0 + S - 1 of every sequence's slice
    of the 8-bit caches (one launch)"""
    B, nkv, max_seq = _need_kv8(kc8, ks, vc8, vs)
    if nkv != n_kv_heads:
        raise ValueError(f"caches of {nkv} kv heads, n_kv_heads={n_kv_heads}")
    rows = k.numel() // (n_kv_heads * 128)
    if rows < B or rows % B:
        raise ValueError(f"{rows} rows of k for caches of {B} sequences")
    S = rows // B
    _need(k, torch.float16, "k", rows * n_kv_heads * 128)
    _need(v, torch.float16, "v", rows * n_kv_heads * 128)
    pos0 = int(pos0)
    if pos0 < 0 or pos0 + S > max_seq:
        raise ValueError(f"rows {pos0} .. {pos0 + S - 1} outside the cache (max_seq={max_seq})")
    _lib.check(_lib.load().amq_kv8_store_f16(*map(_lib.ptr, (k, v, kc8, ks, vc8, vs)), pos0, S, B, n_kv_heads, 128, max_seq, _lib.current_stream()))


def kv8_dequantize(kc8, ks, dtype=torch.float32):
    """the rows an 8-bit cache stands for: fp32(code) * scale (fp32), or that value rounded to fp16 -- plain torch, for tests and tools"""
    x = kc8.to(torch.float32) * ks.unsqueeze(-1)
    return x if dtype is torch.float32 else x.to(dtype)


def attn_decode_kv8_splits(max_seq, n_heads=32, batch=1, n_kv_heads=None):
    """workgroups per (sequence, kv head, head block) the auto policy gives an 8-bit cache of ``max_seq`` rows: enough chunks of at least
    KV8_CHUNK_MIN keys for KV8_WGS workgroups in the launch (chunks beyond the position leave at once)"""
    if max_seq <= KV8_CHUNK_MIN:
        return 1
    nkv = n_kv_heads or n_heads
    hblk = -(-(n_heads // nkv) // KV8_HEADS_PER_WG)
    want = -(-KV8_WGS // max(1, nkv * hblk * batch))
    return max(1, min(want, max_seq // KV8_CHUNK_MIN))


def attn_decode_kv8_chunk(max_seq, n_splits):
    """keys per workgroup of a launch over ``n_splits`` chunks (amq_attn_kv8.hip: kv8_chunk)"""
    return max(32, (-(-max_seq // n_splits) + 31) // 32 * 32)


def attn_decode_kv8(q, k, v, kc8, ks, vc8, vs, out, pos, n_heads, n_kv_heads, table=None, cur=None, n_splits=0, rope_theta=10000.0):
    """One new token per sequence over the 8-bit caches (ops.kv8_alloc): q [B, n_heads*128], k / v [B, n_kv_heads*128] un-rotated; the new row is
    quantized and appended at ``pos`` (shared by the batch) and out [B, n_heads*128] is the attention over the dequantized rows 0 .. pos.  ``pos``:
    an int with ``table`` (or neither: cos/sin computed in the kernel), or with ``cur`` the two views of one step-state block (ops.new_step_state).
    ``n_splits``: workgroups per (sequence, kv head); 0 = :func:`attn_decode_kv8_splits`."""
    B, nkv, max_seq = _need_kv8(kc8, ks, vc8, vs)
    if nkv != n_kv_heads:
        raise ValueError(f"caches of {nkv} kv heads, n_kv_heads={n_kv_heads}")
    if n_splits == 0:
        n_splits = attn_decode_kv8_splits(max_seq, n_heads, B, n_kv_heads)
    _need(q, torch.float16, "q", B * n_heads * 128)
    _need(k, torch.float16, "k", B * n_kv_heads * 128)
    _need(v, torch.float16, "v", B * n_kv_heads * 128)
    _need(out, torch.float16, "out", B * n_heads * 128)
    if isinstance(pos, torch.Tensor):
        _need(pos, torch.int32, "pos", 1)
        pos_dev, pos_i = ctypes.cast(pos.data_ptr(), ctypes.c_void_p), 0
    else:
        pos_dev, pos_i = None, int(pos)
        if not 0 <= pos_i < max_seq:
            raise ValueError(f"pos {pos_i} outside the cache (max_seq={max_seq})")
    if cur is not None:
        _need(cur, torch.float16, "rope_cur", 128)
        if pos_dev is None or pos.data_ptr() != cur.data_ptr() + 256:
            raise ValueError("cur / pos must be the two views of one step-state block (ops.new_step_state)")
    if table is not None:
        _need(table, torch.float16, "rope table", max_seq * 128)
    lib = _lib.load()
    wsb = lib.amq_attn_decode_kv8_workspace_bytes(B, n_heads, n_splits)
    ws, tickets = _ATTN_WS.get(q.device, wsb // 4), _ATTN_TICKETS.get(q.device, B * n_kv_heads * 2)
    _lib.check(lib.amq_attn_decode_kv8_f16(*map(_lib.ptr, (q, k, v, kc8, ks, vc8, vs, out, cur)), pos_dev, pos_i, B, n_heads, n_kv_heads, 128, max_seq,
                                           ctypes.c_float(rope_theta), _lib.ptr(table), n_splits, _lib.ptr(ws), wsb, _lib.ptr(tickets),
                                           _lib.current_stream()))
    return out


# ---- prompt-lookup speculative decoding (include/amq_hip.h: "prompt-lookup speculative decoding"; amq_decode.hip ROWS instantiations, amq_lookup.hip)
LOOKUP_STATE_WORDS = _lib.LOOKUP_STATE_WORDS
LOOKUP_DRAFTS, LOOKUP_NGRAM, LOOKUP_MODE, LOOKUP_COUNT, LOOKUP_STEPS, LOOKUP_ACCEPTED, LOOKUP_TICKET, LOOKUP_DRAFT, LOOKUP_ARGMAX = 0, 1, 2, 3, 4, 5, 6, 8, 16
LOOKUP_MAX_ROWS = 8


def new_lookup_state(device, drafts, ngram_max=2, history_cap=0):
    """-> (state int32 [32], history int32 [history_cap]): the device block amq_decode_tail_lookup_f16 reads and keeps (word layout: include/amq_hip.h)
    and the token history, for ``drafts`` = 1 .. 7 guessed tokens per step and suffixes of up to ``ngram_max`` = 1 .. 4 tokens; no drafts yet (-1)."""
    drafts, ngram_max, history_cap = int(drafts), int(ngram_max), int(history_cap)
    if not 1 <= drafts <= LOOKUP_MAX_ROWS - 1:
        raise ValueError(f"drafts must be 1..{LOOKUP_MAX_ROWS - 1} (got {drafts})")
    if not 1 <= ngram_max <= 4:
        raise ValueError(f"ngram_max must be 1..4 (got {ngram_max})")
    if not 1 <= history_cap <= 1 << 24:
        raise ValueError(f"history_cap must be 1..2^24 (got {history_cap})")
    host = torch.zeros(LOOKUP_STATE_WORDS, dtype=torch.int32)
    host[LOOKUP_DRAFTS], host[LOOKUP_NGRAM] = drafts, ngram_max
    host[LOOKUP_DRAFT:LOOKUP_DRAFT + 8] = -1
    return host.to(device), torch.zeros(history_cap, dtype=torch.int32, device=device)


def attn_rows_gqa_blocks(rows, n_heads, n_kv_heads):
    """MFMA row blocks of the grouped rows launch: 16 query rows (step row, head of the group) each"""
    return -(-rows * (n_heads // n_kv_heads) // 16)


def attn_decode_rows(q, k, v, kcache, vcache, out, cur, pos, n_heads, n_kv_heads, n_splits=0, q_norm=None, k_norm=None, norm_eps=QK_NORM_EPS,
                     grouped=False):
    """``rows`` = 2 .. 8 consecutive positions of ONE sequence (amq_attn_decode_rows_f16): q / out [rows, n_heads*128], k / v [rows, n_kv_heads*128],
    caches [1, n_kv_heads, max_seq, 128] (or 3-D); ``cur`` [rows, 128] / ``pos`` [rows]: the views of one per-sequence step state whose block j holds
    position p + j.  Row j appends cache row p + j and attends rows 0 .. p - 1 of the cache plus this step's rows 0 .. j.
    ``n_splits``: 0 = by cache length, 1 = the single-workgroup kernel, >= 2 the per-head split kernel.
    ``q_norm`` / ``k_norm``: as :func:`attn_decode` (every workgroup normalises the earlier rows' keys it rotates for itself: the same bits).
    ``grouped``: the matrix-core kernel of grouped-query models (amq_attn_decode_rows_gqa_f16; 2 .. 16 query heads per kv head): row j's output has
    the bits of :func:`attn_decode` at position p + j with the same ``n_splits`` >= 2.  ``n_splits``: chunks of the cache (>= 1); 0 = the grouped
    policy of :func:`attn_decode_splits`."""
    norm = _qk_norm(q_norm, k_norm, norm_eps, q.device)
    if grouped and not (n_kv_heads > 0 and n_heads % n_kv_heads == 0 and 2 <= n_heads // n_kv_heads <= 16):
        raise ValueError(f"grouped=True serves 2..16 query heads per kv head (got {n_heads} / {n_kv_heads})")
    states, R = _seq_state(cur, pos)
    if states is None:
        raise ValueError("cur [rows, 128] / pos [rows] must be the views of one per-sequence step state (ops.new_step_state(device, batch=rows))")
    if not 2 <= R <= LOOKUP_MAX_ROWS:
        raise ValueError(f"rows must be 2..{LOOKUP_MAX_ROWS} (got {R})")
    if kcache.dim() == 4 and kcache.shape[0] != 1:
        raise ValueError("the rows of a step belong to ONE sequence: caches [1, n_kv_heads, max_seq, 128]")
    max_seq = kcache.shape[-2]
    if n_splits == 0 and grouped:
        # the single-token grouped policy with the launch's row blocks standing in for sequences (workgroups = kv heads x row blocks x splits).
        # Not tuned for this launch: measured against half and twice its split count only (tools/lookup_gqa_bench.py, profiles/lookup_gqa.json:
        # 32/8, 28/4, 64/8 heads x 2048 / 8192 / 32768 keys x R = 2, 4, 8 -- a neighbour is never more than 2 % faster, and up to 71 % slower).
        n_splits = attn_decode_splits(max_seq, n_heads, attn_rows_gqa_blocks(R, n_heads, n_kv_heads), n_kv_heads)
    elif n_splits == 0:
        n_splits = attn_decode_splits(max_seq, n_heads, R)       # (the per-head policy also for grouped-query models: they take the per-head kernels here)
    _need(q, torch.float16, "q", R * n_heads * 128)
    _need(k, torch.float16, "k", R * n_kv_heads * 128)
    _need(v, torch.float16, "v", R * n_kv_heads * 128)
    _need(kcache, torch.float16, "kcache", n_kv_heads * max_seq * 128)
    _need(vcache, torch.float16, "vcache", n_kv_heads * max_seq * 128)
    _need(out, torch.float16, "out", R * n_heads * 128)
    lib = _lib.load()
    if grouped:                                 # (the workspace is part of every grouped call, one chunk included)
        wsb = lib.amq_attn_decode_split_workspace_bytes(R, n_heads, n_splits)
        scratch = (_lib.ptr(_ATTN_WS.get(q.device, wsb // 4)), wsb, _lib.ptr(_ATTN_TICKETS.get(q.device, R * n_heads)))
        return _attn_call(lib, "amq_attn_decode_rows_gqa_f16", norm, (q, k, v, kcache, vcache, out), (states,), (R, n_heads, n_kv_heads, max_seq),
                          (n_splits,) + scratch)
    return _attn_call(lib, "amq_attn_decode_rows_f16", norm, (q, k, v, kcache, vcache, out), (states,), (R, n_heads, n_kv_heads, max_seq),
                      (n_splits if n_splits > 1 else 0,) + _split_scratch(lib, q.device, R, n_heads, n_splits))


def decode_tail_lookup(logits, embed, token, pos, x, state, history, table, cur, suppress=None):
    """the verify-and-propose tail of a lookup step (amq_decode_tail_lookup_f16), one launch: logits [rows, vocab], token [rows], x [rows, hidden],
    ``cur`` / ``pos`` the per-sequence step state of the rows, ``state`` / ``history`` from :func:`new_lookup_state`."""
    vocab, hidden = embed.shape
    R = token.numel()
    if not 2 <= R <= LOOKUP_MAX_ROWS:
        raise ValueError(f"rows must be 2..{LOOKUP_MAX_ROWS} (got {R})")
    _need(logits, torch.float16, "logits", R * vocab)
    _need(state, torch.int32, "lookup state", LOOKUP_STATE_WORDS)
    _need(history, torch.int32, "history")
    if suppress is not None:
        _need(suppress, torch.int32, "suppress", 8)
    seq, _, mid = _tail_args(embed, token, pos, x, table, cur)
    if not seq:
        raise ValueError(f"cur [rows, 128] / pos [rows] must be the views of one per-sequence step state of {R} blocks")
    _lib.check(_lib.load().amq_decode_tail_lookup_f16(_lib.ptr(logits), vocab, _lib.ptr(embed), hidden, *mid, R, _lib.ptr(suppress), _lib.ptr(state),
                                                      _lib.ptr(history), history.numel(), _lib.current_stream()))


def decode_tail_lookup_sample(logits, embed, token, pos, x, state, history, table, cur, sample_state, suppress=None, u=None, kept_out=None):
    """:func:`decode_tail_lookup` with every row's token drawn by :func:`sample` instead of its arg-max (amq_decode_tail_lookup_sample_f16), one
    launch: row j draws with the parameters of ``sample_state`` (:func:`new_sampling_state`) and draw counter c + j, sequence 0; the counter moves on
    by 1 + accepted drafts; no EOS bookkeeping.  ``u``: float32 [rows] uniform numbers used instead of the generator (tests); ``kept_out``: uint8
    [rows, vocab] receives the kept-set masks."""
    vocab, hidden = embed.shape
    R = token.numel()
    if not 2 <= R <= LOOKUP_MAX_ROWS:
        raise ValueError(f"rows must be 2..{LOOKUP_MAX_ROWS} (got {R})")
    _need(logits, torch.float16, "logits", R * vocab)
    _need(state, torch.int32, "lookup state", LOOKUP_STATE_WORDS)
    _need(history, torch.int32, "history")
    _need(sample_state, torch.int32, "sample_state", _SMP_WORDS)
    if suppress is not None:
        _need(suppress, torch.int32, "suppress", 8)
    if u is not None:
        _need(u, torch.float32, "u", R)
    if kept_out is not None:
        _need(kept_out, torch.uint8, "kept_out", R * vocab)
    seq, _, mid = _tail_args(embed, token, pos, x, table, cur)
    if not seq:
        raise ValueError(f"cur [rows, 128] / pos [rows] must be the views of one per-sequence step state of {R} blocks")
    _lib.check(_lib.load().amq_decode_tail_lookup_sample_f16(_lib.ptr(logits), vocab, _lib.ptr(embed), hidden, *mid, R, _lib.ptr(suppress),
                                                             _lib.ptr(state), _lib.ptr(history), history.numel(), _lib.ptr(sample_state), _lib.ptr(u),
                                                             _lib.ptr(kept_out), _lib.current_stream()))


# ---------------------------------------------------------------- the device of a launch
# Every launch goes to the CURRENT device's stream (``_lib.current_stream()``), kernel attributes and CU counts are the current device's too.  A
# process that keeps its weights on cuda:1 while cuda:0 is current (HF device_map, no set_device) must therefore have cuda:1 made current around
# the call -- the library's own guard cannot help when the stream it is handed is the null stream.  Done here, once, for every
# public entry point that takes tensors: the first CUDA tensor argument names the device; one comparison when it already is the current one.
def _on_tensor_device(fn):
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        for v in args:
            if isinstance(v, torch.Tensor) and v.is_cuda:
                if v.device.index != torch.cuda.current_device():
                    with torch.cuda.device(v.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return wrapped


for _name in ("hqq_quantize", "hqq_quantize_launch", "gptq_quantize", "gptq_quantize_launch", "gptq_quantize_static_launch", "awq_quantize", "awq_quantize_launch", "awq_clip", "awq_clip_launch", "owq_range", "owq_range_launch", "owq_select", "owq_quantize", "owq_quantize_launch", "owq_gather", "owq_outlier_add", "repack_from_hqq", "repack_from_gptq", "repack_from_awq", "dequantize", "dequantize_hqq", "dequantize_bf16", "linear_bf16", "gemv", "gemm", "gemm_f16w", "xfrag",
              "rmsnorm_xfrag", "gemm_xfrag", "gemm_xfrag_grouped", "linear", "gemv_grouped", "rmsnorm", "gemv_f16w", "lm8_gemv", "decode_tail", "sample", "logit_nll", "logit_jsd", "decode_tail_sample", "rope_cache",
              "attn_prefill", "rope_rows", "silu_mul", "gemv_qkv_attn", "attn_decode", "attn_decode_rows", "decode_tail_lookup", "decode_tail_lookup_sample"):
    globals()[_name] = _on_tensor_device(globals()[_name])
del _name

