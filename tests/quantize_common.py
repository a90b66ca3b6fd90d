"""What the tests of the three device quantizers (HQQ, GPTQ, AWQ: tests/test_gpu_*_quantize.py, test_gpu_quantize_shared.py) share: Format A read
back to codes, its shapes and dtypes, bit-for-bit comparison, and the digests of HQQ results (tests/golden/hqq_digests.json)."""
import hashlib
import struct

import torch

from amq_amd import hqq_format


def unpack_rows(W_q, nbits, R):
    """Format A -> [R, G] integer codes (the inverse of hqq_format.pack_rows)"""
    if nbits == 4:
        return torch.cat([W_q >> 4, W_q & 15]).to(torch.int32)
    if nbits == 2:
        return torch.cat([(W_q >> 6) & 3, (W_q >> 4) & 3, (W_q >> 2) & 3, W_q & 3]).to(torch.int32)
    return torch.cat([(W_q >> (27 - 3 * c)) & 7 for c in range(10)])[:R].to(torch.int32)


def same_bits(a, b):
    view = {torch.float16: torch.int16, torch.float32: torch.int32}.get(a.dtype)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return torch.equal(a.view(view), b.view(view)) if view else torch.equal(a, b)


def assert_format_a(h, nbits, group, shape):
    """Format A's shapes and dtypes for a layer [N, K]"""
    N, K = shape
    R = N * K // group
    assert tuple(h.shape) == (N, K) and h.nbits == nbits and h.group_size == group
    if nbits == 3:
        assert h.W_q.dtype == torch.int32 and tuple(h.W_q.shape) == ((R + 9) // 10, group)
    else:
        assert h.W_q.dtype == torch.uint8 and tuple(h.W_q.shape) == (R * nbits // 8, group)
    assert h.scale.dtype == torch.float16 and h.zero.dtype == torch.float16 and tuple(h.scale.shape) == (R, 1) == tuple(h.zero.shape)


def assert_codes(h, codes):
    """the packed layer holds ``codes`` [R, G]: as codes, and as words over the WHOLE tensor (the unpacked view drops the padding of the last
    3-bit words, which must be zeros)"""
    q = unpack_rows(h.W_q.cpu(), h.nbits, codes.shape[0])
    assert torch.equal(q, codes.to(torch.int32)), f"codes: {int((q != codes).sum())} of {q.numel()} differ"
    want = hqq_format.pack_rows(codes, h.nbits)
    assert h.W_q.dtype == want.dtype and torch.equal(h.W_q.cpu(), want), "packed words (padding bits included)"


# ---------------------------------------------------------------------------------------------------------------- HQQ digests
# (48, 256) at every group and bit-width; (48, 11008) / 64 at 3 bits: three passes per wave, several chunks of the stop kernel
HQQ_DIGEST_CASES = [(48, 256, g, b) for g in (32, 64, 128, 256) for b in (2, 3, 4)] + [(48, 11008, 64, 3)]


def hqq_digest_key(N, K, group, bits):
    return f"{N}x{K}_g{group}_b{bits}"


def hqq_digest(h, info):
    """sha256 of the bytes of W_q, scale, zero and the 88-byte info block {int32 stop, int32 nonfinite, float mean_err[20]} of one
    ops.hqq_quantize(..., return_info=True)"""
    def sha(b):
        return hashlib.sha256(b).hexdigest()

    block = struct.pack("<ii", info.stop, info.nonfinite) + info.mean_err.cpu().contiguous().numpy().tobytes()
    assert len(block) == 88
    return {"W_q": sha(h.W_q.cpu().contiguous().numpy().tobytes()), "scale": sha(h.scale.cpu().contiguous().view(torch.int16).numpy().tobytes()),
            "zero": sha(h.zero.cpu().contiguous().view(torch.int16).numpy().tobytes()), "info": sha(block)}
