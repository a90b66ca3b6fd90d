"""Torch restatement of the 8-bit lm_head ("LM8") for the tests: the quantizer, the weights a layer stands for, the normed x of
the GEMV's prologue.  Written from the format's definition, not from amq_amd.hqq_format.

Format: codes uint8 [N, K]; meta fp16 [N, K / 128, 2] = (scale, zero) per group of 128 along K; the stored scale multiplies, the zero is fractional.
Weight of a code c:   w = fp16(fp16(fp16(c) - zero) * scale)   -- two fp16 roundings (fp16(c) is exact for c <= 255)."""
import torch

GROUP = 128


def quantize(W):
    """min/max round to nearest at 8 bits, HQQ's Quantizer.quantize(nbits=8, optimize=False, axis=1, group_size=128) -> (codes uint8 [N, K],
    meta fp16 [N, K / 128, 2]): fp32 statistics per group, scale 255 / (max - min) (1 where the range is <= 1e-4; at most 2e4), zero = -min * scale,
    codes = round(w * scale + zero) clamped to 0 .. 255, the stored scale is the inverse"""
    n, k = W.shape
    g = W.to(torch.float32).reshape(n * k // GROUP, GROUP)
    lo, hi = g.amin(dim=1, keepdim=True), g.amax(dim=1, keepdim=True)
    rng = hi - lo
    s = torch.where(rng.abs() <= 1e-4, torch.ones_like(rng), 255.0 / rng)
    s = torch.minimum(s, torch.full_like(s, 2e4))
    z = -lo * s
    q = torch.clamp(torch.round(g * s + z), 0.0, 255.0)
    meta = torch.stack([(1.0 / s).reshape(-1).to(torch.float16), z.reshape(-1).to(torch.float16)], dim=1)
    return q.to(torch.uint8).reshape(n, k), meta.reshape(n, k // GROUP, 2)


def _f16_round(t32):
    return t32.to(torch.float16)


def dequantize(codes, meta):
    """the weights [N, K] fp16, bit for bit: every operation in fp32 on fp16 operands (exact: an fp16 difference or product has at most 22
    significant bits) and rounded to fp16 once -- the fp16 subtract and the fp16 multiply of the reference's dequantize()"""
    n, k = codes.shape
    c = codes.to(torch.float32).reshape(n, k // GROUP, GROUP)
    scale = meta[..., 0:1].to(torch.float32)
    zero = meta[..., 1:2].to(torch.float32)
    d = _f16_round(c - zero).to(torch.float32)
    return _f16_round(d * scale).reshape(n, k)


def rmsnorm_f16(x, gamma, eps):
    """the GEMV's prologue (and ops.rmsnorm): gamma * fp16(x * rsqrt(mean x^2 + eps)), fp32 statistic"""
    xf = x.to(torch.float32)
    rstd = torch.rsqrt((xf * xf).mean(dim=-1, keepdim=True) + eps)
    return (gamma.to(torch.float32) * (xf * rstd).to(torch.float16).to(torch.float32)).to(torch.float16)


def step_bound(W, meta):
    """the derived bound of |dequantize(quantize(W)) - W| per element, [N, K] fp32, for groups whose (scale, zero) are finite in fp16.
    With s = the fp32 multiplier 1 / scale_q and s16 = fp16(s), z16 = fp16(zero):
      - rounding to the nearest code (clamping only pulls a code towards the value's own side): |(c - z) s - w| <= s / 2;
      - fp16(zero): |z16 - z| <= ulp16(z) / 2, times s;
      - fp16(c - z16): half an ulp of the difference, times s;
      - fp16(s): |c - z16| * ulp16(s) / 2;
      - the product's rounding: half an ulp of the result.
    ulp16(v) = 2^(floor(log2 |v|) - 10), at least 2^-24."""
    n, k = W.shape
    s16 = meta[..., 0:1].to(torch.float32)
    z16 = meta[..., 1:2].to(torch.float32)

    def ulp(v):
        e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
        return torch.exp2(e - 10.0).clamp_min(2.0 ** -24)

    span = torch.maximum(z16.abs(), (255.0 - z16).abs()) + 1.0      # |c - z16| <= span
    w_abs = W.to(torch.float32).abs().reshape(n, k // GROUP, GROUP)
    # the first three terms are in units of s <= s16 (1 + 2^-11); the result is below |w| + s16 in magnitude, and a whole ulp of that (not half)
    # is allowed for the last rounding so that a result in the binade above |w| + s16's is covered
    b = (0.5 + 0.5 * ulp(z16) + 0.5 * ulp(span)) * s16 * (1.0 + 2.0 ** -10) + 0.5 * span * ulp(s16) + ulp(w_abs + s16)
    return b.reshape(n, k)
