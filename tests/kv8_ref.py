"""Reference side of the 8-bit KV cache tests (test_kv8_cpu.py, test_gpu_kv8.py).  numpy / torch; imports no kernel code.

Storage format.  Per block kc8 / vc8 int8 [B, n_kv_heads, max_seq, 128] and ks / vs fp32 [B, n_kv_heads, max_seq]: one scale per
(sequence, kv head, position), K and V separately.  A row r[0..127] is the fp16 values the fp16 cache would hold (K: after the fp16 rotation):

    a = max |r_i|                         fp32 (exact: fp16 values)
    s = a / 127                           ONE rounded fp32 division
    x_i = rint(r_i / s)                   ONE rounded fp32 division, round-half-even
    e_i = fma(-x_i, s, r_i)               ONE rounded fp32 fma: the residual r_i - x_i s (restated in fp64, where it is exact, rounded once)
    c_i = clamp(x_i + [e_i > s / 2] - [e_i < -s / 2], -127, 127)
                                          the quotient near 127 is 2^-17 coarse, so a value that close to a half step can round the wrong way;
                                          the residual moves such a code by one: |c_i s - r_i| <= s / 2 (1 + 2^-22)
    a == 0          ->  s = 0, codes 0
    inf / NaN in r  ->  s = NaN, codes 0  (the row never comes out finite)

and the value the cache stands for is fp32(c_i) * s.  `quantize` restates it with torch's fp32 operations: codes and scale bits are the kernels'.

The attention bound.  attn_decode_kv8_kernel follows the `f32` score model of attndomain_ref: s = (sum_i q_i c_ti) * s_t * (1 / sqrt 128) in fp32, never
rounded to fp16; softmax in fp32 (online, tiles of 256 keys); probabilities NOT rounded to fp16; sum_t (p_t s_t) c_ti by fp32 fma.  The bound is
attndomain_ref's, with an entry of its own in KERNELS, read off amq_attn_kv8.hip for the longest chain of the cases here (<= 1024 keys in one
workgroup = 4 tiles; <= 4 chunks):
  D = 44   l: a lane adds its 4 terms of a tile (4), wave_sum_dpp (3 + 1 DPP levels, 2 readlane levels: 6), l = l * alpha + tile sum (1): 11 per
           tile, 4 tiles.  (O: a group of 8 lanes adds its keys t = group + 32 i serially, 8 per tile x 4 tiles = 32, three shuffle levels over
           the wave's groups, three additions over the four waves: 38; several chunks: 8 + 6 + 4.)
  N = 5    4 tile rescales e^(m_old - m_new) and the final 1 / l  (2 chunks: 2 + combine + 1; 4 chunks: 1 + combine + 1)
and two terms attndomain_ref's kernels do not have, added to R here (EXTRA_REL):
  u          the product p_t * s_t, formed once per key before the fma
  6 u smax   the score itself is rounded: (raw * s_t) and its product with RN32(1 / sqrt 128) (itself u off) put at most 2 u |s| on every score and
             2 u |m| on every maximum, so every exponent's argument carries 2 u (|s| + |m|) more than the E_arg attndomain_ref counts -- three
             times (the key's exponential, the denominator's, the rescale factors), as there
The 2^-11 of R (one fp16 rounding of a probability) and A (its fp16 subnormal floor) stay in the formula although this kernel never rounds a
probability: slack, inside the same bound.  No constant is fitted to a GPU run.
"""
import numpy as np
import torch

import attndomain_ref as A

KV8 = dict(model="f32", D=44, N=5)
A.KERNELS.setdefault("kv8", KV8)
CHUNK_MIN = 256                        # ops.KV8_CHUNK_MIN: the policy's smallest chunk = one tile of the kernel
HEAD_DIM2_STEP = 1                     # the second K dimension of a head: head_dim(g) + 1
ABSMAX_DIM = 111                       # where every exact K row holds its 127 (q is 0 there: below 112, no head_dim(g) or head_dim(g) + 1 for g < 15)
Q_MULT = 4                             # q at the second dimension: raw = K[d1] + 4 K[d2] reaches +-444 with |K| <= 127


# ---------------------------------------------------------------------------------------------------------------- the quantizer
def quantize(rows):
    """rows: torch fp16 [..., 128] -> (codes int8 [..., 128], scale fp32 [...]), bit for bit what kv8_quant16 (amq_attn_kv8.hip) gives"""
    assert rows.dtype is torch.float16 and rows.shape[-1] == 128
    r = rows.detach().to(torch.float32)
    a = r.abs().amax(-1)                                         # NaN propagates (torch.amax), inf stays
    bad = ~torch.isfinite(a)
    s = a / torch.tensor(127.0, dtype=torch.float32, device=r.device)
    zero = bad | (a == 0)
    safe = torch.where(zero, torch.ones_like(s), s)
    s2 = safe.unsqueeze(-1)
    x = torch.round(r / s2)
    e = (r.double() - x.double() * s2.double()).float()          # exact in fp64, rounded once: the fp32 fma
    hs = s2 * 0.5
    c = (x + (e > hs).float() - (e < -hs).float()).clamp(-127.0, 127.0)
    c = torch.where(zero.unsqueeze(-1), torch.zeros_like(c), c)
    s = torch.where(bad, torch.full_like(s, float("nan")), s)
    return c.to(torch.int8), s


def dequantize(codes, scale):
    """-> float64 numpy [..., 128]: fp32(c) * s taken exactly"""
    c = codes.detach().cpu().numpy().astype(np.float64)
    s = scale.detach().cpu().numpy().astype(np.float64)
    return c * s[..., None]


def quant_dequant(rows, dtype=torch.float32):
    """torch: the rows an 8-bit cache stands for after storing ``rows`` (fp32 product, as the kernel forms values)"""
    c, s = quantize(rows)
    return (c.to(torch.float32) * s.unsqueeze(-1)).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- attention, fp64
def attention64(q_rot, Kd, Vd):
    """q_rot [B, nh, 128] (fp16-rotated q, any float array), Kd / Vd float64 [B, nkv, T, 128] dequantized rows 0 .. pos -> float64 [B, nh, 128]:
    softmax(q . K^T / sqrt 128) . V"""
    q = np.asarray(q_rot, np.float64)
    B, nh, _ = q.shape
    nkv, T = Kd.shape[1], Kd.shape[2]
    G = nh // nkv
    s = np.matmul(q.reshape(B, nkv, G, 128), np.swapaxes(Kd, 2, 3)) * A.SCALE          # [B, nkv, G, T]
    s = s - s.max(-1, keepdims=True)
    w = np.exp(s)
    p = w / w.sum(-1, keepdims=True)
    return np.matmul(p, Vd).reshape(B, nh, 128)


def extra_rel(smax):
    """what R of attndomain_ref lacks for this kernel (module docstring)"""
    return A.U + 6 * A.U * smax


def reference(s, V):
    """s [B, nh, T] model scores (fp64, the f32 model), V [B, nkv, T, 128] the DEQUANTIZED value rows (exactly fp16 in the exact cases)
    -> attndomain_ref.Ref(ref, bound, p) with this kernel's bound"""
    V16 = np.asarray(V, np.float16)
    assert np.array_equal(V16.astype(np.float64), np.asarray(V, np.float64)), "the exact cases keep the dequantized V rows in fp16"
    r = A.reference(s, V16, kernel="kv8")
    B, nh, T = s.shape
    nkv = V16.shape[1]
    m = s.max(-1, keepdims=True)
    smax = (np.abs(s) + np.abs(m)).max(-1, keepdims=True)                                # [B, nh, 1]
    extra = np.matmul((extra_rel(smax) * r.p).reshape(B, nkv, nh // nkv, T), np.abs(V16.astype(np.float64))).reshape(B, nh, 128)
    return A.Ref(r.ref, r.bound + extra, r.p)


# ---------------------------------------------------------------------------------------------------------------- exact-score cases
EXACT_PROFILES = A.SPLIT_PROFILES          # tied, spotlight, ramp_up, ramp_down, only_new, only_first


def exact_case(profile, B, nh, nkv, pos, seam_keys=(), rnd=0):
    """attndomain_ref.decode_case refitted to what an 8-bit cache holds exactly: the designed raw score of head g is carried by TWO K dimensions,
    raw = 1 * K[head_dim(g)] + 4 * K[head_dim(g) + 1] with |K| <= 111 (the spotlight's -444 and the +-230 of only_* do not fit one int8), every K
    row holds 127 at ABSMAX_DIM where q is 0 (scale exactly 1.0: the cache holds the integers themselves), and V = 127 at the hot index.
    -> (q, K, V fp16 numpy; raw [B, nh, T] float64, preconditions asserted)"""
    c = A.decode_case(profile, B, nh, nkv, pos, seam_keys, rnd)
    G = nh // nkv
    assert G <= 15
    q, K = c.q.copy(), np.zeros_like(c.K)
    for h in range(nh):
        d1 = A.head_dim(h % G)
        d2 = d1 + HEAD_DIM2_STEP
        raw = c.raw[:, h]                                              # [B, T] integers
        hi = np.trunc(raw / Q_MULT).astype(np.int64)
        lo = raw - Q_MULT * hi
        assert np.abs(hi).max() <= 127 and np.abs(lo).max() < Q_MULT
        q[:, h, d2] = Q_MULT
        K[:, h // G, :, d1] = lo
        K[:, h // G, :, d2] = hi
    assert (q[:, :, ABSMAX_DIM] == 0).all()
    K[..., ABSMAX_DIM] = 127
    V = (c.V.astype(np.float32) * 127).astype(np.float16)
    raw = A.raw_scores(q, K)                                           # asserts integers, |raw| <= 2048, check_exact
    assert np.array_equal(raw, c.raw.astype(np.float64)), "the refit changed a designed score"
    assert np.abs(K).max() == 127 and (np.abs(K).max(-1) == 127).all()
    return q, K, V, raw


# ---------------------------------------------------------------------------------------------------------------- whole model, stepwise
def _rms(x, g, eps):
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).half() * g


class StepModel:
    """_ref_forward of tests/test_gpu_decode.py restated with a per-block cache: exact causal fp16 attention for the prompt rows; every cached row
    is the quantize-then-dequantize of the fp16 row; a decode row attends the dequantized rows 0 .. pos (its own included) with fp32 scores,
    fp32 softmax and unrounded probabilities.  Fed the runner's own tokens.  ``blocks``: dicts of dense fp16 weights + ln1 / ln2 (test-side)."""

    def __init__(self, embed, norm, lm_head, blocks, nh, nkv, eps=1e-5, theta=10000.0):
        self.embed, self.norm, self.lm_head, self.blocks, self.nh, self.nkv, self.eps = embed, norm, lm_head, blocks, nh, nkv, eps
        self.inv = 1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float32, device=embed.device) / 128.0))
        self.K = [None] * len(blocks)
        self.V = [None] * len(blocks)
        self.pos = 0

    def _rope(self, t, pos):
        fr = pos.float()[:, None] * self.inv[None]
        emb = torch.cat([fr, fr], -1)
        cos, sin = emb.cos().half()[:, None], emb.sin().half()[:, None]
        return t * cos + torch.cat([-t[..., 64:], t[..., :64]], -1) * sin

    def _mlp(self, x, d):
        import torch.nn.functional as F
        h2 = _rms(x, d["ln2"], self.eps)
        return x + F.linear(F.silu(F.linear(h2, d["mlp.gate_proj"])) * F.linear(h2, d["mlp.up_proj"]), d["mlp.down_proj"])

    def _logits(self, x):
        import torch.nn.functional as F
        return F.linear(_rms(x[-1:], self.norm, self.eps), self.lm_head)[0]

    def prompt(self, ids):
        import torch.nn.functional as F
        S, nh, nkv, G = ids.numel(), self.nh, self.nkv, self.nh // self.nkv
        x = self.embed.index_select(0, ids)
        pos = torch.arange(S, device=ids.device)
        for i, d in enumerate(self.blocks):
            h = _rms(x, d["ln1"], self.eps)
            q = self._rope(F.linear(h, d["self_attn.q_proj"]).view(S, nh, 128), pos).transpose(0, 1)
            k = self._rope(F.linear(h, d["self_attn.k_proj"]).view(S, nkv, 128), pos).transpose(0, 1)
            v = F.linear(h, d["self_attn.v_proj"]).view(S, nkv, 128).transpose(0, 1)
            self.K[i], self.V[i] = quant_dequant(k.contiguous()), quant_dequant(v.contiguous())          # what the cache stands for
            w = torch.matmul(q, k.repeat_interleave(G, 0).transpose(1, 2)) * (128 ** -0.5)
            w = w + torch.full((S, S), float("-inf"), device=ids.device).triu(1).half()
            a = torch.matmul(torch.softmax(w.float(), -1).half(), v.repeat_interleave(G, 0)).transpose(0, 1).reshape(S, nh * 128)
            x = self._mlp(x + F.linear(a, d["self_attn.o_proj"]), d)
        self.pos = S
        return self._logits(x)

    def step(self, token):
        import torch.nn.functional as F
        nh, nkv, G = self.nh, self.nkv, self.nh // self.nkv
        x = self.embed.index_select(0, token.reshape(1))
        pos = torch.full((1,), self.pos, device=token.device)
        for i, d in enumerate(self.blocks):
            h = _rms(x, d["ln1"], self.eps)
            q = self._rope(F.linear(h, d["self_attn.q_proj"]).view(1, nh, 128), pos)[0]                  # [nh, 128]
            k = self._rope(F.linear(h, d["self_attn.k_proj"]).view(1, nkv, 128), pos).transpose(0, 1)    # [nkv, 1, 128]
            v = F.linear(h, d["self_attn.v_proj"]).view(1, nkv, 128).transpose(0, 1)
            self.K[i] = torch.cat([self.K[i], quant_dequant(k.contiguous())], 1)
            self.V[i] = torch.cat([self.V[i], quant_dequant(v.contiguous())], 1)
            w = torch.einsum("hd,htd->ht", q.float(), self.K[i].repeat_interleave(G, 0)) * (128 ** -0.5)
            a = torch.einsum("ht,htd->hd", torch.softmax(w, -1), self.V[i].repeat_interleave(G, 0)).half().reshape(1, nh * 128)
            x = self._mlp(x + F.linear(a, d["self_attn.o_proj"]), d)
        self.pos += 1
        return self._logits(x)
