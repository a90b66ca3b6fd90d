"""Reference side of the attention-domain tests (test_attndomain_cpu.py, test_gpu_attndomain.py): inputs on which every attention score is known
EXACTLY, the two score models the kernel families implement, an fp64 softmax . V with a DERIVED error bound per kernel, the keys each kernel's
structure makes special (seams), and the case table both test modules walk.  Plain numpy; imports no kernel code.

Exact scores.  q and every K row hold small integers, so every raw score q . k is an integer, |q . k| <= 2048: every product and every partial
sum is an integer below 2^24 -- exact in fp32 whatever the order (v_dot2, DPP sums, MFMA) -- and fp16(q . k) is exact.  The rotation is handed
(cos 1, sin 0): q' = q * 1 + (-q2) * 0 = q.  V is address-coded (one-hot rows): out[h, d] is the sum of the probabilities of the keys given
dimension d.

The two score models (SCALE32 = 0x3DB504F3 = RN32(1 / sqrt 128)):
  eager   attn_decode_kernel, attn_decode_split_kernel (amq_decode.hip `score`): s = RN16(RN32(RN16(q . k)) * rsqrtf(128.f)) -- one rounding, as
          numpy's float32 * float32 -> float16.  rsqrtf may be folded or taken by v_rsq_f32 (1 ulp): raw values whose score moves under
          SCALE32 -+ 1 ulp are AMBIGUOUS (+-1189: found by ambiguous_raws(), kept out of every case by check_exact()).
  f32     attn_prefill_kernel, attn_decode_gqa_kernel (+ attn_gqa_combine_kernel): s = (q . k) / sqrt(128) in fp32, never rounded to fp16 (the
          kernel works in the exp2 domain with sl2 = RN32(RN32(1 / sqrt 128) * RN32(log2 e)): its distance from the real product is an fp32
          term of the bound).
The three roundings of a probability:
  single workgroup, and the split kernel with ONE active chunk   p = RN16(RN32(e^(s - m) * (1 / l)))      normalised, then rounded (HF eager)
  split kernel, several chunks                                   e^(s - m_z) stays fp32, O / L at the end  never rounded
  matrix-core kernels                                            RN16(exp2((s - m_run) sl2)), m_run the RUNNING maximum of the lane's row when
                                                                 the key's tile is taken; rescaled by exp2((m_run - m_new) sl2) in fp32 later

The bound, per output element d (u = 2^-24, fp32's unit roundoff; p_t the fp64 model probability; first order):

    |out_d - ref_d|  <=  sum_t (R p_t + A) |v_td|  +  2^-11 |ref_d|  +  2^-25

  2^-11 |ref_d| + 2^-25   the output's own rounding to fp16 (2^-25: half the subnormal spacing, for |out| < 2^-14)
  A = 2^-24               the fp16 subnormal floor of a probability below 2^-14 of its reference maximum: absolute 2^-25 (half of the spacing
                          2^-24), doubled because the reference maximum at rounding time (running maximum / normaliser) is not the final one and
                          the value is rescaled in fp32 afterwards; dividing by l >= 1 only shrinks it
  R = 2^-11               the ONE fp16 rounding of a probability (none in the several-chunk split kernel: inside the same bound)
    + 2 (E_exp + D u)     numerator and denominator each: E_exp = 4 u (__expf = v_exp_f32 of a product, __builtin_amdgcn_exp2f: taken at 2 ulp);
                          D u: a sum of non-negative fp32 terms along a chain of D additions carries at most D u relative error
    + 3 E_arg             the exponent's argument: s - m and its product with log2 e (eager) / the fma s * sl2 - m * sl2 with sl2 2^-24 off
                          (f32): at most 2 u (|s| + |m|) absolute in the natural domain = relative in the exponential; once for the key's own
                          exponential, once for the denominator's, once for the rescale factors between the key's tile / chunk and the end
                          (their argument errors add up to that of one difference of maxima: they telescope).  |s| + |m| is taken from the
                          case's model scores (<= 128: the cases keep |s| <= 64)
    + N (E_exp + 2 u)     N multiplicative steps between a term and the result -- running-maximum rescales exp2((m_run - m_new) sl2), the
                          cross-wave merge factor, the combine's e^(m_c - M), the final 1 / l -- each an exponential and one rounding on the
                          O side and one on the l side

D and N per kernel, read off the code for the LONGEST chain of the cases below (KERNELS):
  single   attn_decode_kernel, T <= 1024.  l: <= 2 terms per thread, wave_sum_dpp 6, 8 wave partials: 15.  O: a 16-lane group adds its keys
           t = grp + 32 i serially: <= 32, then part[32] serially: 32.  D = 64; N = 1 (sc * inv with inv = 1 / tot)
  split    attn_decode_split_kernel, chunks <= 768 keys, <= 16 chunks.  O: 24 per group + 32 groups + 16 chunks in the last arriver: D = 72
           (l: 2 + 6 + 8 + 16 = 32); N = 2 (e^(m_c - M), O / L)
  gqa      attn_decode_gqa_kernel + attn_gqa_combine_kernel, <= 11 stages per workgroup, <= 40 chunks.  O: one 16x16x32 MFMA per stage (32
           products into the accumulator) x 11, 4 waves merged, 40 chunks: 352 + 4 + 40 = 396 (l: (8 + 1) x 11 + 2 shuffles + 4 + 40 = 145).
           D = 396; N = 11 stage rescales + merge + combine + O / L = 14
  prefill  attn_prefill_kernel, <= 4 key tiles (S + pos0 <= 200).  O: two 32-key MFMAs per tile x 4 = 256 (l: (8 + 2) x 4 + 2 shuffles = 42).
           D = 256; N = 4 rescales + 1 / l = 5
No constant above is fitted to a GPU run.
"""
import collections
import functools

import numpy as np

U = 2.0 ** -24
A = 2.0 ** -24
OUT_FLOOR = 2.0 ** -25
E_EXP = 4 * U
SCALE32 = np.array([0x3DB504F3], np.uint32).view(np.float32)[0]
SCALE = 128.0 ** -0.5
RAW_MAX = 2048
S_MAX = 64.0                          # |scaled score| the cases stay under
KERNELS = {                           # model, D, N (module docstring)
    "single": dict(model="eager", D=64, N=1),
    "split": dict(model="eager", D=72, N=2),
    "gqa": dict(model="f32", D=396, N=14),
    "prefill": dict(model="f32", D=256, N=5),
}
ATT_GROUPS, ATT_SPEC, ATT_PF = 32, 2, 12          # amq_decode.hip: 16-lane groups per workgroup, speculative / prefetched rows per group
ATT_MIN_CHUNK = 256                               # amq_kernels.h
TILE, STAGE = 64, 128                             # amq_attn_prefill.hip: AP_BKV, AG_STAGE_KEYS
PROFILES = ("tied", "spotlight", "ramp_up", "ramp_down", "only_new", "only_first", "integers")
LADDER_MAX = 24                                   # seam keys per head of a spotlight launch
BG_GAP = 444                                      # raw: 444 / sqrt(128) = 39.2 (eager: RN16 -> 39.25)
ONLY = 230                                        # raw: +-230 -> scaled gap 40.6
BG_DIM = 127                                      # the V dimension that collects a spotlight's background

Ref = collections.namedtuple("Ref", "ref bound p")


def _scaled16(raw, scale32):
    return (np.asarray(raw, np.float32) * np.float32(scale32)).astype(np.float16)


@functools.lru_cache(maxsize=None)
def ambiguous_raws():
    """raw scores in [-2048, 2048] whose eager score depends on the last bit of the kernel's scale (rsqrtf(128.f) folded or not)"""
    raw = np.arange(-RAW_MAX, RAW_MAX + 1)
    s = _scaled16(raw, SCALE32)
    bits = np.array([0x3DB504F3 - 1, 0x3DB504F3 + 1], np.uint32).view(np.float32)
    bad = (_scaled16(raw, bits[0]) != s) | (_scaled16(raw, bits[1]) != s)
    return tuple(int(r) for r in raw[bad])


def raw_scores(q, K):
    """q [B, nh, 128] or [B, nh, S, 128], K [B, nkv, T, 128] (fp16, integers) -> the integer scores [B, nh, (S,) T] as float64, preconditions asserted"""
    q, K = np.asarray(q, np.float16), np.asarray(K, np.float16)
    for a in (q, K):
        assert np.isfinite(a).all() and (a == np.round(a)).all(), "q and K must hold integers"
    dec = q.ndim == 3
    q4 = q[:, :, None, :] if dec else q
    B, nh, S, _ = q4.shape
    nkv, T = K.shape[1], K.shape[2]
    G = nh // nkv
    # integers below 2^24 at every partial sum: exact in fp32, in any order
    assert float(np.abs(q4.astype(np.float64)).max(initial=0)) * float(np.abs(K.astype(np.float64)).max(initial=0)) * 128 < 2 ** 24
    raw = np.matmul(q4.astype(np.float32).reshape(B, nkv, G * S, 128), K.astype(np.float32).transpose(0, 1, 3, 2)).reshape(B, nh, S, T).astype(np.float64)
    check_exact(raw)
    return raw[:, :, 0] if dec else raw


def check_exact(raw):
    raw = np.asarray(raw, np.float64)
    assert (raw == np.round(raw)).all() and np.abs(raw).max(initial=0) <= RAW_MAX, "raw scores must be integers within +-2048"
    assert not np.isin(raw, ambiguous_raws()).any(), "a raw score whose fp16 scaled value depends on the last bit of the scale"
    assert np.abs(raw).max(initial=0) * SCALE <= S_MAX, "scaled scores beyond 64"


def eager_round(raw):
    """the VALU kernels' rounding of a raw score (no precondition: also what HF's fp16 eager expression does to an fp16 matmul result)"""
    return _scaled16(np.asarray(raw, np.float16), SCALE32).astype(np.float64)


def scores_eager(q, K):
    return eager_round(raw_scores(q, K))


def scores_f32(q, K):
    return raw_scores(q, K) * SCALE


def scores(kernel, q, K):
    return scores_eager(q, K) if KERNELS[kernel]["model"] == "eager" else scores_f32(q, K)


def rel_bound(kernel, smax):
    """R of the module docstring; smax = max (|s| + |m|) over the visible keys, from the model scores"""
    k = KERNELS[kernel]
    return 2.0 ** -11 + 2 * (E_EXP + k["D"] * U) + 3 * 2 * U * smax + k["N"] * (E_EXP + 2 * U)


def reference(s, V, mask=None, kernel="single"):
    """s [B, nh, (S,) T] model scores (fp64), V [B, nkv, T, 128], mask like s (True = visible; None: all) -> Ref(ref, bound, p), fp64:
    ref = sum_t p_t v_t [B, nh, (S,) 128], the derived bound at every element, the probabilities"""
    s = np.asarray(s, np.float64)
    dec = s.ndim == 3
    s4 = s[:, :, None, :] if dec else s
    B, nh, S, T = s4.shape
    V = np.asarray(V, np.float16).astype(np.float64)
    nkv = V.shape[1]
    G = nh // nkv
    vis = np.ones(s4.shape, bool) if mask is None else np.broadcast_to(np.asarray(mask, bool)[:, :, None, :] if dec else np.asarray(mask, bool), s4.shape)
    assert vis.any(-1).all()
    sm = np.where(vis, s4, -np.inf)
    m = sm.max(-1, keepdims=True)
    w = np.exp(sm - m)
    p = w / w.sum(-1, keepdims=True)
    Vv = np.where(np.isnan(V), 0.0, V)                                  # rows past the context (NaN): no visible key points there
    assert not (np.isnan(V).any(-1)[:, :, None, :] & vis.reshape(B, nkv, G * S, T)).any(), "a visible key with a NaN value row"
    pg = p.reshape(B, nkv, G * S, T)
    ref = np.matmul(pg, Vv).reshape(B, nh, S, 128)
    smax = np.where(vis, np.abs(s4) + np.abs(m), 0.0).max(-1, keepdims=True)         # [B, nh, S, 1]
    R = rel_bound(kernel, smax)
    absv = np.abs(Vv)
    bound = (np.matmul((R * p).reshape(B, nkv, G * S, T), absv) + A * np.matmul(vis.reshape(B, nkv, G * S, T).astype(np.float64), absv)).reshape(B, nh, S, 128)
    bound = bound + 2.0 ** -11 * np.abs(ref) + OUT_FLOOR
    if dec:
        return Ref(ref[:, :, 0], bound[:, :, 0], p[:, :, 0])
    return Ref(ref, bound, p)


# ------------------------------------------------------------------------------------------------------------------ kernel structure
def split_chunk(T, n_splits):
    """attn_decode_split_kernel: keys per workgroup at T = pos + 1"""
    return max(ATT_MIN_CHUNK, ((T + n_splits - 1) // n_splits + 31) // 32 * 32)


def gqa_chunk(max_seq, n_splits):
    """attn_decode_gqa_kernel: whole stages of 128 keys, from the cache length (attn_decode_gqa_iters)"""
    return STAGE * -(-(-(-max_seq // n_splits)) // STAGE)


def chunk_of(kernel, pos, max_seq, n_splits):
    if kernel == "split":
        return split_chunk(pos + 1, n_splits)
    if kernel == "gqa":
        return gqa_chunk(max_seq, n_splits)
    return None


def seams(kernel, pos, chunk=None):
    """the keys 0 .. pos a kernel's structure makes special, sorted: always 0, 1, pos - 1, pos (the new token: from LDS, not the cache); the group
    stride 32 and the register prefetch limits (ATT_SPEC, ATT_PF: 64 / 384 keys); tiles of 64 and stages of 128 keys; every chunk boundary
    (which holds chunks 7 / 8 and 15 / 16 of the split kernel's combine batches and 31 / 32, 47 / 48 of the grouped combine launch); the split
    kernel's prefetch limit inside every chunk; the grouped kernel's last tile and stage"""
    ks = {0, 1, pos - 1, pos}
    if kernel in ("single", "split"):
        for e in (ATT_GROUPS, ATT_GROUPS * ATT_SPEC, ATT_GROUPS * ATT_PF):
            ks |= {e - 1, e, e + 1}
    ks |= {TILE - 1, TILE, TILE + 1, STAGE - 1, STAGE, STAGE + 1}
    if chunk:
        for c in range(1, pos // chunk + 1):
            ks |= {c * chunk - 1, c * chunk}
    if kernel == "split" and chunk > ATT_GROUPS * ATT_PF:            # the prefetch limit counts from the chunk's first key: the remainder loop of every chunk
        for c in range(pos // chunk + 1):
            ks |= {c * chunk + ATT_GROUPS * ATT_PF + e for e in (-1, 0, 1)}
    if kernel == "gqa":                                              # the tile and the stage the new token sits in (the last chunk may end mid-stage)
        ks |= {pos // TILE * TILE - 1, pos // TILE * TILE, pos // STAGE * STAGE - 1, pos // STAGE * STAGE}
    return sorted(k for k in ks if 0 <= k <= pos)


# ------------------------------------------------------------------------------------------------------------------ decode cases
def head_dim(g):
    """the K dimension head g of a kv group reads its designed score from (q = e_dim there): distinct for g < 16, below 112"""
    return 7 * g + 3


Case = collections.namedtuple("Case", "profile q K V raw held dims")
Case.__doc__ = """q [B, nh, 128], K / V [B, nkv, T, 128] fp16 (row T - 1 = the new token's key / value), raw [B, nh, T] the designed scores,
held [B][nh] -> the keys whose loss this case must show, dims [B][nkv] -> {key: V dimension} of a spotlight (else None)"""


def ladder_capacity(nh, nkv):
    G = nh // nkv
    return min(LADDER_MAX, 120 // G)


def spotlight_rounds(n_seams, B, nh, nkv):
    """launches a spotlight needs for every seam key to sit on some head's ladder"""
    return max(1, -(-n_seams // (B * nh * ladder_capacity(nh, nkv))))


def decode_case(profile, B, nh, nkv, pos, seam_keys=(), rnd=0, dense_v=False, seed=0):
    """one decode step at position pos: (q, K, V) with K / V rows 0 .. pos (row pos: the new token).  Every designed profile gives head g of a kv
    group its own K dimension (head_dim), so the heads of a group see different distributions over the same rows; q carries junk integers in
    dimensions >= 112, where K is zero.  seam_keys / rnd: the spotlight's keys and which slice of them this launch holds."""
    assert profile in PROFILES
    G, T = nh // nkv, pos + 1
    rng = np.random.default_rng([seed, PROFILES.index(profile), B, nh, nkv, pos, rnd])
    t = np.arange(T)
    raw = np.zeros((B, nh, T), np.int64)
    held = [[[] for _ in range(nh)] for _ in range(B)]
    dims = [[None] * nkv for _ in range(B)]
    V = np.zeros((B, nkv, T, 128), np.float16)
    V[:, :, t, t % 128] = 1.0
    if profile == "integers":
        q = rng.integers(-4, 5, (B, nh, 128)).astype(np.float16)
        K = rng.integers(-4, 5, (B, nkv, T, 128)).astype(np.float16)
        for _ in range(8):                                            # a row that makes an ambiguous raw score is drawn again
            r = np.matmul(q.astype(np.float32).reshape(B, nkv, G, 128), K.astype(np.float32).transpose(0, 1, 3, 2))
            bad = np.isin(r, ambiguous_raws()).any(2)                  # [B, nkv, T]
            if not bad.any():
                break
            K[bad] = rng.integers(-4, 5, (int(bad.sum()), 128)).astype(np.float16)
        raw = r.reshape(B, nh, T).astype(np.int64)
    else:
        cap = ladder_capacity(nh, nkv)
        n = len(seam_keys)
        for b in range(B):
            for h in range(nh):
                g = h % G
                if profile == "tied":
                    raw[b, h] = 2 * (1 + (h + b) % 5)
                    held[b][h] = list(seam_keys)
                elif profile == "spotlight":
                    slot = (rnd * B + b) * nh + h
                    mine = [seam_keys[(slot * cap + j) % n] for j in range(min(cap, n))]
                    mine = list(dict.fromkeys(mine))
                    rungs = 2 * rng.permutation(len(mine))             # distinct even raw scores 0 .. 2 (n - 1), shuffled over the keys
                    raw[b, h] = -BG_GAP
                    raw[b, h, mine] = rungs
                    held[b][h] = mine
                elif profile in ("ramp_up", "ramp_down"):
                    step = 2 + 2 * ((g + b) % 3)
                    lv = t // ATT_GROUPS
                    mid = (lv.max() + 1) // 2
                    if profile == "ramp_up":
                        raw[b, h] = step * (lv - mid)
                        raw[b, h, pos] = raw[b, h, :].max() + 2       # the new token is the largest
                    else:
                        raw[b, h] = -step * (lv - mid)
                        raw[b, h, 0] = raw[b, h].max() + 20            # key 0 is the sink
                        raw[b, h, pos] = raw[b, h].min() - 2
                elif profile in ("only_new", "only_first"):
                    raw[b, h] = -ONLY - 2 * (t % 5)
                    raw[b, h, pos if profile == "only_new" else 0] = ONLY
        if profile == "spotlight":
            V[:] = 0
            for b in range(B):
                for kv in range(nkv):
                    ks = sorted({k for g in range(G) for k in held[b][kv * G + g]})
                    assert len(ks) <= BG_DIM
                    dims[b][kv] = {k: i for i, k in enumerate(ks)}
                    V[b, kv, :, BG_DIM] = 1.0
                    for k, d in dims[b][kv].items():
                        V[b, kv, k, BG_DIM] = 0.0
                        V[b, kv, k, d] = 1.0
        q = np.zeros((B, nh, 128), np.float16)
        q[:, :, 112:] = rng.integers(-4, 5, (B, nh, 16))
        K = np.zeros((B, nkv, T, 128), np.float16)
        for h in range(nh):
            q[:, h, head_dim(h % G)] = 1.0
            K[:, h // G, :, head_dim(h % G)] = raw[:, h]
    if dense_v:
        V = rng.integers(1, 5, (B, nkv, T, 128)).astype(np.float16)        # positive: no cancellation for the bound to hide in
    return Case(profile, q, K, V, raw, held, dims)


def held_keys(case, p, b, h):
    """the keys of head (b, h) whose loss, doubling or replacement the case must show: a designed profile's seam keys, else every key the model
    gives a probability >= 2e-3"""
    if case.profile in ("tied", "spotlight"):
        return list(case.held[b][h])
    return [int(k) for k in np.nonzero(p[b, h] >= P_HELD)[0]]


# ------------------------------------------------------------------------------------------------------------------ prompt cases
PREFILL_PROFILES = ("tied", "ramp_up", "ramp_down", "only_first", "integers")
PCase = collections.namedtuple("PCase", "profile q K V raw")
PCase.__doc__ = "q [B, nh, S, 128] (rotated), K / V [B, nkv, T, 128] with T = pos0 + S, raw [B, nh, S, T]"


def prefill_case(profile, B, nh, nkv, S, pos0=0, dense_v=False, seed=0):
    """a prompt chunk of S rows behind pos0 cached keys; query row i multiplies its head's designed key score by 1 + (i + h) % 2 (3 for the ramps'
    third of the rows): every row its own distribution"""
    assert profile in PREFILL_PROFILES
    G, T = nh // nkv, pos0 + S
    rng = np.random.default_rng([seed, 100 + PREFILL_PROFILES.index(profile), B, nh, nkv, S, pos0])
    t = np.arange(T)
    V = np.zeros((B, nkv, T, 128), np.float16)
    V[:, :, t, t % 128] = 1.0
    if profile == "integers":
        q = rng.integers(-4, 5, (B, nh, S, 128)).astype(np.float16)
        K = rng.integers(-4, 5, (B, nkv, T, 128)).astype(np.float16)
        for _ in range(8):
            r = np.matmul(q.astype(np.float32).reshape(B, nkv, G * S, 128), K.astype(np.float32).transpose(0, 1, 3, 2))
            bad = np.isin(r, ambiguous_raws()).any(2)
            if not bad.any():
                break
            K[bad] = rng.integers(-4, 5, (int(bad.sum()), 128)).astype(np.float16)
        raw = r.reshape(B, nh, S, T).astype(np.int64)
    else:
        key = np.zeros((B, nh, T), np.int64)
        for b in range(B):
            for h in range(nh):
                if profile == "tied":
                    key[b, h] = 2 * (1 + (h + b) % 5)
                elif profile == "ramp_up":
                    key[b, h] = t - T // 2
                elif profile == "ramp_down":
                    key[b, h] = T // 2 - t
                    key[b, h, 0] += 20
                else:
                    key[b, h] = -ONLY - 2 * (t % 5)
                    key[b, h, 0] = ONLY
        mult = np.zeros((B, nh, S), np.int64)
        i = np.arange(S)
        for h in range(nh):
            mult[:, h] = 1 + (i + h) % (3 if profile.startswith("ramp") else 2)
        raw = mult[:, :, :, None] * key[:, :, None, :]
        q = np.zeros((B, nh, S, 128), np.float16)
        q[..., 112:] = rng.integers(-4, 5, (B, nh, S, 16))
        K = np.zeros((B, nkv, T, 128), np.float16)
        for h in range(nh):
            q[:, h, :, head_dim(h % G)] = mult[:, h]
            K[:, h // G, :, head_dim(h % G)] = key[:, h]
    if dense_v:
        V = rng.integers(1, 5, (B, nkv, T, 128)).astype(np.float16)        # positive: no cancellation for the bound to hide in
    return PCase(profile, q, K, V, raw)


def causal_mask(S, pos0, shift=0):
    """[S, T]: row i sees keys 0 .. pos0 + i (+ shift: the mask moved by one, for the mutation check)"""
    return np.arange(pos0 + S)[None, :] <= (pos0 + np.arange(S) + shift)[:, None]


# ------------------------------------------------------------------------------------------------------------------ the case tables
ALL = PROFILES
FEW = ("tied", "spotlight")
SPLIT_PROFILES = ("tied", "spotlight", "ramp_up", "ramp_down", "only_new", "only_first")

SINGLE_POS = (0, 1, 31, 32, 63, 64, 383, 384, 385, 700, 1023)
SINGLE_HEADS = ((2, 2), (4, 1))
# (max_seq, n_splits, pos): attn_decode_split_kernel, heads (2, 2)
SPLIT_SHAPES = tuple((1024, 4, p) for p in (255, 256, 257, 511, 512, 1023)) + ((4096, 16, 4000), (4096, 4, 3000))
# (max_seq, n_splits, pos): attn_decode_gqa_kernel + attn_gqa_combine_kernel
GQA_SHAPES = tuple((2048, 32, p) for p in (0, 63, 64, 65, 127, 128, 129)) + ((1024, 8, 255), (1024, 8, 256), (4096, 4, 3000), (4096, 3, 2999), (5120, 40, 5000))
GQA_HEADS = ((2, 1, 1), (7, 1, 1), (16, 1, 1), (8, 2, 2))          # (heads, kv heads, batch)


def single_profiles(pos):
    return ALL if pos in (385, 700) else FEW


def decode_launches(kernel, B, nh, nkv, pos, max_seq, n_splits, profiles):
    """-> [(name, Case)]: every launch of one (kernel, shape): each profile once, the spotlight as many rounds as its seams need"""
    chunk = chunk_of(kernel, pos, max_seq, n_splits)
    sk = seams(kernel, pos, chunk)
    out = []
    for prof in profiles:
        rounds = spotlight_rounds(len(sk), B, nh, nkv) if prof == "spotlight" else 1
        for rnd in range(rounds):
            out.append((prof + (f"#{rnd}" if rounds > 1 else ""), decode_case(prof, B, nh, nkv, pos, sk, rnd)))
    return out


# ------------------------------------------------------------------------------------------------------------------ mutations (CPU check)
def head_parts(s, V):
    """s [T] model scores, V [T, 128] -> (w [T], l, O [128]) relative to the maximum"""
    w = np.exp(s - s.max())
    return w, w.sum(), w @ V


P_HELD, P_ALONE = 2e-3, 0.98


def mutants(s, V, t):
    """outputs [128] of one head after each single-key fault at key t: dropped, counted twice, the neighbour read in its place.  A context of ONE
    key has no such fault (its softmax is 1 however often the key is counted), and for the same reason a key that holds more than P_ALONE of the
    mass has no "counted twice": p -> 2 p / (1 + p) moves its output by (1 - p) / (1 + p) < 2^-6 of itself, towards a value fp16 cannot tell from
    it as p -> 1; the tied and spotlight cases hold that key (0 or pos) at a probability where doubling shows"""
    if len(s) == 1:
        return {}
    w, l, O = head_parts(s, V)
    n = t + 1 if t + 1 < len(s) else t - 1
    if w[t] > 0.5 * l:                               # the rest is lost under the key in (l - w_t): taken from the remaining keys directly
        s2, V2, s3 = np.delete(s, t), np.delete(V, t, 0), s.copy()
        s3[t] = s[n]
        V3 = V.copy()
        V3[t] = V[n]
        (w2, l2, O2), (w3, l3, O3) = head_parts(s2, V2), head_parts(s3, V3)
        res = {"dropped": O2 / l2, "neighbour": O3 / l3}
    else:
        res = {"dropped": (O - w[t] * V[t]) / (l - w[t]), "neighbour": (O - w[t] * V[t] + w[n] * V[n]) / (l - w[t] + w[n])}
    if w[t] <= P_ALONE * l:
        res["twice"] = (O + w[t] * V[t]) / (l + w[t])
    return res


def chunk_mutant(s, V, chunk, c):
    """chunk c's (m, l, O) combined with chunk c - 1's m"""
    T = len(s)
    n_act = -(-T // chunk)
    parts = []
    for z in range(n_act):
        sz, Vz = s[z * chunk:(z + 1) * chunk], V[z * chunk:(z + 1) * chunk]
        wz = np.exp(sz - sz.max())
        parts.append((sz.max(), wz.sum(), wz @ Vz))
    M = max(p_[0] for p_ in parts)
    L, O = 0.0, np.zeros(128)
    for z, (m, l, o) in enumerate(parts):
        f = np.exp((parts[z - 1][0] if z == c else m) - M)
        L += l * f
        O = O + o * f
    return O / L
