"""Reference side of the metadata-domain tests (test_metadomain_cpu.py, test_gpu_metadomain.py): exact numpy restatements of the weight unpacks
the matmul kernels run (amq_common.cuh: the "scaled-subnormal" form, its MODE_FMA / MODE_FMA1 variants, the group-scale first rounding, the
MATH_LINEAR fp32 form), fixture layers whose (scale, zero) cover the fp16 range instead of today's sliver of it, and the set on which -- and the
bound within which -- the scaled-subnormal form equals the reference's two-rounding dequant.  Plain numpy; imports no kernel code.

Every restatement is written from the FORMULA in the header comments, in fp64 with an explicit rounding to fp16 (``rn16``: numpy converts
float64 -> float16 with one round-to-nearest-even, overflow to inf, gradual underflow) wherever the device rounds.  Each fp64 step is exact, so
the only roundings are the stated ones:
  * q 2^E, z 2^E, s 2^-E: a power-of-two scaling of an fp16 value / a small integer -- exact in fp64 (exponents within +-50);
  * q 2^E + zc: q 2^E is a multiple of 2^-9 below 2^4, zc an fp16 value, i.e. a multiple of 2^-24 below 2^16 -- at most 40 significant bits;
  * d sc: two fp16 significands, 22 bits;
  * (q 2^E) sc + c: q 2^E is a multiple of 2^-5 below 2, sc and c are fp16 values: every term a multiple of 2^-29 below 2^17 -- 46 bits;
  * the one-op form's q 2^(SH-24) RN16(s 2^(24-SH)) is q s itself (the multiplier is finite: asserted), a multiple of 2^-24 below 2^20.
"""
import numpy as np

SD_E = {4: -3, 3: -5, 2: -5}         # SdCfg<BITS>::E
GS_E = -9
F16_MAX = 65504.0
CLASSES = ("synthetic", "neg_zero", "zero_above", "int_zero", "int_eps", "tiny_zero", "subnormal_scale", "large_scale", "neg_scale")


def rn16(x):
    """ONE round-to-nearest-even of real (fp64) values to fp16"""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float16)


def _f64(a):
    return np.asarray(a, dtype=np.float16).astype(np.float64)


def expand(meta, group):
    """[N, K / group] per-group values -> [N, K] fp64"""
    return np.repeat(_f64(meta), group, axis=1)


# ------------------------------------------------------------------------------------------------------------------ the unpacks
def hqq_exact(q, scale, zero, bits, group):
    """MODE_HQQ, scaled-subnormal form:  d = RN16(q 2^E + RN16(-z 2^E)),  w = RN16(d RN16(s 2^-E))."""
    e = SD_E[bits]
    q = np.asarray(q, np.float64)
    zc = rn16(-expand(zero, group) * 2.0 ** e).astype(np.float64)
    sc = rn16(expand(scale, group) * 2.0 ** -e).astype(np.float64)
    d = rn16(q * 2.0 ** e + zc).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return rn16(d * sc)


def fma_exact(q, scale, c, bits, group):
    """MODE_FMA, two-op form:  w = RN16(fma(q 2^E, RN16(s 2^-E), c))  (q 2^E exact)."""
    e = SD_E[bits]
    sc = rn16(expand(scale, group) * 2.0 ** -e).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return rn16(np.asarray(q, np.float64) * 2.0 ** e * sc + expand(c, group))


def fma1_shift(bits):
    """the lowest mantissa position a field is brought to in the one-op form (4-bit: 6; 2-, 3-bit: 4): the largest multiplier 2^(24 - SH)"""
    return 6 if bits == 4 else 4


def fma1_exact(q, scale, c, bits, group):
    """MODE_FMA1:  w = RN16(fma(q 2^(SH-24), RN16(s 2^(24-SH)), c)).  Within amq_fma1_scale_bound the multiplier is finite at the lowest field
    position, hence at every one, and a power-of-two scaling that neither overflows nor leaves fp16's exponent range downwards (scaling UP) is
    exact -- so one position stands for all; the multiplier's finiteness is asserted."""
    sh = fma1_shift(bits)
    k = rn16(expand(scale, group) * 2.0 ** (24 - sh)).astype(np.float64)
    assert np.isfinite(k).all(), "a scale beyond amq_fma1_scale_bound: MODE_FMA1 does not apply"
    return rn16(np.asarray(q, np.float64) * 2.0 ** (sh - 24) * k + expand(c, group))


def gs_first(q, zero, group):
    """group-scale first rounding, scaled:  d = RN16(q 2^-9 + RN16(-z 2^-9))  (returned as fp64: d itself, NOT d 2^9)"""
    zc = rn16(-expand(zero, group) * 2.0 ** GS_E).astype(np.float64)
    return rn16(np.asarray(q, np.float64) * 2.0 ** GS_E + zc).astype(np.float64)


def gs_weight(q, scale, zero, group):
    """what a one-hot x row recovers under MATH_GROUPSCALE: the fp32 product (s 2^9) d (22 significant bits: exact) rounded once to fp16"""
    return rn16(gs_first(q, zero, group) * expand(scale, group) * 2.0 ** -GS_E)


def linear_weight(q, scale, zc, group, fma):
    """what a one-hot x row recovers under MATH_LINEAR (amq_gemv_body.cuh): y = RN16(fmaf(s 2^(24-SH), q 2^(SH-24), fmaf(zx, 1, 0))) with
    zx = RN32(-(s z)) (MODE_HQQ) or c (MODE_FMA).  s z has 22 significant bits and stays inside fp32's normal range: zx is exact, and so are the
    power-of-two scalings; the one fp32 rounding is that of the exact s q + zx, then the result is rounded to fp16.  In fp64 s q + zx is exact
    (a multiple of 2^-48 below 2^27)."""
    s = expand(scale, group)
    zx = expand(zc, group) if fma else -(s * expand(zc, group))
    with np.errstate(over="ignore", under="ignore"):
        return (np.asarray(q, np.float64) * s + zx).astype(np.float32).astype(np.float16)


# ------------------------------------------------------------------------------------------------------------------ safe set and bounds
def ulp16(v):
    """spacing of fp16 at |v| (2^-24 through the subnormal range)"""
    a = np.abs(np.asarray(v, np.float64))
    ex = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (ex - 10)


def safe_threshold(bits=None, gs=False):
    """|z| and |q - z| from which z 2^E and (q - z) 2^E are NORMAL halves: 2^(-14 - E)"""
    return 2.0 ** (-14 - (GS_E if gs else SD_E[bits]))


def masks(q, zero, group, thr):
    """-> (safe, z_small, d_small) element masks"""
    z = expand(zero, group)
    z_small = np.abs(z) < thr
    d_small = np.abs(np.asarray(q, np.float64) - z) < thr
    return ~(z_small | d_small), z_small, d_small


def exact_bound(q, scale, zero, w_ref, bits, group):
    """Largest |w - w_ref| the scaled-subnormal MODE_HQQ form may show OUTSIDE the safe set (0 on it), derived from the arithmetic:

    * |q - z| < T = 2^(-14-E)  (whatever |z|): the kernel's d is (q - z) 2^E -- or, where z 2^E was subnormal too, that of a z moved by at most
      2^-25 2^-E -- rounded to a multiple of fp16's subnormal quantum: 2^-25 2^-E off (q - z), twice.  The reference's own first rounding is exact
      there or as good.  Times |s|, plus the two second roundings' half ulps of a weight below T |s| (<= 2^-11 T |s| = 2^-25 2^-E |s| together):
      <= 2^-24 2^-E |s|, the bound the header always gave, with fp16's own quantum 2^-24 as a floor.
    * |z| < T <= |q - z|: zc = RN16(-z 2^E) is a subnormal, so z is taken to a multiple of 2^-24 2^-E first: the kernel rounds q - z' with
      |z' - z| <= 2^-25 2^-E where the reference rounds q - z.  Rounding is monotonic and the shift is far below an ulp of (q - z) >= 2^-9, so
      the two first roundings are equal or NEIGHBOURS: one fp16 ulp of (q - z) apart.  (They do differ: an fp16 z lies on a 2^-20 grid or
      finer, q - z then sits exactly on rounding ties, and a z moved by 2^-20 falls off the tie on the other side.)  Times |s|, plus the second
      roundings' half ulp each of the weight: ulp16(q - z) |s| + ulp16(w)."""
    e = SD_E[bits]
    thr = safe_threshold(bits)
    s = np.abs(expand(scale, group))
    z = expand(zero, group)
    d = np.asarray(q, np.float64) - z
    safe, z_small, d_small = masks(q, zero, group, thr)
    w = np.abs(np.asarray(w_ref, np.float64))
    b = np.zeros(d.shape)
    only_z = z_small & ~d_small
    b[only_z] = (ulp16(d) * s + ulp16(w + ulp16(d) * s))[only_z]
    b[d_small] = np.maximum(2.0 ** -24 * 2.0 ** -e * s, 2.0 ** -24)[d_small]
    return b


def first_rounding_bound(q, zero, bits, group):
    """the same statement about d alone, in units of (q - z): 0 on the safe set, 2^-24 2^-E where |q - z| < T, one fp16 ulp of (q - z) where only |z| is"""
    e = SD_E[bits]
    safe, z_small, d_small = masks(q, zero, group, safe_threshold(bits))
    d = np.asarray(q, np.float64) - expand(zero, group)
    b = np.zeros(d.shape)
    b[z_small & ~d_small] = ulp16(d)[z_small & ~d_small]
    b[d_small] = 2.0 ** -24 * 2.0 ** -e
    return b


def gs_bound(q, scale, zero, group):
    """group-scale weights outside ITS safe set (|z|, |q - z| >= 2^-5): (2^-9 |q - z| + 2^-15) |s|, floor 2^-24 (amq_common.cuh, unchanged)"""
    d = np.abs(np.asarray(q, np.float64) - expand(zero, group))
    return np.maximum((2.0 ** -9 * d + 2.0 ** -15) * np.abs(expand(scale, group)), 2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------------ fixtures
def fma1_bound16(bits):
    """(the fp16 value at or just below amq_fma1_scale_bound(bits) = 65504 / 2^(24 - SH), the next fp16 value above it)"""
    bound = F16_MAX / 2.0 ** (24 - fma1_shift(bits))
    at = np.float16(bound)
    if float(at) > bound:
        at = np.nextafter(at, np.float16(0))
    return at, np.nextafter(at, np.float16(np.inf))


def payload(bits, n, k):
    """codes q[n, k]: over the rows every code value at every one of the 128 positions of a group (7 is odd: n -> 7 n mod 2^b is onto), and
    neighbouring positions, pairs and dwords of a lane differ"""
    nn, kk = np.meshgrid(np.arange(n), np.arange(k), indexing="ij")
    return ((7 * nn + 5 * kk + (kk >> 4) + (kk >> 7)) % (2 ** bits)).astype(np.int32)


def class_map(n, k, group):
    nn, gg = np.meshgrid(np.arange(n), np.arange(k // group), indexing="ij")
    return (nn + gg) % len(CLASSES)


def make_layer(bits, group, n, k, seed=0, fma1=False):
    """One fixture layer: dict(q [n, k] int32, scale / zero [n, k / group] fp16, cls [n, k / group] class index, and for the one-rounding modes
    c = -RN16(z s) [n, k / group] fp16 -- the reference's scale_zeros, negated as the native meta holds it).  Class of (row, group) =
    (row + group index) mod 9: every 16-row tile and every tile row mixes classes.  All values fp16, all weights finite in every arithmetic.
    ``fma1``: the large scales stop at amq_fma1_scale_bound (the layer is one that MODE_FMA1 serves) instead of at the unpack's own limit."""
    rng = np.random.default_rng(1000 * bits + group + seed)
    maxq = 2 ** bits - 1
    cls = class_map(n, k, group)
    shape = cls.shape
    s_syn = 2.7e-3 * rng.uniform(0.5, 1.5, shape) * 16.0 / 2 ** bits
    z_syn = rng.uniform(0.0, maxq, shape)
    s, z = s_syn.copy(), z_syn.copy()

    def put(name, arr, val):
        m = cls == CLASSES.index(name)
        arr[m] = val[m]
        return m
    put("neg_zero", z, -rng.uniform(0.0, 40.0, shape))
    put("zero_above", z, rng.uniform(maxq, 300.0, shape))
    zi = rng.integers(0, maxq + 1, shape).astype(np.float64)
    m = put("int_zero", z, zi)
    put("int_eps", z, rng.integers(0, maxq + 1, shape) + rng.choice([3e-4, -3e-4, 1e-3, 0.01], shape))
    # |z| <= 0.03 -- half of them drawn, half placed where the unpack's treatment of a small z shows: below T = 2^(-14-E) the kernel takes z to a
    # multiple of g = 2^-24 2^-E, so z = t +- g / 2 with t a rounding tie of some q - z (t = k 2^-12: ties of 1 - z, 2 - z, 3 - z, 4 - z) goes
    # to t itself, and q - t is then rounded to even where the reference rounds q - z to the nearer side
    g = 2.0 ** (-24 - SD_E[bits])
    ties = np.array([k * 2.0 ** -12 for k in range(1, 8)] if SD_E[bits] == -5 else [2.0 ** -12])
    placed = rng.choice([-1.0, 1.0], shape) * (rng.choice(ties, shape) + rng.choice([-0.5, 0.5], shape) * g)
    put("tiny_zero", z, np.where(rng.random(shape) < 0.5, placed, rng.uniform(-0.03, 0.03, shape)))
    put("subnormal_scale", s, 2.0 ** rng.uniform(-24.0, -14.0, shape))
    put("neg_scale", s, -s_syn)
    z16 = rn16(z)
    idx = np.argwhere(m)                                   # +0 and -0 both present among the integer zero points
    z16[tuple(idx[0])] = np.float16(0.0)
    z16[tuple(idx[1])] = np.float16(-0.0)
    # large scales: up to 0.99 of the largest |s| at which s 2^-E and every weight of the group are finite
    zz = z16.astype(np.float64)
    dmax = np.maximum(np.abs(rn16(0.0 - zz).astype(np.float64)), np.abs(rn16(maxq - zz).astype(np.float64)))
    smax = np.minimum(float(fma1_bound16(bits)[0]) / 0.99 if fma1 else F16_MAX * 2.0 ** SD_E[bits], F16_MAX / np.maximum(dmax, 1e-3))
    big = smax * rng.uniform(0.5, 0.99, shape)
    mb = cls == CLASSES.index("large_scale")
    ib = np.argwhere(mb)
    big[tuple(ib[0])] = 0.99 * smax[tuple(ib[0])]
    s[mb] = big[mb]
    s16 = rn16(s)
    c16 = rn16(-(z16.astype(np.float64) * s16.astype(np.float64)))
    assert np.isfinite(s16.astype(np.float64)).all() and np.isfinite(c16.astype(np.float64)).all()
    return dict(bits=bits, group=group, n=n, k=k, q=payload(bits, n, k), scale=s16, zero=z16, c=c16, cls=cls)


def make_boundary_layer(bits, n, k, above, seed=0):
    """MODE_FMA only (groups of 128): today's synthetic draw with ONE scale raised to the fp16 value at amq_fma1_scale_bound (``above`` False:
    the layer must select MODE_FMA1) or to the next fp16 value (True: it must keep MODE_FMA)"""
    rng = np.random.default_rng(77 * bits + seed + (1 if above else 0))
    maxq = 2 ** bits - 1
    shape = (n, k // 128)
    s16 = rn16(2.7e-3 * rng.uniform(0.5, 1.5, shape) * 16.0 / 2 ** bits)
    z16 = rn16(rng.uniform(0.0, maxq, shape))
    at, nxt = fma1_bound16(bits)
    s16[n // 2 + 1, (k // 128) // 2] = nxt if above else at
    c16 = rn16(-(z16.astype(np.float64) * s16.astype(np.float64)))
    return dict(bits=bits, group=128, n=n, k=k, q=payload(bits, n, k), scale=s16, zero=z16, c=c16, cls=np.zeros(shape, np.int64))


def hqq_buffers(layer):
    """-> (W_q, scale [R, 1], zero [R, 1]) in the reference's HQQ format (oracle.hqq_ref.pack)"""
    from oracle import hqq_ref
    return hqq_ref.pack(layer["q"], layer["bits"], layer["group"]), layer["scale"].reshape(-1, 1), layer["zero"].reshape(-1, 1)


def gptq_buffers(layer):
    """-> (qweight int32, scales fp32 [K / G, N], zeros fp32 [K / G, N] = -c) in the reference's GPTQ format (oracle.gptq_ref.pack_qweight)"""
    from oracle import gptq_ref
    return (gptq_ref.pack_qweight(layer["q"], layer["bits"]), np.ascontiguousarray(layer["scale"].T).astype(np.float32),
            np.ascontiguousarray((-layer["c"]).T).astype(np.float32))


def class_names(layer):
    """[N, K] class name index per element"""
    return np.repeat(layer["cls"], layer["group"], axis=1)
