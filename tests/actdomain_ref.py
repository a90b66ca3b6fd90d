"""Reference side of the activation-domain tests (test_actdomain_cpu.py, test_gpu_actdomain.py): fp64 restatements, with every rounding explicit,
of the transforms the kernels fuse around a matmul -- the RMSNorm prologues, SiLU*mul, the bias / act / residual / gate epilogue -- the fixture
rows of x they are judged on, and the "selection" layers (one code 1 per weight row, scale 1, zero 0) through which a matmul kernel reads its
staged activation back without a rounding of its own.  Plain numpy; imports no kernel code.

The arithmetic (amq_gemv_body.cuh stage_x / x_finish / x_finish_dma, amq_decode.hip rmsnorm_kernel, amq_gemm.hip splitk_reduce_norm_kernel):

  RMSNorm      nrm = RN16(RN32(x * rstd)),  y = RN16(gamma * nrm)            rstd = rsqrtf(sum(x^2) / K + eps) in fp32
  SiLU * mul   s   = RN16(g / (1 + __expf(-g))) in fp32,  y = RN16(s * up)
  epilogue     v = RN16(acc);  v = RN16(v + bias);  v = RN16(silu(v)) [act];  v = RN16(residual + v);  gated: y = RN16(RN16(silu(gate)) * v)

gamma * nrm and s * up are products of two halves: exact in fp32 (22 bits), so each has ONE rounding.  The first rounding of RMSNorm and of SiLU
is that of an fp32 value which is not the fp64 one: with t the fp64 value the kernel's fp32 value is t (1 + d), |d| <= EPS, and -- rounding being
monotonic -- the staged half is RN16(t (1 - EPS)) or RN16(t (1 + EPS)): the two ends of the BAND (equal at all but a few per cent of elements:
2 EPS is 2^-5 of an fp16 ulp; those few are "ambiguous").  The epilogue's adds are fp16 adds of fp16 values: exact, no band.

EPS, derived (u = 2^-24, fp32's unit roundoff; first order in u):

  RMSNorm.  x^2 is exact in fp32 (22 bits).  A sum of positive fp32 terms along a chain of D additions carries at most D u relative error.  D per
  staging path is the lane's serial adds, then the wave tree (4 DPP steps + 2 adds of the readlane form, or 6 shuffle steps), then the waves:
     x_finish          4 / 8 / 16 waves, 1 / 2 / 4 chunks of 8 per thread:   8 XCH + 6 + NW   <= 32 + 6 + 16 = 54   (K = 28672)
     x_finish_dma      as x_finish (8 XCH + 6 + NW)                                            <= 16 + 6 + 16 = 38
     stage_x           rows side by side, WPR = NW / M waves per row: K / (8 . 64 WPR) chunks per lane: 16 rows of K = 8192 on 16 waves,
                       WPR = 1: 16 chunks x 8 = 128 serial adds, + 6 + (WPR - 1)               <= 134                (the longest)
     stage_x (linear)  K / (8 . 64 NW) chunks per lane x 8 + 6 + NW                            <= 54
     partial sums      16 squares per partial (an MFMA tile row: <= 16), 8 partials per lane, + 6                    <= 30
     rmsnorm_kernel, splitk_reduce_norm_kernel  (256 threads) K / 2048 chunks x 8 + 6 + 4      <= 42 at K = 8192
     gemv_f16w         as rmsnorm_kernel
  rstd = rsqrtf(tot / K + eps): the square root halves the relative error of its argument, so D u / 2 from the sum, (u + u) / 2 from the
  division (or the exact multiply by 2^-log2 K) and the eps add; rsqrtf (v_rsq_f32: 1 ulp) 2 u; the product x * rstd u.
     D = 134:   (67 + 1 + 2 + 1) u = 71 u  <  128 u = 2^-17 = RMS_EPS, which covers every path up to K = 8192 rows and the one-row forms to 28672.

  SiLU.  silu_f(g) = g / (1 + __expf(-g)); __expf(a) = v_exp_f32(a * log2(e)).  a * log2(e): the fp32 constant is 2^-26 off, the product rounds: the
  argument is (1.25 u) relative off, which is |g| (1.25 u) relative in the exponential; v_exp_f32 1 ulp = 2 u; the add u; the division (correctly
  rounded) u.  The exponential's error reaches silu scaled by e^-g / (1 + e^-g) <= 1.  Beyond |g| = 88.7 the exponential is 0 or inf and silu is
  g or -0, exactly what the fp64 expression rounds to.  So (1.25 x 88.7 + 2 + 1 + 1) u = 115 u < 128 u = 2^-17 = SILU_EPS  (the cap the design
  allows: 2^-16).
"""
import numpy as np

from metadomain_ref import rn16

RMS_EPS = 2.0 ** -17
SILU_EPS = 2.0 ** -17
D_LONGEST = 134                     # stage_x, 16 rows of K = 8192 (see above)
RMS_AMBIGUOUS_CAP = 0.04            # per row
SILU_AMBIGUOUS_CAP = 0.035          # over all finite gates
X_CLASSES = ("gauss3", "massive", "massive_tiny", "zero", "one_hot", "subnormal_grid", "const", "gauss_small")
NORM_EPS = 1e-5


def f64(a):
    return np.asarray(a, np.float16).astype(np.float64)


def same16(a, b):
    """fp16 arrays equal bit for bit, +0 and -0 taken as equal (a sum of zeros loses the sign)"""
    a, b = np.asarray(a, np.float16), np.asarray(b, np.float16)
    return (a.view(np.uint16) == b.view(np.uint16)) | ((a == 0) & (b == 0))


class Band:
    """lo / hi: the output with the first rounding taken at either end of the band; mid: with RN16 of the fp64 value; amb: lo != hi"""

    def __init__(self, lo, hi, mid):
        self.lo, self.hi, self.mid = (np.asarray(v, np.float16) for v in (lo, hi, mid))
        self.amb = ~same16(self.lo, self.hi)
        for v in (self.lo, self.hi, self.mid):
            assert np.isfinite(v.astype(np.float64)).all(), "a restated activation is not finite: 0 * inf would pollute a selection read-out"

    def accepts(self, y):
        return same16(y, self.lo) | same16(y, self.hi)

    def take(self, idx):
        return Band(self.lo[idx], self.hi[idx], self.mid[idx])


def _ends(t, eps):
    with np.errstate(over="ignore", under="ignore"):
        return rn16(t * (1.0 - eps)).astype(np.float64), rn16(t * (1.0 + eps)).astype(np.float64), rn16(t).astype(np.float64)


def rms_t(x16, eps=NORM_EPS, drop=None):
    """t = x rsqrt(mean(x^2) + float32(eps)) in fp64 from the fp16 values; ``drop``: a column mask left OUT of the sum (a mutant's statistic)"""
    x = f64(x16)
    sq = x * x
    if drop is not None:
        sq = np.where(drop, 0.0, sq)
    return x / np.sqrt(sq.sum(axis=-1, keepdims=True) / x.shape[-1] + float(np.float32(eps)))


def rmsnorm_band(x16, gamma16, eps=NORM_EPS, rel=RMS_EPS):
    """RN16(gamma * nrm) with nrm = RN16(t (1 -+ rel)) -- a Band over x's shape"""
    g = f64(gamma16)
    return Band(*(rn16(g * n) for n in _ends(rms_t(x16, eps), rel)))


def silu64(g16):
    g = f64(g16)
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


def silu_band(g16, up16=None, rel=SILU_EPS):
    """RN16(RN16(silu(g) (1 -+ rel)) * up)  (up None: fp16(silu(g)) itself)"""
    ends = _ends(silu64(g16), rel)
    if up16 is None:
        return Band(*(rn16(s) for s in ends))
    u = f64(up16)
    return Band(*(rn16(s * u) for s in ends))


def epilogue(acc, bias=None, residual=None, act=False, gate=None):
    """the documented order on fp64 ``acc`` [M, N] -> Band (lo == hi unless ``act`` / ``gate`` bring SiLU's first rounding in).
    inf is a legitimate result here (an fp16 add that overflows), so this Band is built without the finiteness assertion."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = rn16(acc).astype(np.float64)
        if bias is not None:
            v = rn16(v + f64(bias)).astype(np.float64)
        vs = (v, v, v)
        if act:
            vs = _ends(np.where(np.isfinite(v), v / (1.0 + np.exp(-np.where(np.isfinite(v), v, 0.0))), v), SILU_EPS)
        if residual is not None:
            vs = tuple(rn16(f64(residual) + w).astype(np.float64) for w in vs)
        if gate is not None:
            gs = _ends(silu64(gate), SILU_EPS)
            vs = tuple(rn16(s * w).astype(np.float64) for s, w in zip(gs, vs))
    b = Band.__new__(Band)
    b.lo, b.hi, b.mid = (rn16(w) for w in vs)
    b.amb = ~same16(b.lo, b.hi)
    return b


# ------------------------------------------------------------------------------------------------------------------ mutants (CPU sensitivity)
def mutant_rms_single_rounding(x16, gamma16, eps=NORM_EPS):
    """RN16(gamma * x * rstd): the intermediate rounding of LlamaRMSNorm forgotten"""
    return rn16(f64(gamma16) * rms_t(x16, eps))


def mutant_rms_lost_share(x16, gamma16, eps=NORM_EPS):
    """a sum of squares that lost every eighth 8-column chunk (one wave's share of eight)"""
    k = np.asarray(x16).shape[-1]
    drop = (np.arange(k) // 8) % 8 == 7
    return rn16(f64(gamma16) * rn16(rms_t(x16, eps, drop=drop)).astype(np.float64))


def mutant_silu_sigmoid_rounded(g16):
    """g * fp16(sigmoid(g)): the other order of SiLU's two operations"""
    g = f64(g16)
    with np.errstate(over="ignore"):
        return rn16(g * rn16(1.0 / (1.0 + np.exp(-g))).astype(np.float64))


def mutant_epilogue_single_rounding(acc, bias, residual):
    """bias and residual folded into ONE rounding of the fp32 accumulator"""
    with np.errstate(over="ignore"):
        return rn16(np.asarray(acc, np.float64) + f64(bias) + f64(residual))


# ------------------------------------------------------------------------------------------------------------------ fixtures
def x_row(cls, k, seed=0):
    """one fixture row of x [k] fp16 of class ``cls`` (an index into X_CLASSES)"""
    rng = np.random.default_rng(7919 * cls + 13 * k + seed)
    name = X_CLASSES[cls]
    if name == "gauss3":
        v = 3.0 * rng.standard_normal(k)
    elif name == "massive":                     # a Llama residual stream: a few channels in the thousands beside a bulk near 1
        v = rng.standard_normal(k)
        v[3], v[k - 2], v[k // 2 + 1] = 60000.0, -2500.0, 900.0        # first chunk, last chunk, middle
    elif name == "massive_tiny":                # nearly every normalised value is an fp16 subnormal
        v = 0.01 * rng.standard_normal(k)
        v[k // 3] = 65504.0
    elif name == "zero":
        v = np.zeros(k)
    elif name == "one_hot":
        v = np.zeros(k)
        v[(5 * k) // 8 + 1] = -3.0
    elif name == "subnormal_grid":              # subnormal inputs: sum of squares far below eps
        v = rng.integers(-1023, 1024, k) * 2.0 ** -24
    elif name == "const":
        v = np.full(k, 0.7)
    else:
        v = 1e-3 * rng.standard_normal(k)       # mean(x^2) ~ 1e-6: eps matters
    return rn16(v)


def capped_row(cls, k, seed=0):
    """x_row, redrawn (seed + 997, ...) while the band would leave more of the row open than RMS_AMBIGUOUS_CAP: a condition on the INPUT, decided by
    the restatement alone.  (The expected share is 2 RMS_EPS / (an fp16 ulp, relative) = 1.6 .. 3.1 %; a row whose rstd makes x * rstd cluster
    next to ties -- a few per cent of Gaussian draws do -- is passed over, no kernel result is consulted.)"""
    for attempt in range(16):
        x = x_row(cls, k, seed + 997 * attempt)
        if rmsnorm_band(x[None], gamma_vec(k)).amb.mean() <= RMS_AMBIGUOUS_CAP:
            return x
    raise AssertionError(f"no row of class {X_CLASSES[cls]} at K = {k} within the cap")


def launches(rows, k, seed=0):
    """[L][rows, k] fp16 + [L][rows] class index: slot t = launch * rows + row holds class t mod 8 (rows a multiple of 8: shifted by the launch index),
    so every class appears in every case and every row slot meets several classes"""
    n_launch = max(3 if rows > 1 else 8, -(-len(X_CLASSES) // rows))
    xs, cs = [], []
    for j in range(n_launch):
        cl = [(j * rows + i + (j if rows % 8 == 0 else 0)) % len(X_CLASSES) for i in range(rows)]
        xs.append(np.stack([capped_row(c, k, seed + 31 * j + i) for i, c in enumerate(cl)]))
        cs.append(np.asarray(cl))
    return xs, cs


def gamma_vec(k, seed=0):
    """1 + 0.1 randn in fp16; every 7th entry negated, every 11th an exact power of two"""
    rng = np.random.default_rng(4001 + k + seed)
    g = 1.0 + 0.1 * rng.standard_normal(k)
    idx = np.arange(k)
    g[idx % 7 == 3] *= -1.0
    p2 = idx % 11 == 5
    g[p2] = (2.0 ** rng.integers(-2, 2, k) * rng.choice([-1.0, 1.0], k))[p2]
    return rn16(g)


def up_rows(rows, k, seed=0, gate=None):
    """Gaussian second operands; under a ``gate`` whose product with them would leave fp16's range (the massive channels) they are +-0.5:
    staged values must stay finite"""
    up = rn16(np.random.default_rng(911 + 17 * rows + k + seed).standard_normal((rows, k)))
    if gate is not None:
        big = np.abs(silu64(gate) * f64(up)) > 60000.0
        up[big] = (np.sign(up[big]) * np.float16(0.5)).astype(np.float16)
    return up


def all_finite_halves():
    """every finite fp16 value: 63488 of them (both zeros included)"""
    v = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    v = v[np.isfinite(v.astype(np.float32))]
    assert v.size == 63488
    return v


def gate_rows(k):
    """all finite gates as rows of k (the last row padded with zeros) -> [R, k] fp16"""
    v = all_finite_halves()
    r = -(-v.size // k)
    out = np.zeros(r * k, np.float16)
    out[:v.size] = v
    return out.reshape(r, k)


# ------------------------------------------------------------------------------------------------------------------ selection layers
def selection_cols(n, k):
    """the column weight row i selects: i itself where n == k; else n columns spread over K that touch every 8-column chunk where n >= k / 8:
    i (k / n) + i mod (k / n)"""
    if n == k:
        return np.arange(k)
    assert k % n == 0
    step = k // n
    i = np.arange(n)
    return i * step + i % step


def selection_codes(n, k, cols, second=None):
    """codes q [n, k] uint8: 1 at (i, cols[i]) (and at (i, second[i])), else 0"""
    q = np.zeros((n, k), np.uint8)
    q[np.arange(n), cols] = 1
    if second is not None:
        q[np.arange(n), second] = 1
    return q


def hqq_selection(q, bits, group):
    """-> (W_q, scale, zero) in the reference's HQQ format: scale 1, zero 0 -- the weights are the codes, exactly, at 2, 3 and 4 bit"""
    from oracle import hqq_ref
    r = q.size // group
    return hqq_ref.pack(q if bits != 3 else q.astype(np.int32), bits, group), np.ones(r, np.float16), np.zeros(r, np.float16)


def gptq_selection(q, bits, group):
    from oracle import gptq_ref
    n, k = q.shape
    return gptq_ref.pack_qweight(q.astype(np.int32), bits), np.ones((k // group, n), np.float32), np.zeros((k // group, n), np.float32)


# ------------------------------------------------------------------------------------------------------------------ epilogue fixtures
def epilogue_case(m, n, seed=0):
    """Two-hot layer inputs for the epilogue probes: acc[m, j] = xa[m, j] + xb[m, j] exactly in fp32 (xa in [1, 2), xb a multiple of 2^-16 in
    [2^-9, 2^-8): 17 significant bits), NOT an fp16 value, so all three roundings show: RN16(acc), RN16(v + bias) and RN16(residual + v).
      * bias[j]: odd columns an odd multiple of 2^-11 (v + bias sits ON a tie of [1, 2)'s 2^-10 grid: round-to-even decides), even columns a
        multiple of 2^-16 in [2^-6, 2^-5), every eighth column +-(16 .. 64);
      * residual[m, j] in [1, 2) chosen from v1 = RN16(RN16(acc) + bias) so that residual + v1 is an odd multiple of 2^-10 in [2, 4): ON a tie of
        the 2^-9 grid.  The staged arithmetic rounds it to even; a single rounding of acc + bias + residual goes where the dropped bits point.
      * row 0, in the columns of the large biases: xa = 65504, xb = 0: the bias add overflows to inf where the bias is >= 16 (and residual + inf
        stays inf).
    -> dict(xa, xb, bias, residual [fp16], acc [fp64])"""
    rng = np.random.default_rng(5000 + 7 * m + n + seed)
    xa = rn16(1.0 + rng.integers(0, 1024, (m, n)) * 2.0 ** -10)
    xb = rn16(2.0 ** -9 + rng.integers(0, 128, (m, n)) * 2.0 ** -16)
    j = np.arange(n)
    xa[0, j % 8 == 6], xb[0, j % 8 == 6] = np.float16(65504.0), np.float16(0.0)
    bias = np.where(j % 2 == 1, (2 * rng.integers(16, 32, n) + 1) * 2.0 ** -11, 2.0 ** -6 + rng.integers(0, 1024, n) * 2.0 ** -16)
    big = j % 8 == 6
    bias[big] = (rng.integers(16, 65, n) * rng.choice([-1.0, 1.0], n))[big]
    bias = rn16(bias)
    acc = f64(xa) + f64(xb)
    with np.errstate(over="ignore"):
        v1 = rn16(rn16(acc).astype(np.float64) + f64(bias)).astype(np.float64)
    r0 = 1.0 + rng.integers(0, 900, (m, n)) * 2.0 ** -10
    tie = (np.floor((r0 + np.where(np.isfinite(v1), v1, 0.0)) * 2.0 ** 9) + 0.5) * 2.0 ** -9      # an odd multiple of 2^-10
    res = tie - np.where(np.isfinite(v1), v1, 0.0)
    ok = np.isfinite(v1) & (v1 >= 1.0) & (v1 < 2.1) & (res >= 1.0) & (res < 2.0) & (tie < 4.0)
    res = rn16(np.where(ok, res, r0))
    return dict(xa=xa, xb=xb, bias=bias, residual=res, acc=acc)
