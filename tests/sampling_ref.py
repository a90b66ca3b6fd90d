"""numpy fp64 restatement of the sampling kernel's rules (amq_amd/csrc/amq_sample.hip, include/amq_hip.h "sampled decoding"): what is kept, what
is drawn, and the generator.  A helper of tests/test_sampling_cpu.py and tests/test_gpu_sampling.py -- not the product, not an oracle of the reference."""
import numpy as np

GRID = ((1.0, 0, 1.0), (0.7, 50, 1.0), (0.8, 0, 0.9), (1.3, 40, 0.95), (0.6, 5, 0.5), (1.0, 1, 1.0), (1.0, 0, 0.3), (0.9, 200, 0.8))
VOCABS = (1000, 32000, 32003, 128256, 152064)
SCALES = (1.0, 3.0, 6.0)


def logits_row(vocab, scale, seed):
    """fp16 normal logits x scale"""
    return (np.random.default_rng(seed).standard_normal(vocab) * scale).astype(np.float16)


def scaled(logits, temperature, suppress=()):
    """z = logit / temperature in fp64; suppressed ids, NaN and -inf -> -inf (no candidates); -0 == +0 as numbers already"""
    z = np.asarray(logits).astype(np.float64)
    z[np.isnan(z)] = -np.inf
    z[np.isposinf(z)] = 65504.0
    for s in suppress:
        if s >= 0:
            z[s] = -np.inf
    return z / float(temperature)


def mass_above(z, kept):
    """per token: the probability mass (softmax over the kept set) of the kept tokens with a STRICTLY larger z"""
    zz = np.where(kept, z, -np.inf)
    p = np.exp(zz - zz.max())
    p /= p.sum()
    vals, inv = np.unique(zz, return_inverse=True)             # ascending
    per_val = np.bincount(inv.reshape(-1), weights=p, minlength=len(vals))
    above = np.concatenate([np.cumsum(per_val[::-1])[::-1][1:], [0.0]])
    return above[inv.reshape(-1)], p


def kept_set(logits, temperature, top_k, top_p, suppress=()):
    """-> (kept mask after top-k and top-p, kept mask after top-k alone, d = mass of strictly larger logits over the top-k set)"""
    z = scaled(logits, temperature, suppress)
    cand = z > -np.inf
    kept_k = cand.copy()
    if 0 < top_k < int(cand.sum()):
        kth = np.sort(z[cand])[-top_k]
        kept_k &= z >= kth                                      # ties with the k-th value are all kept
    d, _ = mass_above(z, kept_k)
    kept = kept_k.copy()
    if top_p < 1.0:
        kept &= d < top_p                                       # the largest has d = 0: always kept
    return kept, kept_k, d


def cdf(logits, temperature, kept, suppress=()):
    """inclusive cumulative distribution over the kept set in ascending token index (fp64)"""
    z = scaled(logits, temperature, suppress)
    zz = np.where(kept, z, -np.inf)
    p = np.exp(zz - zz.max())
    c = np.cumsum(p)
    return c / c[-1], p / p.sum()


def draw(logits, temperature, kept, u, suppress=()):
    """the first token, ascending, whose inclusive cumulative probability exceeds u"""
    c, _ = cdf(logits, temperature, kept, suppress)
    return int(np.searchsorted(c, u, side="right"))


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): counter 4 x uint32, key 2 x uint32 -> 4 x uint32"""
    c = [int(x) & 0xFFFFFFFF for x in counter]
    k = [int(x) & 0xFFFFFFFF for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def uniform(seed, draw_counter, seq):
    """the kernel's u in [0, 1): key = seed, counter = {draw counter (64 bit), sequence index, 0}"""
    w = philox4x32_10([draw_counter & 0xFFFFFFFF, draw_counter >> 32, seq, 0], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    return (w[0] >> 8) * 2.0 ** -24
