"""Reference statements for the per-head q / k RMSNorm in front of the rotation (Qwen3), in torch on the CPU, and the summation tree every
rotating kernel forms its statistic with.

``norm_rope_f16``: HF's arithmetic for one head -- Qwen3RMSNorm (fp32 statistic, one fp16 rounding of x * rstd, fp16 multiply by the weight) and
apply_rotary_pos_emb (fp16 t * cos + rotate_half(t) * sin).  ``norm_rope_f64``: the same function in fp64 end to end.  The test module pins the
first to transformers' own modules; neither runs any code of the package.
"""
import torch


def table_cos_sin(row):
    """a row of the runner's cos/sin table ([64][2] = 128 fp16 values: (cos_i, sin_i) pairs) as the (cos, sin) [128] the references take"""
    cs = row.detach().cpu().view(64, 2)
    return torch.cat([cs[:, 0], cs[:, 0]]), torch.cat([cs[:, 1], cs[:, 1]])


def _rotate_half(t):
    return torch.cat([-t[..., 64:], t[..., :64]], -1)


def norm_rope_f16(x, gamma, eps, cos, sin):
    """x [..., 128] fp16, gamma [128] fp16, cos / sin [128] fp16 -> fp16, with fp16 operations where HF has them"""
    x, gamma = x.detach().cpu(), gamma.detach().cpu()
    xf = x.to(torch.float32)
    var = xf.pow(2).mean(-1, keepdim=True)
    y = gamma * (xf * torch.rsqrt(var + eps)).to(torch.float16)          # Qwen3RMSNorm.forward: weight * hidden_states.to(input_dtype)
    return y * cos + _rotate_half(y) * sin                               # apply_rotary_pos_emb


def norm_rope_f64(x, gamma, eps, cos, sin):
    """the same function in fp64 end to end (the fp16 inputs, weights and cos / sin values are exact in fp64)"""
    x, gamma, cos, sin = (t.detach().cpu().to(torch.float64) for t in (x, gamma, cos, sin))
    y = gamma * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
    return y * cos + _rotate_half(y) * sin


def rope_f64(x, cos, sin):
    x, cos, sin = (t.detach().cpu().to(torch.float64) for t in (x, cos, sin))
    return x * cos + _rotate_half(x) * sin


def attention_f64(q, K, V):
    """q [nh, 128], K / V [nh, T, 128] fp64 -> softmax(q K^T / sqrt(128)) V, [nh, 128]"""
    w = torch.einsum("hd,htd->ht", q, K) * (128 ** -0.5)
    return torch.einsum("ht,htd->hd", torch.softmax(w, -1), V)


# ---- the summation tree: 64 pair sums p_i = x_i^2 + x_(i+64)^2, added level by level over index bit 0, 1, .. 5 -------------------------------
class Tree:
    """records, per level, which operands are added; a node is the frozenset of the pair indices under it"""

    def __init__(self):
        self.levels = [set() for _ in range(6)]

    def add(self, level, a, b):
        self.levels[level].add(frozenset((a, b)))
        return a | b


def leaves():
    return [frozenset((i,)) for i in range(64)]


def tree_statement():
    """the definition: level j adds the two nodes whose index sets differ in bit j only"""
    t = Tree()
    nodes = {i: n for i, n in enumerate(leaves())}
    for level in range(6):
        nxt = {}
        for i, n in nodes.items():
            if not (i >> level) & 1:
                nxt[i] = t.add(level, n, nodes[i | (1 << level)])
        nodes = nxt
    assert list(nodes) == [0] and nodes[0] == frozenset(range(64))
    return t


def tree_wave64():
    """64 lanes x 1 pair (the per-head decode kernels' wave 0): an all-reduce butterfly, lane l adds lane l ^ 2^j at level j"""
    t = Tree()
    v = leaves()
    for level in range(6):
        v = [t.add(level, v[l], v[l ^ (1 << level)]) for l in range(64)]
    assert all(n == frozenset(range(64)) for n in v)
    return t


def _in_thread8(t, p):
    """levels 0 .. 2 over the eight pairs a thread holds: ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))"""
    a = [t.add(0, p[2 * i], p[2 * i + 1]) for i in range(4)]
    b = [t.add(1, a[0], a[1]), t.add(1, a[2], a[3])]
    return t.add(2, b[0], b[1])


def tree_threads8():
    """8 threads x 8 pairs (the prompt kernels): thread c holds pairs 8c .. 8c + 7; levels 3 .. 5 across the eight neighbouring lanes"""
    t = Tree()
    lf = leaves()
    v = [_in_thread8(t, lf[8 * c:8 * c + 8]) for c in range(8)]
    for j in range(3):
        v = [t.add(3 + j, v[c], v[c ^ (1 << j)]) for c in range(8)]
    assert all(n == frozenset(range(64)) for n in v)
    return t


def tree_fragments():
    """4 lanes x 16 pairs in MFMA fragment order (the grouped-query kernel's queries): lane o holds pairs 32 t + 8 o + e, t = 0 / 1, e = 0 .. 7;
    levels 0 .. 2 over e in the lane, 3 .. 4 over o across the lanes (for each t), level 5 over t in the lane"""
    t = Tree()
    lf = leaves()
    s = [[_in_thread8(t, [lf[32 * tt + 8 * o + e] for e in range(8)]) for o in range(4)] for tt in range(2)]
    for j in range(2):
        s = [[t.add(3 + j, s[tt][o], s[tt][o ^ (1 << j)]) for o in range(4)] for tt in range(2)]
    v = [t.add(5, s[0][o], s[1][o]) for o in range(4)]
    assert all(n == frozenset(range(64)) for n in v)
    return t
