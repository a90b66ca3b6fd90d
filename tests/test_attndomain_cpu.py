"""CPU: the reference side of the attention-domain tests (tests/attndomain_ref.py) checked without a GPU -- it agrees with plain float64 attention and
with HF's fp16-score eager expression; every case the GPU module launches meets the exactness preconditions and its profile's conditions; and the
MUTATION CHECK: for every case and every key the case holds, a reference with that key dropped, counted twice or replaced by its neighbour, with a
chunk combined under the previous chunk's maximum, or with the causal mask moved by one, leaves the derived bound by a factor >= 4 at some output
element -- the proof that the GPU tests fail on a subtly wrong kernel, obtained without running one.  The tightness cap keeps the bound from
swallowing a launch: at most 1 % of the elements with |ref| >= 2^-10 may carry a bound above 2^-8 |ref|."""
import functools

import numpy as np
import pytest
import torch

import attndomain_ref as ref

FACTOR = 4.0
SHAPES = ([("single", (1, nh, nkv, 1024, 1, pos)) for nh, nkv in ref.SINGLE_HEADS for pos in ref.SINGLE_POS] + [("single", (2, 4, 1, 1024, 1, 385))]
          + [("split", (1, 2, 2, ms, ns, pos)) for ms, ns, pos in ref.SPLIT_SHAPES]
          + [("gqa", (B, nh, nkv, ms, ns, pos)) for nh, nkv, B in ref.GQA_HEADS for ms, ns, pos in ref.GQA_SHAPES])
PREFILL = ([(1, nh, nkv, S, 0) for nh, nkv in ((2, 2), (4, 1)) for S in (1, 15, 16, 17, 63, 64, 65, 128, 129, 200)]
           + [(1, nh, nkv, S, p0) for nh, nkv in ((2, 2), (4, 1)) for S in (5, 64) for p0 in (11, 64, 100)] + [(2, 2, 2, 65, 0), (2, 4, 1, 65, 0)])
SEAM_ROWS = (0, 1, 15, 16, 17, 31, 32, 63, 64, 65, 127, 128, 129)


def _id(v):
    return v[0] + "-" + "x".join(str(i) for i in v[1]) if isinstance(v[0], str) else "x".join(str(i) for i in v)


def test_reference_is_plain_float64_attention():
    g = torch.Generator().manual_seed(3)
    B, nh, nkv, T = 2, 4, 2, 77
    q = torch.randn(B, nh, 128, generator=g, dtype=torch.float64)
    K = torch.randn(B, nkv, T, 128, generator=g).half()
    V = torch.randn(B, nkv, T, 128, generator=g).half()
    s = torch.einsum("bhd,bhtd->bht", q, K.double().repeat_interleave(2, 1)) * 128 ** -0.5
    want = torch.einsum("bht,bhtd->bhd", torch.softmax(s, -1), V.double().repeat_interleave(2, 1))
    got = ref.reference(s.numpy(), V.numpy())
    assert np.abs(got.ref - want.numpy()).max() < 1e-13 and np.abs(got.p.sum(-1) - 1).max() < 1e-13
    # causal, several rows
    S = 9
    q4 = torch.randn(B, nh, S, 128, generator=g, dtype=torch.float64)
    s4 = torch.einsum("bhsd,bhtd->bhst", q4, K.double().repeat_interleave(2, 1)[:, :, :S + 3]) * 128 ** -0.5
    mask = ref.causal_mask(S, 3)
    want4 = torch.softmax(s4.masked_fill(~torch.from_numpy(mask), float("-inf")), -1) @ V.double().repeat_interleave(2, 1)[:, :, :S + 3]
    got4 = ref.reference(s4.numpy(), V.numpy()[:, :, :S + 3], np.broadcast_to(mask, s4.shape), kernel="prefill")
    assert np.abs(got4.ref - want4.numpy()).max() < 1e-13
    assert (got4.p[..., ~mask] == 0).all()


def test_eager_model_is_hf_fp16_score_expression():
    """HF eager: matmul(q, k^T) in fp16, * scaling in fp16, softmax in fp32, probabilities to fp16, matmul with v -- on randn inputs the eager
    score rounding reproduces the fp16 scores bit for bit and the reference holds HF's output inside the single-workgroup kernel's bound"""
    g = torch.Generator().manual_seed(4)
    nh, T = 4, 300
    q = torch.randn(1, nh, 1, 128, generator=g).half()
    K = torch.randn(1, nh, T, 128, generator=g).half()
    V = torch.randn(1, nh, T, 128, generator=g).half()
    raw16 = (q.float() @ K.float().transpose(2, 3)).half()
    s16 = raw16 * (128 ** -0.5)
    mine = ref.eager_round(raw16.numpy())
    assert np.array_equal(mine, s16.double().numpy())
    p16 = torch.softmax(s16, -1, dtype=torch.float32).half()
    hf = (p16.float() @ V.float()).half()[0, :, 0]
    got = ref.reference(mine[:, :, 0], V.numpy(), kernel="single")
    assert (np.abs(hf.double().numpy() - got.ref[0]) <= got.bound[0]).all()


def test_ambiguous_raws_are_found_and_score_models_assert_them():
    amb = ref.ambiguous_raws()
    assert all(abs(r) <= ref.RAW_MAX and r % 2 for r in amb)              # (odd: the even ladders cannot meet them)
    for r in amb:
        q = np.zeros((1, 1, 128), np.float16); K = np.zeros((1, 1, 1, 128), np.float16)
        q[0, 0, :2] = (1, 1); K[0, 0, 0, :2] = (r - np.sign(r) * 1000, np.sign(r) * 1000)
        with pytest.raises(AssertionError):
            ref.scores_eager(q, K)
    with pytest.raises(AssertionError):
        ref.scores_f32(np.full((1, 1, 128), 0.5, np.float16), np.ones((1, 1, 1, 128), np.float16))


@pytest.mark.parametrize("pos", [385, 700])
def test_each_family_needs_its_own_model(pos):
    """on the integers profile the eager-score and the fp32-score references are several bounds apart: a kernel judged by the other family's
    model would fail, which is why no test holds both families to one formula"""
    c = ref.decode_case("integers", 1, 4, 1, pos)
    e = ref.reference(ref.scores_eager(c.q, c.K), c.V, kernel="single")
    f = ref.reference(ref.scores_f32(c.q, c.K), c.V, kernel="gqa")
    assert (np.abs(e.ref - f.ref) >= FACTOR * np.maximum(e.bound, f.bound)).any()


def test_seams_hold_the_constants_of_the_sources():
    assert {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 383, 384, 385, 699, 700} <= set(ref.seams("single", 700))
    assert ref.split_chunk(4001, 16) == 256 and ref.split_chunk(3001, 4) == 768 and ref.split_chunk(257, 4) == 256
    s = set(ref.seams("split", 4000, 256))
    assert {7 * 256 + 255, 8 * 256, 15 * 256 - 1, 15 * 256, 3999, 4000} <= s            # chunks 7 / 8 (combine batches) .. 14 / 15 (the last boundary)
    assert ref.gqa_chunk(5120, 40) == 128 and ref.gqa_chunk(4096, 3) == 1408 and ref.gqa_chunk(4096, 4) == 1024 and ref.gqa_chunk(2048, 32) == 128
    s = set(ref.seams("gqa", 5000, 128))
    assert {31 * 128 + 127, 32 * 128, 39 * 128 - 1, 39 * 128} <= s       # chunks 31 / 32: the combine launch's first batch ends
    assert {47 * 128 + 127, 48 * 128} <= set(ref.seams("gqa", 6200, 128))  # ... and 47 / 48, its second (a cache longer than the cases here)
    assert ref.seams("gqa", 0, 128) == [0] and max(ref.seams("split", 1023, 256)) == 1023
    assert {383, 384, 385, 768 + 383, 768 + 384, 768 + 385, 3 * 768 + 384} <= set(ref.seams("split", 3000, 768))     # every chunk's remainder loop
    assert {2943, 2944, 2815, 2816} <= set(ref.seams("gqa", 2999, 1408))                # the new token's tile and stage: the chunk ends mid-stage


def _detect(mut, r, bound):
    return bool((np.abs(mut - r) >= FACTOR * bound).any())


@functools.lru_cache(maxsize=None)
def _walk(kernel, shape):
    """every launch of one decode shape -> findings: exactness (asserted on the way), profile conditions, undetected mutations, tightness.
    Which case must show what: the tied launch and the spotlight launches every seam key of the kernel (dropped, twice, neighbour); the other
    address-coded profiles every key their model gives >= P_HELD; a stale chunk maximum every chunk >= 1 on some spotlight ladder and the last
    chunk of ramp_up (elsewhere the chunk carries no mass that could move); the dense-V launch a shift of the output dimensions"""
    B, nh, nkv, max_seq, ns, pos = shape
    profiles = ref.single_profiles(pos) if kernel == "single" else ref.SPLIT_PROFILES
    chunk = ref.chunk_of(kernel, pos, max_seq, ns)
    sk = ref.seams(kernel, pos, chunk)
    n_act = -(-(pos + 1) // chunk) if chunk else 1
    problems, loose = [], []
    held = {"tied": set(), "spotlight": set()}
    chunk_seen = set()
    launches = ref.decode_launches(kernel, B, nh, nkv, pos, max_seq, ns, profiles)
    launches.append(("integers/denseV", ref.decode_case("integers", B, nh, nkv, pos, dense_v=True)))
    for name, c in launches:
        s = ref.scores(kernel, c.q, c.K)                               # asserts integers, |raw| <= 2048, no ambiguous raw, |s| <= 64
        if c.profile != "integers":
            assert np.array_equal(ref.raw_scores(c.q, c.K), c.raw), (name, "the designed scores are not what q . K gives")
        r = ref.reference(s, c.V, kernel=kernel)
        G = nh // nkv
        big = np.abs(r.ref) >= 2.0 ** -10
        share = float((r.bound[big] > 2.0 ** -8 * np.abs(r.ref[big])).mean()) if big.any() else 0.0
        if share > 0.01:
            loose.append((name, share))
        Vf = c.V.astype(np.float64)
        for b in range(B):
            for h in range(nh):
                p = r.p[b, h]
                if c.profile == "tied":
                    assert np.abs(p * (pos + 1) - 1).max() < 1e-12
                if c.profile == "spotlight":
                    ks = c.held[b][h]
                    ps = np.sort(p[ks])[::-1]
                    bg = np.delete(s[b, h], ks)
                    if not (len(ks) <= ref.LADDER_MAX and (ps[1:] / ps[:-1] <= 0.85).all() and ps.min() >= 2e-3
                            and (bg.size == 0 or s[b, h, ks].min() - bg.max() >= 39) and len({c.dims[b][h // G][k] for k in ks}) == len(ks)):
                        problems.append((name, b, h, "spotlight conditions"))
                if c.profile in ("only_new", "only_first"):
                    one = pos if c.profile == "only_new" else 0
                    if pos and s[b, h, one] - np.delete(s[b, h], one).max() < 40:
                        problems.append((name, b, h, "gap below 40"))
                if name.endswith("denseV"):                            # not address-coded: what it is there for is a dimension mix-up in P . V
                    if not _detect(np.roll(r.ref[b, h], 1), r.ref[b, h], r.bound[b, h]):
                        problems.append((name, b, h, "dimensions shifted by one: inside the bound"))
                    continue
                keys = ref.held_keys(c, r.p, b, h)
                if c.profile in held:
                    held[c.profile] |= set(keys)
                for t in keys:
                    for mname, mut in ref.mutants(s[b, h], Vf[b, h // G], t).items():
                        if not _detect(mut, r.ref[b, h], r.bound[b, h]):
                            problems.append((name, b, h, f"key {t} {mname}: inside {FACTOR} x bound"))
                if c.profile == "spotlight":                           # every chunk boundary is a seam: some head's ladder must show the stale maximum
                    for cc in range(1, n_act):
                        if _detect(ref.chunk_mutant(s[b, h], Vf[b, h // G], chunk, cc), r.ref[b, h], r.bound[b, h]):
                            chunk_seen.add(cc)
                if c.profile == "ramp_up" and n_act > 1:               # the last chunk holds the mass: under the previous chunk's maximum it loses it
                    if not _detect(ref.chunk_mutant(s[b, h], Vf[b, h // G], chunk, n_act - 1), r.ref[b, h], r.bound[b, h]):
                        problems.append((name, b, h, "last chunk combined with the previous chunk's maximum: inside the bound"))
    for prof, keys in held.items():                                      # every seam key is held by the tied launch AND by some head of some spotlight launch
        if set(sk) - keys:
            problems.append((prof, "seam keys no launch holds", sorted(set(sk) - keys)))
    if set(range(1, n_act)) - chunk_seen:
        problems.append(("chunks", "combined with the previous chunk's maximum", sorted(set(range(1, n_act)) - chunk_seen)))
    return problems, loose


@pytest.mark.parametrize("kernel,shape", SHAPES, ids=[_id(v) for v in SHAPES])
def test_decode_cases_are_exact_and_every_mutation_shows(kernel, shape):
    """(the causal mask of a decode step moved down by one is the new token dropped -- key pos is a seam of every case; moved up by one it reads a
    row the GPU module fills with NaN)"""
    problems, _ = _walk(kernel, shape)
    assert not problems, problems[:10]


@pytest.mark.parametrize("kernel,shape", SHAPES, ids=[_id(v) for v in SHAPES])
def test_decode_bound_is_tight(kernel, shape):
    _, loose = _walk(kernel, shape)
    assert not loose, loose


@functools.lru_cache(maxsize=None)
def _walk_prefill(shape):
    B, nh, nkv, S, pos0 = shape
    G = nh // nkv
    problems, loose = [], []
    mask = ref.causal_mask(S, pos0)
    cases = [(p, ref.prefill_case(p, B, nh, nkv, S, pos0)) for p in ref.PREFILL_PROFILES] + [("integers/denseV", ref.prefill_case("integers", B, nh, nkv, S, pos0, dense_v=True))]
    for name, c in cases:
        s = ref.scores("prefill", c.q, c.K)
        if c.profile != "integers":
            assert np.array_equal(ref.raw_scores(c.q, c.K), c.raw), name
        full = np.broadcast_to(mask, s.shape)
        r = ref.reference(s, c.V, full, kernel="prefill")
        big = np.abs(r.ref) >= 2.0 ** -10
        share = float((r.bound[big] > 2.0 ** -8 * np.abs(r.ref[big])).mean()) if big.any() else 0.0
        if share > 0.01:
            loose.append((name, share))
        Vf = c.V.astype(np.float64)
        rows = sorted({i for i in SEAM_ROWS + (S - 2, S - 1) if 0 <= i < S})
        if c.profile == "tied":
            vis = pos0 + np.arange(S) + 1
            assert np.abs(r.p * vis[None, None, :, None] - full).max() < 1e-12
            for sh in (-1, 1):                                         # the causal mask moved by one: every row it changes must show it
                m2 = ref.causal_mask(S, pos0, sh)
                m2[~m2.any(1)] = mask[~m2.any(1)]
                r2 = ref.reference(s, c.V, np.broadcast_to(m2, s.shape), kernel="prefill")
                changed = (m2 != mask).any(1)
                seen = (np.abs(r2.ref - r.ref) >= FACTOR * r.bound).any(-1)               # [B, nh, S]
                if not seen[:, :, changed].all():
                    problems.append((name, f"mask moved by {sh}", np.argwhere(~seen[:, :, changed])[:3].tolist()))
        if c.profile == "only_first" and pos0 + S > 1:
            if (np.where(full[..., 1:], s[..., :1] - s[..., 1:], 99) < 40).any():
                problems.append((name, "gap below 40"))
        for b in range(B):
            for h in range(nh):
                for i in rows:
                    n = pos0 + i + 1
                    if name.endswith("denseV"):
                        if not _detect(np.roll(r.ref[b, h, i], 1), r.ref[b, h, i], r.bound[b, h, i]):
                            problems.append((name, b, h, i, "dimensions shifted by one: inside the bound"))
                        continue
                    if c.profile == "tied":
                        keys = sorted({k for k in (0, 1, 63, 64, 65, 127, 128, n - 2, n - 1) if 0 <= k < n})
                    else:
                        keys = [int(k) for k in np.nonzero(r.p[b, h, i, :n] >= ref.P_HELD)[0]][:40]
                    for t in keys:
                        for mname, mut in ref.mutants(s[b, h, i, :n], Vf[b, h // G, :n], t).items():
                            if not _detect(mut, r.ref[b, h, i], r.bound[b, h, i]):
                                problems.append((name, b, h, i, f"key {t} {mname}: inside {FACTOR} x bound"))
    return problems, loose


@pytest.mark.parametrize("shape", PREFILL, ids=[_id(v) for v in PREFILL])
def test_prefill_cases_are_exact_and_every_mutation_shows(shape):
    problems, _ = _walk_prefill(shape)
    assert not problems, problems[:10]


@pytest.mark.parametrize("shape", PREFILL, ids=[_id(v) for v in PREFILL])
def test_prefill_bound_is_tight(shape):
    _, loose = _walk_prefill(shape)
    assert not loose, loose
