"""GPU: the attention kernels read back key by key on inputs whose scores are known exactly (tests/attndomain_ref.py): integer q and K, an identity
rotation, address-coded V -- out[h, d] is the sum of the probabilities of the keys given dimension d.  Every launch is judged at EVERY element
against its family's own model (eager fp16 scores: attn_decode_kernel, attn_decode_split_kernel; fp32 scores: attn_decode_gqa_kernel +
attn_gqa_combine_kernel, attn_prefill_kernel) inside the bound derived there; an element no visible key points at must be +0 exactly.  What the
bound lets through -- and that a dropped, doubled or misread key, a stale chunk maximum or a mask off by one is NOT among it -- is
tests/test_attndomain_cpu.py's business.  Every launch runs through the product library and the conservative-waits twin (_both), twice: the same
bits; the appended cache rows are the new k and v bit for bit; tickets are zero after every split launch.  Each judged launch prints one line:
attndomain | kernel | case | elements | worst |err| / bound."""
import functools

import numpy as np
import pytest
import torch

import attndomain_ref as ref
from test_gpu_metadomain import _both, _dev, _t

pytestmark = pytest.mark.gpu


def _keys_of(V, vis, d):
    """the visible keys a V [T, 128] gives dimension d"""
    return [int(t) for t in np.nonzero((V[:, d] != 0) & vis)[0]]


def _judge(kernel, name, out, r, V, vis, G):
    """out [B, nh, (S,) 128] fp16 against Ref r at every element; V [B, nkv, T, 128], vis broadcastable to [B, nh, (S,) T]"""
    out = np.asarray(out, np.float16)
    assert out.shape == r.ref.shape, (out.shape, r.ref.shape)
    err = np.abs(out.astype(np.float64) - r.ref)
    ratio = err / r.bound
    worst = float(np.nanmax(ratio)) if np.isfinite(out).all() else float("nan")
    print(f"attndomain | {kernel} | {name} | {out.size} | {worst:.3f}")
    vis = np.broadcast_to(vis, r.p.shape)
    Vf = np.where(np.isnan(V), 0, V).astype(np.float64)
    shp = r.p.shape
    mass = np.matmul(vis.reshape(shp[0], Vf.shape[1], -1, shp[-1]).astype(np.float64), np.abs(Vf)).reshape(r.ref.shape)
    bad = ~(ratio <= 1.0) | ((mass == 0) & (out.view(np.uint16) != 0))
    if bad.any():
        idx = tuple(int(v) for v in np.argwhere(bad)[0])
        b, h, d = idx[0], idx[1], idx[-1]
        pv = r.p[idx[:-1]]
        keys = _keys_of(Vf[b, h // G], vis[idx[:-1]], d)
        top = sorted(keys, key=lambda t: -pv[t])[:12]
        pytest.fail(f"{kernel} | {name}: {int(bad.sum())} of {bad.size} elements outside the bound (worst |err| / bound {worst:.3f}); first at sequence {b}, head {h}"
                    + (f", row {idx[2]}" if len(idx) == 4 else "") + f", dimension {d}: kernel {float(out[idx])!r} (0x{int(out.view(np.uint16)[idx]):04x}), model "
                    f"{r.ref[idx]!r}, bound {r.bound[idx]!r}; {len(keys)} visible keys point there"
                    + (" (must be +0)" if not keys else f", the heaviest (key: model probability x value): {[(t, float(pv[t]), float(Vf[b, h // G, t, d])) for t in top]}"))
    return worst


@functools.lru_cache(maxsize=None)
def _identity_rotation(max_seq):
    tab = torch.zeros(max_seq, 64, 2, dtype=torch.float16)
    tab[..., 0] = 1.0
    return tab.to(_dev())


def _tickets_zero():
    from amq_amd import ops
    return all(int(t.abs().sum().item()) == 0 for t in ops._ATTN_TICKETS._cur.values())


def _decode(c, B, nh, nkv, pos, max_seq, n_splits, source):
    """one decode step of Case c over a cache of max_seq rows (rows past pos: NaN) -> out [B, nh, 128] fp16 (numpy), judged for the side effects: the
    appended rows are k and v, nothing else is written, tickets zero, twin and second launch give the same bits"""
    from amq_amd import ops
    dev = _dev()
    kc = torch.full((B, nkv, max_seq, 128), float("nan"), dtype=torch.float16)
    vc = torch.full((B, nkv, max_seq, 128), float("nan"), dtype=torch.float16)
    kc[:, :, :pos] = torch.from_numpy(c.K[:, :, :pos]); vc[:, :, :pos] = torch.from_numpy(c.V[:, :, :pos])
    kc, vc = kc.to(dev), vc.to(dev)
    q, k, v = _t(c.q.reshape(B, nh * 128)), _t(c.K[:, :, pos].reshape(B, nkv * 128)), _t(c.V[:, :, pos].reshape(B, nkv * 128))
    tab = _identity_rotation(max_seq)

    def run():
        kc_, vc_ = kc.clone(), vc.clone()
        out = torch.zeros(B, nh * 128, dtype=torch.float16, device=dev)
        if source == "cur":
            cur, pos_state, err = ops.new_step_state(dev)
            cur.copy_(tab[0].reshape(128)); pos_state.fill_(pos)
            ops.attn_decode(q, k, v, kc_, vc_, out, pos_state, nh, nkv, cur=cur, n_splits=n_splits)
            assert int(err.item()) == 0
        else:
            ops.attn_decode(q, k, v, kc_, vc_, out, torch.full((1,), pos, dtype=torch.int32, device=dev), nh, nkv, table=tab, n_splits=n_splits)
        assert _tickets_zero()
        assert torch.equal(kc_[:, :, :pos], kc[:, :, :pos]) and torch.equal(vc_[:, :, :pos], vc[:, :, :pos])
        assert torch.isnan(kc_[:, :, pos + 1:]).all() and torch.isnan(vc_[:, :, pos + 1:]).all()
        return torch.cat([out.reshape(-1), kc_[:, :, pos].reshape(-1), vc_[:, :, pos].reshape(-1)])

    y = _both(run)
    assert np.array_equal(_both(run).view(np.uint16), y.view(np.uint16)), "a second launch computes other bits"
    n = B * nh * 128
    app = y[n:].view(np.uint16)
    assert np.array_equal(app[:B * nkv * 128], c.K[:, :, pos].reshape(-1).view(np.uint16)), "the appended key row is not k"
    assert np.array_equal(app[B * nkv * 128:], c.V[:, :, pos].reshape(-1).view(np.uint16)), "the appended value row is not v"
    return y[:n].reshape(B, nh, 128)


def _decode_shape(kernel, B, nh, nkv, pos, max_seq, n_splits, profiles, sources):
    worst = 0.0
    launches = ref.decode_launches(kernel, B, nh, nkv, pos, max_seq, n_splits, profiles)
    launches.append(("integers/denseV", ref.decode_case("integers", B, nh, nkv, pos, dense_v=True)))
    for name, c in launches:
        r = ref.reference(ref.scores(kernel, c.q, c.K), c.V, kernel=kernel)
        outs = {}
        for source in sources:
            what = f"{name} {nh}/{nkv} heads x{B} pos {pos} of {max_seq} splits {n_splits} {source}"
            outs[source] = _decode(c, B, nh, nkv, pos, max_seq, n_splits, source)
            worst = max(worst, _judge(kernel, what, outs[source], r, c.V, np.ones((1, 1, pos + 1), bool), nh // nkv))
            if c.profile in ("only_new", "only_first"):               # the output is one V row, exactly
                one = pos if c.profile == "only_new" else 0
                want = np.repeat(c.V[:, :, one], nh // nkv, 1)
                assert np.array_equal(outs[source].view(np.uint16), want.view(np.uint16)), what
        if len(sources) == 2:
            assert np.array_equal(outs["table"].view(np.uint16), outs["cur"].view(np.uint16)), (name, "the two position sources give other bits")
        if kernel == "split" and pos + 1 <= ref.split_chunk(pos + 1, n_splits):     # one active chunk: the single-workgroup kernel's bits
            one = _decode(c, B, nh, nkv, pos, max_seq, 1, "table")
            assert np.array_equal(one.view(np.uint16), outs["table"].view(np.uint16)), (name, "one active chunk, other bits than the single-workgroup kernel")
    return worst


# ------------------------------------------------------------------------------------------------ 1. the single-workgroup kernel (eager model)
@pytest.mark.parametrize("pos", ref.SINGLE_POS)
@pytest.mark.parametrize("nh,nkv", ref.SINGLE_HEADS)
def test_single_workgroup_kernel(nh, nkv, pos):
    _decode_shape("single", 1, nh, nkv, pos, 1024, 1, ref.single_profiles(pos), ("table", "cur"))


def test_single_workgroup_kernel_two_sequences():
    _decode_shape("single", 2, 4, 1, 385, 1024, 1, ref.ALL, ("table", "cur"))


# ------------------------------------------------------------------------------------------------ 2. the per-head split kernel (eager scores)
@pytest.mark.parametrize("max_seq,n_splits,pos", ref.SPLIT_SHAPES)
def test_split_kernel(max_seq, n_splits, pos):
    _decode_shape("split", 1, 2, 2, pos, max_seq, n_splits, ref.SPLIT_PROFILES, ("table", "cur"))


# ------------------------------------------------------------------------------------------------ 3. the grouped matrix-core kernel + its combine launch
@pytest.mark.parametrize("max_seq,n_splits,pos", ref.GQA_SHAPES)
@pytest.mark.parametrize("nh,nkv,B", ref.GQA_HEADS)
def test_grouped_kernel_and_combine(nh, nkv, B, max_seq, n_splits, pos):
    _decode_shape("gqa", B, nh, nkv, pos, max_seq, n_splits, ref.SPLIT_PROFILES, ("table", "cur"))


# ------------------------------------------------------------------------------------------------ 4. the prompt kernel (fp32 model, causal)
def _unfrag(x, S, nh):
    """amq_xfrag_f16's layout of the [S, nh * 128] matrix (K tile = head) -> row-major [S, nh, 128]"""
    s, h, dd = np.meshgrid(np.arange(S), np.arange(nh), np.arange(128), indexing="ij")
    at = ((((s >> 6) * nh + h) * 16 + ((s & 63) >> 4) * 4 + dd // 32) * 64 + 16 * ((dd & 31) >> 3) + (s & 15)) * 8 + (dd & 7)
    return np.asarray(x).reshape(-1)[at]


def _prefill(c, B, nh, nkv, S, pos0, kv_cache, out_xfrag=False):
    """-> out [B, nh, S, 128] fp16 (numpy); product and twin, two launches: the same bits"""
    from amq_amd import ops
    dev = _dev()
    T = pos0 + S
    q = _t(c.q.transpose(0, 2, 1, 3).reshape(B * S, nh * 128))
    if kv_cache:
        k = torch.full((B, nkv, T + 9, 128), float("nan"), dtype=torch.float16); v = k.clone()       # rows past the context must never be read into the result
        k[:, :, :T] = torch.from_numpy(c.K); v[:, :, :T] = torch.from_numpy(c.V)
        k, v = k.to(dev), v.to(dev)
    else:
        assert pos0 == 0
        k, v = _t(c.K.transpose(0, 2, 1, 3).reshape(B * S, nkv * 128)), _t(c.V.transpose(0, 2, 1, 3).reshape(B * S, nkv * 128))
    if out_xfrag:
        assert B == 1
        like = ops.xfrag(q, S, nh * 128)

    def run():
        out = torch.full_like(like, float("nan")) if out_xfrag else torch.full_like(q, float("nan"))
        return ops.attn_prefill(q, k, v, out, S, nh, nkv, batch=B, pos0=pos0, kv_cache=kv_cache, out_xfrag=out_xfrag)

    y = _both(run)
    assert np.array_equal(_both(run).view(np.uint16), y.view(np.uint16)), "a second launch computes other bits"
    if out_xfrag:
        y = _unfrag(y, S, nh)[None]
        return y.transpose(0, 2, 1, 3)
    return y.reshape(B, S, nh, 128).transpose(0, 2, 1, 3)


def _prefill_shape(B, nh, nkv, S, pos0, kv_cache, xfrag=False):
    mask = ref.causal_mask(S, pos0)
    cases = [(p, ref.prefill_case(p, B, nh, nkv, S, pos0)) for p in ref.PREFILL_PROFILES]
    cases.append(("integers/denseV", ref.prefill_case("integers", B, nh, nkv, S, pos0, dense_v=True)))
    for name, c in cases:
        s = ref.scores("prefill", c.q, c.K)
        r = ref.reference(s, c.V, np.broadcast_to(mask, s.shape), kernel="prefill")
        what = f"{name} {nh}/{nkv} heads x{B} S {S} pos0 {pos0}" + (" cache" if kv_cache else "") + (" xfrag" if xfrag else "")
        out = _prefill(c, B, nh, nkv, S, pos0, kv_cache)
        _judge("prefill", what, out, r, c.V, mask[None, None], nh // nkv)
        if xfrag:
            assert np.array_equal(_prefill(c, B, nh, nkv, S, pos0, kv_cache, out_xfrag=True).view(np.uint16), np.ascontiguousarray(out).view(np.uint16)), what
        if name == "tied" and pos0 + S <= 128:       # V = I: the whole causal probability matrix -- row i reads exactly 1 / (pos0 + i + 1) on its keys, +0 above the diagonal
            want = np.where(mask, (1.0 / (pos0 + np.arange(S) + 1.0))[:, None], 0.0).astype(np.float16)
            got = out[..., :pos0 + S]
            assert np.array_equal(got.view(np.uint16), np.broadcast_to(want, got.shape).view(np.uint16)), what
            assert not out[..., pos0 + S:].view(np.uint16).any()
        if name == "only_first":
            want = np.broadcast_to(np.repeat(c.V[:, :, 0], nh // nkv, 1)[:, :, None, :], out.shape)
            assert np.array_equal(out.view(np.uint16), want.view(np.uint16)), what


@pytest.mark.parametrize("S", [1, 15, 16, 17, 63, 64, 65, 128, 129, 200])
@pytest.mark.parametrize("nh,nkv", [(2, 2), (4, 1)])
def test_prompt_kernel(nh, nkv, S):
    """S <= 128: V = I, the whole causal probability matrix is read back"""
    _prefill_shape(1, nh, nkv, S, 0, False, xfrag=S in (17, 64, 65))


@pytest.mark.parametrize("pos0", [11, 64, 100])
@pytest.mark.parametrize("S", [5, 64])
@pytest.mark.parametrize("nh,nkv", [(2, 2), (4, 1)])
def test_prompt_kernel_behind_cached_keys(nh, nkv, S, pos0):
    _prefill_shape(1, nh, nkv, S, pos0, True)


@pytest.mark.parametrize("nh,nkv", [(2, 2), (4, 1)])
def test_prompt_kernel_two_sequences(nh, nkv):
    _prefill_shape(2, nh, nkv, 65, 0, False)
