"""GPU: the prompt kernel of the 8-bit KV cache (amq_attn_prefill_kv8_f16, ops.attn_prefill_kv8, QuantLlama(kv8_prompt="cache"))
against tests/kv8_ref.py's fp64 attention over the dequantized rows 0 .. pos0 + s of every query row, chunk invariance bit for bit, the runner fed
a prompt in chunks, and the refusals.  Inputs: tests/test_gpu_kv8.py's random caches (NaN scales behind the last valid row)."""
import numpy as np
import pytest
import torch

import kv8_ref
from test_gpu_kv8 import _arch_bits, _bands_intact, _bits, _caches, _dev, _random_setup, _step_model
from test_gpu_kv8_gqa import _gqa_cfg

pytestmark = pytest.mark.gpu

MAX_SEQ = 576
HEADS = [(4, 4), (8, 2), (7, 1)]
# (pos0, S): one row; a whole tile; one row past it; a chunk that starts on a tile's last row; a tile-aligned chunk; a chunk starting mid-tile; two
# query blocks behind 130 cached rows; five query blocks whose last tile reaches past the end (keys 0 .. 499)
CASES = [(0, 1), (0, 64), (0, 65), (63, 2), (64, 64), (1, 127), (130, 129), (200, 300)]


def _setup(B, nh, nkv, pos0, S, dev, seed):
    """-> q [B * S, nh * 128], the four guarded caches (rows 0 .. pos0 + S - 1 valid, NaN scales behind them), their guard bands"""
    rand = _random_setup(B, nh, nkv, pos0 + S - 1, MAX_SEQ, dev, seed)[3:]
    c, bands = _caches(B, nkv, MAX_SEQ, dev)
    for t, r in zip(c, rand):
        t.copy_(r)
    q = torch.randn(B * S, nh * 128, generator=torch.Generator().manual_seed(seed + 1)).half().to(dev)
    return q, list(c), bands


def _launch(ops, q, c, pos0, S, nh, nkv, B=1, out_xfrag=False):
    return ops.attn_prefill_kv8(q, *c, None if out_xfrag else torch.zeros_like(q), S, nh, nkv, batch=B, pos0=pos0, out_xfrag=out_xfrag)


def _reference(q, c, pos0, S, B, nh):
    """fp64, per query row s over the dequantized rows 0 .. pos0 + s -> [B * S, nh * 128]"""
    T = pos0 + S
    Kd, Vd = kv8_ref.dequantize(c[0][:, :, :T], c[1][:, :, :T]), kv8_ref.dequantize(c[2][:, :, :T], c[3][:, :, :T])
    qn = q.cpu().double().numpy().reshape(B, S, nh, 128)
    rows = [kv8_ref.attention64(qn[:, s], Kd[:, :, :pos0 + s + 1], Vd[:, :, :pos0 + s + 1]) for s in range(S)]
    return np.stack(rows, 1).reshape(B * S, nh * 128)


@pytest.mark.parametrize("pos0,S", CASES)
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("B", [1, 2])
def test_against_fp64(pos0, S, nh, nkv, B):
    from amq_amd import ops
    dev, H = _dev(), nh * 128
    q, c, bands = _setup(B, nh, nkv, pos0, S, dev, 31 * pos0 + S + nh + B)
    before = [t.clone() for t in c]
    got = _launch(ops, q, c, pos0, S, nh, nkv, B)
    ref = _reference(q, c, pos0, S, B, nh)
    mx, e = np.abs(ref).max(), np.abs(got.cpu().double().numpy() - ref).max()
    print(f"kv8 prefill pos0={pos0} S={S} heads=({nh},{nkv}) B={B}: max err {e:.3e} of max |ref| {mx:.3e}")
    assert e <= 4e-3 * mx + 1e-3
    assert torch.equal(_launch(ops, q, c, pos0, S, nh, nkv, B), got)                             # two launches: equal bits
    for b in range(B):                                                                            # a batch row = the single-sequence launch
        alone = _launch(ops, q[b * S:(b + 1) * S], [t[b:b + 1] for t in c], pos0, S, nh, nkv)
        assert torch.equal(alone, got[b * S:(b + 1) * S]), b
    assert all(torch.equal(_bits(a), _bits(b4)) for a, b4 in zip(c, before)) and _bands_intact(bands)
    if B == 1:                                                                                    # the fragment-ordered form: the same bits, zero pad rows
        xf = _launch(ops, q, c, pos0, S, nh, nkv, out_xfrag=True)
        assert torch.equal(xf, ops.xfrag(got, S, H))
        pad = ops.xfrag(torch.ones(S, H, dtype=torch.float16, device=dev), S, H) == 0
        assert int(pad.sum()) == (-S % 64) * H and bool((xf[pad] == 0).all())


@pytest.mark.parametrize("nh,nkv", [(8, 2), (7, 1)])
def test_chunk_invariance_bit_for_bit(nh, nkv):
    """the row at position p over the same cache bytes has the same bits however the launch that computes it is cut"""
    from amq_amd import ops
    T = 200
    q, c, _ = _setup(1, nh, nkv, 0, T, _dev(), 77 + nh)
    whole = _launch(ops, q, c, 0, T, nh, nkv)
    for a in (1, 63, 64, 65, 133):
        assert torch.equal(_launch(ops, q[a:].contiguous(), c, a, T - a, nh, nkv), whole[a:]), a


def test_small_v_scales():
    """V scales of 2^-6 x [0.005, 0.035] (tests/test_gpu_kv8_gqa.py::test_small_v_scales): no absolute term in the bound"""
    from amq_amd import ops
    nh, nkv, pos0, S = 8, 2, 130, 129
    q, c, _ = _setup(1, nh, nkv, pos0, S, _dev(), 5)
    c[3].mul_(2.0 ** -6)
    got = _launch(ops, q, c, pos0, S, nh, nkv)
    ref = _reference(q, c, pos0, S, 1, nh)
    mx, e = np.abs(ref).max(), np.abs(got.cpu().double().numpy() - ref).max()
    print(f"kv8 prefill small V scales: max err {e:.3e} of max |ref| {mx:.3e}")
    assert mx > 6.2e-5 and e <= 4e-3 * mx


def _chunked_run(m, ids, cuts, steps, use_graph):
    """the prompt fed in chunks ending at ``cuts``, then ``steps`` token steps -> logits rows (clones), the tokens fed to the steps"""
    m.reset()
    out, toks, a = [], [], 0
    for b in cuts:
        out.append(m.prefill(ids[a:b], use_graph=use_graph, start_pos=a).clone())
        a = b
    for _ in range(steps):
        toks.append(m.token.clone())
        m.decode_step(use_graph=use_graph)
        out.append(m.logits.clone())
    m.check()
    return out, toks


def test_runner_chunked_prompt():
    """135 tokens as chunks of 70, 60 and 5, then 4 steps, against the reference stepped token by token over dequantized rows -- what cache mode
    computes; captured == eager bit for bit; the same tokens in ONE pass stay within the bar"""
    from amq_amd.llama import QuantLlama
    cfg = _gqa_cfg()
    m = QuantLlama(cfg, _arch_bits(cfg), device="cuda:0", max_seq=160, seed=3, kv_bits=8, kv8_prompt="cache")
    ids = torch.randint(0, 1024, (135,), generator=torch.Generator().manual_seed(5)).to(_dev())
    cuts = (70, 130, 135)
    got, toks = _chunked_run(m, ids, cuts, 4, use_graph=True)
    ref = _step_model(m)
    ref.K = [torch.zeros(m.nkv, 0, 128, device=_dev()) for _ in m.blocks]
    ref.V = [torch.zeros(m.nkv, 0, 128, device=_dev()) for _ in m.blocks]
    rows = [ref.step(t) for t in list(ids) + toks]
    want = [rows[b - 1] for b in cuts] + rows[135:]
    scale = want[0].float().abs().max()
    for i, (g, w) in enumerate(zip(got, want)):
        e = float((g.view(-1).float() - w.float()).abs().max() / scale)
        print(f"kv8 chunked runner row {i}: max |dlogit| / max |ref| = {e:.2e}")
        assert e <= 2e-2, i
    eager, _ = _chunked_run(m, ids, cuts, 4, use_graph=False)
    assert all(torch.equal(a, b) for a, b in zip(eager, got))
    m.reset()
    one = m.prefill(ids, use_graph=False)
    assert float((one.view(-1).float() - want[2].float()).abs().max() / scale) <= 2e-2
    assert int(m.pos.item()) == 135


def test_hf_surface_serves_rows_behind_cached_rows():
    """convert_model_to_hip(kv8_prompt="cache"): model(ids, start_pos=p) with several rows behind cached rows is served; every row's logits within
    the kv8 runner tests' bar of HF's own fp16 forward over the oracle's weights (which does not quantize: the 8-bit rows' drift, 1e-3 .. 3e-3 of
    the largest logit in DESIGN.md 3.13's records, lies inside that bar)"""
    pytest.importorskip("transformers")
    from test_gpu_hf_fast import _prepared
    from amq_amd import hf_fast
    model, ref = _prepared("llama")
    with pytest.raises(ValueError, match="needs kv_bits=8"):
        hf_fast.convert_model_to_hip(model, kv8_prompt="cache")
    hf_fast.convert_model_to_hip(model, kv_bits=8, kv8_prompt="cache")
    try:
        ids = torch.randint(0, 1000, (1, 20), generator=torch.Generator().manual_seed(2)).to(_dev())
        with torch.inference_mode():
            first = model(ids[:, :12], start_pos=0, use_cache=False)
            more = model(ids[:, 12:], start_pos=12, use_cache=False)
            assert more["start_pos"] == 20 and hf_fast._RUNNERS[model][1].kv8_prompt == "cache"
            got, want = torch.cat([first.logits, more.logits], 1), ref(ids).logits.float()
            assert (got - want).abs().max() <= 2e-2 * want.abs().max()
    finally:
        hf_fast.revert_model_to_hf(model)


def test_refusals_say_why():
    from amq_amd import ops, _lib
    from amq_amd.llama import QuantLlama
    for kw, why in ((dict(kv_bits=16, kv8_prompt="cache"), "needs kv_bits=8"), (dict(kv_bits=8, kv8_prompt="scratch"), "'exact'.*'cache'")):
        with pytest.raises(ValueError, match=why):
            QuantLlama(_gqa_cfg(), None, device="cuda:0", max_seq=64, **kw)
    q, c, _ = _setup(1, 8, 2, 0, 4, _dev(), 1)
    with pytest.raises(ValueError, match="do not fit the cache"):
        _launch(ops, q, c, MAX_SEQ - 3, 4, 8, 2)
    q32, c1, _ = _setup(1, 32, 1, 0, 4, _dev(), 1)
    with pytest.raises(_lib.AmqError, match=r"1\.\.16 query heads per kv head"):
        _launch(ops, q32, c1, 0, 4, 32, 1)
    q2, c2, _ = _setup(2, 8, 2, 0, 4, _dev(), 1)
    with pytest.raises(ValueError, match="batch == 1"):
        _launch(ops, q2, c2, 0, 4, 8, 2, B=2, out_xfrag=True)
