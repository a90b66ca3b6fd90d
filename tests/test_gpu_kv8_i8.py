"""GPU: the integer matrix-core 8-bit attention kernel (amq_attn_decode_kv8_i8_f16, ops.attn_decode_kv8(kernel="i8"),
QuantLlama(kv8_kernel="i8")) for 1 .. 16 query heads per kv head against tests/kv8_ref.py's fp64 attention over the dequantized cache with the
unquantized fp16-rotated q, the per-head kernel's cache bytes, the position guard, the runner and the refusals.  Inputs: tests/test_gpu_kv8.py's."""
import numpy as np
import pytest
import torch

from test_gpu_kv8 import _arch_bits, _bands_intact, _bits, _caches, _dev, _random_setup, _run, _step_model
from test_gpu_kv8_gqa import POS, SPLITS, _gqa_cfg, _launch, _reference

pytestmark = pytest.mark.gpu

HEADS = [(4, 4), (8, 2), (7, 1), (16, 1)]        # G = 1 (15 padding rows), 4, 7 (ragged block), 16 (full block)


@pytest.mark.parametrize("qmul", [1, 4])
@pytest.mark.parametrize("max_seq", [64, 1024])
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("B", [1, 3])
def test_random_inputs_against_fp64(max_seq, nh, nkv, B, qmul):
    """two int8 planes of q and of the weights stay near 2e-4 of max |ref| on these inputs; one plane of either (>= 1e-2) fails the bar"""
    from amq_amd import ops
    dev = _dev()
    tab = ops.rope_table(max_seq, 10000.0, dev)
    for pos in POS[max_seq]:
        inputs = _random_setup(B, nh, nkv, pos, max_seq, dev, 31 * pos + nh + B)
        inputs[0] = inputs[0] * qmul
        _, c_dot = _launch(ops, inputs, pos, nh, nkv, tab, 1, kernel="dot")
        ref = _reference(ops, inputs, c_dot, pos, nh, nkv, tab)
        mx = np.abs(ref).max()
        for ns in SPLITS[max_seq]:
            got, c = _launch(ops, inputs, pos, nh, nkv, tab, ns, kernel="i8")
            e = np.abs(got.cpu().double().numpy() - ref).max()
            print(f"kv8 i8 max_seq={max_seq} pos={pos} splits={ns} heads=({nh},{nkv}) B={B} q x{qmul}: max err {e:.3e} of max |ref| {mx:.3e}")
            assert e <= 4e-3 * mx + 1e-3, (pos, ns)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(c, c_dot)), (pos, ns)      # the per-head kernel's cache, bit for bit
            assert torch.equal(_launch(ops, inputs, pos, nh, nkv, tab, ns, kernel="i8")[0], got), (pos, ns)       # two runs: equal bits
            for b in range(B):                                                                    # a batch row = the single-sequence launch
                assert torch.equal(_launch(ops, inputs, pos, nh, nkv, tab, ns, kernel="i8", sl=slice(b, b + 1))[0][0], got[b]), (pos, ns, b)


@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 2)])
def test_small_v_scales(nh, nkv):
    """V scales of 2^-6 x [0.005, 0.035] enter through w = p vs in fp32 only; no absolute term in the bound"""
    from amq_amd import ops
    dev, max_seq, pos = _dev(), 1024, 1023
    tab = ops.rope_table(max_seq, 10000.0, dev)
    inputs = _random_setup(1, nh, nkv, pos, max_seq, dev, 31 * pos + nh + 1)
    inputs[6] = inputs[6] * 2.0 ** -6
    for ns in (1, 4):
        got, c = _launch(ops, inputs, pos, nh, nkv, tab, ns, kernel="i8")
        ref = _reference(ops, inputs, c, pos, nh, nkv, tab)
        mx, e = np.abs(ref).max(), np.abs(got.cpu().double().numpy() - ref).max()
        print(f"kv8 i8 small V scales heads=({nh},{nkv}) splits={ns}: max err {e:.3e} of max |ref| {mx:.3e}")
        assert mx > 6.2e-5 and e <= 4e-3 * mx


@pytest.mark.parametrize("bad_pos", ["max_seq", -1])
@pytest.mark.parametrize("n_splits", [1, 3])
def test_position_guard(bad_pos, n_splits):
    from amq_amd import ops, _lib
    dev, nh, nkv, max_seq = _dev(), 4, 4, 1024
    (kc8, ks, vc8, vs), bands = _caches(2, nkv, max_seq, dev, code_fill=5, scale_fill=0.5)
    before = [t.clone() for t in (kc8, ks, vc8, vs)]
    q, k, v = (torch.randn(2, n * 128).half().to(dev) for n in (nh, nkv, nkv))
    out = torch.full((2, nh * 128), 7.0, dtype=torch.float16, device=dev)
    cur, pos_state, err = ops.new_step_state(dev)
    pos_state.fill_(max_seq if bad_pos == "max_seq" else -1)
    ops.attn_decode_kv8(q, k, v, kc8, ks, vc8, vs, out, pos_state, nh, nkv, cur=cur, n_splits=n_splits, kernel="i8")
    torch.cuda.synchronize()
    assert int(err.item()) == 1 and bool((out == 7.0).all())
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((kc8, ks, vc8, vs), before)) and _bands_intact(bands)
    with pytest.raises(_lib.AmqError):
        ops.check_step_state(err)


@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("max_seq,S", [(64, 12), (1024, 520)])
def test_runner(max_seq, S, nh, nkv):
    """captured == eager bit for bit; logits within test_gpu_kv8.py's runner tolerance of the stepwise reference; the "dot" runner's cache bytes"""
    from amq_amd.llama import QuantLlama
    cfg = _gqa_cfg(nh, nkv)
    al = _arch_bits(cfg)
    m = QuantLlama(cfg, al, device="cuda:0", max_seq=max_seq, seed=3, kv_bits=8, kv8_kernel="i8")
    ids = torch.randint(0, 1024, (S,), generator=torch.Generator().manual_seed(5)).to(_dev())
    got, toks = _run(m, ids, 5, graph_from=2)
    ref = _step_model(m)
    want = [ref.prompt(ids)] + [ref.step(t) for t in toks]
    scale = want[0].float().abs().max()
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g.view(-1).float() - w.float()).abs().max() <= 2e-2 * scale, i
    eager, _ = _run(m, ids, 5, graph_from=99)
    assert all(torch.equal(a, b) for a, b in zip(eager, got))
    d = QuantLlama(cfg, al, device="cuda:0", max_seq=max_seq, seed=3, kv_bits=8)
    assert d.kv8_kernel == "dot" and m.kv8_kernel == "i8"
    d.reset(); m.reset()
    d.prefill(ids, use_graph=False); m.prefill(ids, use_graph=False)
    for i, t in enumerate(toks):                    # both fed the same tokens: block 0's k / v rows do not depend on any attention output
        for r in (d, m):
            r.set_token(t)
            r.decode_step(use_graph=False)
        for key in m.cache_keys:
            assert torch.equal(_bits(m.blocks[0][key][:, :, :S + i + 1]), _bits(d.blocks[0][key][:, :, :S + i + 1])), (key, i)


def test_refusals_say_why():
    from amq_amd import ops, _lib
    from amq_amd.llama import QuantLlama
    for cfg, kw, why in ((_gqa_cfg(), dict(kv_bits=16, kv8_kernel="i8"), "needs kv_bits=8"),
                         (_gqa_cfg(32, 1), dict(kv_bits=8, kv8_kernel="i8"), "1 .. 16 query heads"),
                         (_gqa_cfg(), dict(kv_bits=8, kv8_kernel="i4"), "'dot'.*'mfma'.*'i8'")):
        with pytest.raises(ValueError, match=why):
            QuantLlama(cfg, None, device="cuda:0", max_seq=64, **kw)
    dev = _dev()
    with pytest.raises(_lib.AmqError, match=r"1\.\.16 query heads per kv head"):
        _launch(ops, _random_setup(1, 32, 1, 5, 64, dev, 1), 5, 32, 1, None, 1, kernel="i8")
    with pytest.raises(ValueError, match="'dot'.*'mfma'.*'i8'"):
        _launch(ops, _random_setup(1, 8, 2, 5, 64, dev, 1), 5, 8, 2, None, 1, kernel="i4")
