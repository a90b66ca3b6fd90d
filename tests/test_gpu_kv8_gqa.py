"""GPU: the matrix-core 8-bit attention kernel of grouped-query models (amq_attn_decode_kv8_gqa_f16, ops.attn_decode_kv8(kernel="mfma"),
QuantLlama(kv8_kernel="mfma")) against tests/kv8_ref.py's fp64 attention over the dequantized cache, the per-head kernel's cache bytes, the
position guard, the runner and the refusals.  Inputs: tests/test_gpu_kv8.py's."""
import numpy as np
import pytest
import torch

import kv8_ref
from test_gpu_kv8 import _arch_bits, _bands_intact, _bits, _caches, _dev, _random_setup, _run, _step_model

pytestmark = pytest.mark.gpu

HEADS = [(8, 2), (7, 1), (16, 1)]                # G = 4, 7 (ragged block), 16 (full block)
POS = {64: (0, 1, 31, 32, 63), 1024: (63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 1023)}
SPLITS = {64: (1,), 1024: (1, 2, 4, 0)}


def _launch(ops, inputs, pos, nh, nkv, tab, ns, kernel="mfma", sl=slice(None)):
    q, k, v, *caches = (t[sl].clone() for t in inputs)
    out = torch.zeros(q.shape[0], nh * 128, dtype=torch.float16, device=q.device)
    ops.attn_decode_kv8(q, k, v, *caches, out, pos, nh, nkv, table=tab, n_splits=ns, kernel=kernel)
    return out, caches


def _reference(ops, inputs, caches, pos, nh, nkv, tab):
    qr, kr = inputs[0].clone(), inputs[1].clone()
    ops.rope_rows(qr, kr, tab, 1, nh, nkv, pos0=pos)                         # the fp16-rotated q
    Kd = kv8_ref.dequantize(caches[0][:, :, :pos + 1], caches[1][:, :, :pos + 1])
    Vd = kv8_ref.dequantize(caches[2][:, :, :pos + 1], caches[3][:, :, :pos + 1])
    return kv8_ref.attention64(qr.cpu().view(-1, nh, 128).double().numpy(), Kd, Vd).reshape(qr.shape[0], -1)


@pytest.mark.parametrize("max_seq", [64, 1024])
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("B", [1, 3])
def test_random_inputs_against_fp64(max_seq, nh, nkv, B):
    from amq_amd import ops
    dev = _dev()
    tab = ops.rope_table(max_seq, 10000.0, dev)
    for pos in POS[max_seq]:
        inputs = _random_setup(B, nh, nkv, pos, max_seq, dev, 31 * pos + nh + B)
        _, c_dot = _launch(ops, inputs, pos, nh, nkv, tab, 1, kernel="dot")
        ref = _reference(ops, inputs, c_dot, pos, nh, nkv, tab)
        mx = np.abs(ref).max()
        for ns in SPLITS[max_seq]:
            got, c = _launch(ops, inputs, pos, nh, nkv, tab, ns)
            e = np.abs(got.cpu().double().numpy() - ref).max()
            print(f"kv8 gqa max_seq={max_seq} pos={pos} splits={ns} heads=({nh},{nkv}) B={B}: max err {e:.3e} of max |ref| {mx:.3e}")
            assert e <= 4e-3 * mx + 1e-3, (pos, ns)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(c, c_dot)), (pos, ns)      # the per-head kernel's cache, bit for bit
            assert torch.equal(_launch(ops, inputs, pos, nh, nkv, tab, ns)[0], got), (pos, ns)    # two runs: equal bits
            for b in range(B):                                                                    # a batch row = the single-sequence launch
                assert torch.equal(_launch(ops, inputs, pos, nh, nkv, tab, ns, sl=slice(b, b + 1))[0][0], got[b]), (pos, ns, b)
    assert all(int(t.abs().sum().item()) == 0 for t in ops._ATTN_TICKETS._cur.values())           # tickets left zero


def test_small_v_scales():
    """V scales of 2^-6 x [0.005, 0.035]: a kernel that rounds p s or s to fp16 loses them to fp16's subnormals; no absolute term in the bound"""
    from amq_amd import ops
    dev, nh, nkv, max_seq, pos = _dev(), 8, 2, 1024, 1023
    tab = ops.rope_table(max_seq, 10000.0, dev)
    inputs = _random_setup(1, nh, nkv, pos, max_seq, dev, 31 * pos + nh + 1)
    inputs[6] = inputs[6] * 2.0 ** -6
    for ns in (1, 4):
        got, c = _launch(ops, inputs, pos, nh, nkv, tab, ns)
        ref = _reference(ops, inputs, c, pos, nh, nkv, tab)
        mx, e = np.abs(ref).max(), np.abs(got.cpu().double().numpy() - ref).max()
        print(f"kv8 gqa small V scales splits={ns}: max err {e:.3e} of max |ref| {mx:.3e}")
        assert mx > 6.2e-5 and e <= 4e-3 * mx


@pytest.mark.parametrize("bad_pos", ["max_seq", -1])
@pytest.mark.parametrize("n_splits", [1, 3])
def test_position_guard(bad_pos, n_splits):
    from amq_amd import ops, _lib
    dev, nh, nkv, max_seq = _dev(), 8, 2, 1024
    (kc8, ks, vc8, vs), bands = _caches(2, nkv, max_seq, dev, code_fill=5, scale_fill=0.5)
    before = [t.clone() for t in (kc8, ks, vc8, vs)]
    q, k, v = (torch.randn(2, n * 128).half().to(dev) for n in (nh, nkv, nkv))
    out = torch.full((2, nh * 128), 7.0, dtype=torch.float16, device=dev)
    cur, pos_state, err = ops.new_step_state(dev)
    pos_state.fill_(max_seq if bad_pos == "max_seq" else -1)
    ops.attn_decode_kv8(q, k, v, kc8, ks, vc8, vs, out, pos_state, nh, nkv, cur=cur, n_splits=n_splits, kernel="mfma")
    torch.cuda.synchronize()
    assert int(err.item()) == 1 and bool((out == 7.0).all())
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((kc8, ks, vc8, vs), before)) and _bands_intact(bands)
    with pytest.raises(_lib.AmqError):
        ops.check_step_state(err)


def _gqa_cfg(nh=8, nkv=2):
    from amq_amd import arch
    return dict(arch._cfg(2, nh * 128, 1024, nh, nkv, 1, vocab=1024))


@pytest.mark.parametrize("max_seq,S", [(64, 12), (1024, 520)])
def test_runner(max_seq, S):
    """captured == eager bit for bit; logits within test_gpu_kv8.py's runner tolerance of the stepwise reference; the "dot" runner's cache bytes"""
    from amq_amd.llama import QuantLlama
    cfg = _gqa_cfg()
    al = _arch_bits(cfg)
    m = QuantLlama(cfg, al, device="cuda:0", max_seq=max_seq, seed=3, kv_bits=8, kv8_kernel="mfma")
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
    assert d.kv8_kernel == "dot" and m.kv8_kernel == "mfma"
    d.reset(); m.reset()
    d.prefill(ids, use_graph=False); m.prefill(ids, use_graph=False)
    for i, t in enumerate(toks):                    # both fed the same tokens: block 0's k / v rows do not depend on any attention output
        for r in (d, m):
            r.set_token(t)
            r.decode_step(use_graph=False)
        for key in m.cache_keys:                    # (rows behind the position: m's earlier runs)
            assert torch.equal(_bits(m.blocks[0][key][:, :, :S + i + 1]), _bits(d.blocks[0][key][:, :, :S + i + 1])), (key, i)


def test_refusals_say_why():
    from amq_amd import ops, _lib
    from amq_amd.llama import QuantLlama
    for cfg, kw, why in ((_gqa_cfg(), dict(kv_bits=16, kv8_kernel="mfma"), "needs kv_bits=8"),
                         (_gqa_cfg(4, 4), dict(kv_bits=8, kv8_kernel="mfma"), "grouped-query"),
                         (_gqa_cfg(), dict(kv_bits=8, kv8_kernel="wmma"), "'dot'.*'mfma'")):
        with pytest.raises(ValueError, match=why):
            QuantLlama(cfg, None, device="cuda:0", max_seq=64, **kw)
    dev = _dev()
    for nh, nkv, why in ((4, 4, "multi-head models: the per-head 8-bit kernel"), (32, 1, r"2\.\.16 query heads per kv head")):
        inputs = _random_setup(1, nh, nkv, 5, 64, dev, 1)
        with pytest.raises(_lib.AmqError, match=why):
            _launch(ops, inputs, 5, nh, nkv, None, 1)
    with pytest.raises(ValueError, match="'dot'.*'mfma'"):
        _launch(ops, _random_setup(1, 8, 2, 5, 64, dev, 1), 5, 8, 2, None, 1, kernel="wmma")
