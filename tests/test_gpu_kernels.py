"""GPU parity: HIP kernels (through the C ABI) vs the CPU oracle.

Bar: bit-exact for integer work and for the dequantized fp16 weights;
matmul outputs within 1e-3 relative (fp16) of the reference CPU path
nn.Linear-on-dequantized-weights (BASELINE.json north_star)."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import hqq_ref, gptq_ref, awq_ref, linear_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = sorted(glob.glob(os.path.join(GOLDEN, "hqq_b*.npz")))
RTOL = 1e-3


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _load(path):
    d = np.load(path)
    return {k: d[k] for k in d.files}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _assert_close_biased(y, y_ref, what=""):
    """outputs with a bias added as a SECOND fp16 rounding (the unfused reference's order): the two roundings of two summation orders can differ by two
    fp16 ulps on an element, one more than _assert_close's bar grants near |y| ~ rms"""
    y, y_ref = np.asarray(y, np.float32), np.asarray(y_ref, np.float32)
    floor = RTOL * float(np.sqrt(np.mean(y_ref.astype(np.float64) ** 2)))
    err = np.abs(y - y_ref)
    bad = err > (RTOL + 2.0 ** -10) * np.abs(y_ref) + floor
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} out of tolerance, max err {err.max()}"


def _assert_close(y, y_ref, what=""):
    """|y - ref| <= 1e-3*|ref| + 1e-3*rms(ref): fp16-relative with a floor for
    outputs that cancel to ~0 (one fp16 ulp of a typical output)."""
    y = np.asarray(y, np.float32)
    y_ref = np.asarray(y_ref, np.float32)
    floor = RTOL * float(np.sqrt(np.mean(y_ref.astype(np.float64) ** 2)))
    err = np.abs(y - y_ref)
    bad = err > RTOL * np.abs(y_ref) + floor
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} out of tolerance, max err {err.max()}"


def _native_from_golden(g):
    from amq_amd import ops
    bits, (n, k) = int(g["nbits"]), tuple(int(v) for v in g["shape"])
    qn, mn = ops.repack_from_hqq(_t(g["W_q"]), _t(g["scale"].reshape(-1)), _t(g["zero"].reshape(-1)), bits, n, k)
    return bits, n, k, qn, mn


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(c) for c in CASES])
def test_repack_dequant_bit_exact_golden(path):
    """native repack + in-register unpack + (q - z) * s reproduces the
    reference's HQQLinear.dequantize() bit for bit."""
    from amq_amd import ops
    g = _load(path)
    bits, n, k, qn, mn = _native_from_golden(g)
    w = ops.dequantize(qn, mn, bits, ops.MODE_HQQ, n, k).cpu().numpy()
    assert np.array_equal(w.view(np.uint16), g["W_deq"].view(np.uint16))
    w2 = ops.dequantize_hqq(_t(g["W_q"]), _t(g["scale"].reshape(-1)), _t(g["zero"].reshape(-1)), bits, n, k).cpu().numpy()
    assert np.array_equal(w2.view(np.uint16), g["W_deq"].view(np.uint16))


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(c) for c in CASES])
def test_forward_matches_reference_golden(path):
    """y for the reference's own captured x (3 rows) and for 1 row, vs the
    captured torch CPU result."""
    from amq_amd import ops
    g = _load(path)
    bits, n, k, qn, mn = _native_from_golden(g)
    bias = _t(g["bias"]) if "bias" in g else None
    y3 = ops.gemv(_t(g["x"]), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias).cpu().numpy()
    _assert_close(y3, g["y_ref"], "gemv M=3")
    y1 = ops.gemv(_t(g["x"][:1]), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias).cpu().numpy()
    _assert_close(y1, g["y_ref"][:1], "gemv M=1")
    ym = ops.gemm(_t(g["x"]), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias).cpu().numpy()
    _assert_close(ym, g["y_ref"], "gemm M=3")
    # M=128 rows: the GPTQLinear fallback capture uses the same integers; compare to the oracle on W_deq
    xg = g["gptq_x"]
    yg = ops.gemm(_t(xg), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias).cpu().numpy()
    _assert_close(yg, linear_ref.linear_f16(xg, g["W_deq"], g.get("bias")), "gemm M=128")


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(c) for c in CASES])
def test_gptq_and_awq_import_golden(path):
    """Format B / C buffers captured from the reference -> native (MODE_FMA):
    integers identical, weights equal the reference kernels' fma dequant."""
    from amq_amd import ops
    g = _load(path)
    bits, (n, k) = int(g["nbits"]), tuple(int(v) for v in g["shape"])
    qn, mn = ops.repack_from_gptq(_t(g["gptq_qweight"]), _t(g["gptq_scales"]), _t(g["gptq_zeros"]), bits, n, k)
    w = ops.dequantize(qn, mn, bits, ops.MODE_FMA, n, k).cpu().numpy()
    w_ref = gptq_ref.dequant_kernel(g["gptq_qweight"], g["gptq_scales"], g["gptq_zeros"], bits)
    assert np.array_equal(w.view(np.uint16), w_ref.view(np.uint16))
    # same payload as the HQQ import (the packed integers are the same integers)
    _, _, _, qn_h, _ = _native_from_golden(g)
    assert torch.equal(qn, qn_h)
    y = ops.gemm(_t(g["gptq_x"]), qn, mn, bits, ops.MODE_FMA, n, k).cpu().numpy()
    # parity with the reference CUDA kernels' arithmetic (fma dequant)
    _assert_close(y, linear_ref.linear_f16(g["gptq_x"], w_ref), "gptq-format forward, kernel arithmetic")
    # GPTQLinear.forward's captured torch fallback rounds the weight twice
    # (s*q, then -zeros; autogptq.py:281) where the kernels fuse: the
    # reference's two branches differ from each other by up to one weight ulp,
    # so this capture is matched to 3e-3 of the output rms, not 1e-3
    yf = g["gptq_y"].astype(np.float32)
    assert np.max(np.abs(y.astype(np.float32) - yf)) <= 3e-3 * np.sqrt(np.mean(yf ** 2)) + 1e-3 * np.max(np.abs(yf))
    if bits == 4:
        qa, ma = ops.repack_from_awq(_t(g["awq_qweight"]), _t(g["awq_scales"]), _t(g["awq_scaled_zeros"]), n, k)
        assert torch.equal(qa, qn_h)
        wa = ops.dequantize(qa, ma, 4, ops.MODE_FMA, n, k).cpu().numpy()
        wa_ref = awq_ref.dequant_kernel(g["awq_qweight"], g["awq_scales"], g["awq_scaled_zeros"])
        assert np.array_equal(wa.view(np.uint16), wa_ref.view(np.uint16))


def _random_case(bits, n, k, seed, bias=False):
    from amq_amd.hqq_format import random_hqq
    from amq_amd import ops
    h = random_hqq(n, k, bits, seed=seed, bias=bias)
    hd = h.to(_dev())
    qn, mn = ops.repack_from_hqq(hd.W_q, hd.scale.reshape(-1), hd.zero.reshape(-1), bits, n, k)
    w_ref = hqq_ref.dequantize(h.W_q.numpy(), h.scale.numpy(), h.zero.numpy(), bits, (n, k))
    return h, qn, mn, w_ref


GCASES = sorted(glob.glob(os.path.join(GOLDEN, "hqq_g*_b*.npz")))


@pytest.mark.parametrize("path", GCASES, ids=[os.path.basename(c) for c in GCASES])
def test_group256_reference_golden(path):
    """the reference's own group-256, group-64 and group-32 layers (HQQ Format A payload and GPTQLinear buffers): native dequant == its
    W_deq bit for bit, outputs vs its captured CPU results (GEMV kernel; 128 rows: the fused kernels at 256, dequantize-once + the fp16
    GEMM at 64 / 32), GPTQ import == the reference kernels' fma dequant"""
    from amq_amd import ops
    g = _load(path)
    bits, (n, k), G = int(g["nbits"]), tuple(int(v) for v in g["shape"]), int(g["group_size"])
    qn, mn = ops.repack_from_hqq(_t(g["W_q"]), _t(g["scale"].reshape(-1)), _t(g["zero"].reshape(-1)), bits, n, k, group=G)
    w = ops.dequantize(qn, mn, bits, ops.MODE_HQQ, n, k).cpu().numpy()
    assert np.array_equal(w.view(np.uint16), g["W_deq"].view(np.uint16))
    w2 = ops.dequantize_hqq(_t(g["W_q"]), _t(g["scale"].reshape(-1)), _t(g["zero"].reshape(-1)), bits, n, k, group=G).cpu().numpy()
    assert np.array_equal(w2.view(np.uint16), g["W_deq"].view(np.uint16))
    _assert_close(ops.gemv(_t(g["x"]), qn, mn, bits, ops.MODE_HQQ, n, k).cpu().numpy(), g["y_ref"], f"gemv M=3, group {G}")
    _assert_close(ops.gemm(_t(g["gptq_x"]), qn, mn, bits, ops.MODE_HQQ, n, k).cpu().numpy(),
                  linear_ref.linear_f16(g["gptq_x"], g["W_deq"]), f"gemm M=128, group {G}")
    qg, mg = ops.repack_from_gptq(_t(g["gptq_qweight"]), _t(g["gptq_scales"]), _t(g["gptq_zeros"]), bits, n, k, group=G)
    wg = ops.dequantize(qg, mg, bits, ops.MODE_FMA, n, k).cpu().numpy()
    assert np.array_equal(wg.view(np.uint16), gptq_ref.dequant_kernel(g["gptq_qweight"], g["gptq_scales"], g["gptq_zeros"], bits, G).view(np.uint16))
    assert torch.equal(qg, qn)


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("n,k,group", [(64, 512, 256), (48, 1536, 512), (256, 1024, 1024), (32, 768, 384)])
def test_coarser_groups_are_read_bit_exact(bits, n, k, group):
    """source formats with a group size that is a multiple of 128 (HQQ Format A, whose packing geometry depends on it; GPTQ int32
    and AWQ int16 with [K / group, N] metadata): repack -> native -> dequantize == the oracle's dequant of the same buffers, bit for
    bit; the standalone HQQ dequant too; GEMV on them within the output tolerance; group 64 is refused."""
    from amq_amd import ops
    from amq_amd.hqq_format import random_hqq
    from amq_amd.quant_linear import HIPQuantLinear
    dev = _dev()
    h = random_hqq(n, k, bits, seed=7 * bits + group, group=group)
    w_ref = hqq_ref.dequantize(h.W_q.numpy(), h.scale.numpy(), h.zero.numpy(), bits, (n, k), group_size=group)
    hd = h.to(dev)
    qn, mn = ops.repack_from_hqq(hd.W_q, hd.scale.reshape(-1), hd.zero.reshape(-1), bits, n, k, group=group)
    w = ops.dequantize(qn, mn, bits, ops.MODE_HQQ, n, k).cpu().numpy()
    assert np.array_equal(w.view(np.uint16), np.asarray(w_ref, np.float16).view(np.uint16))
    w2 = ops.dequantize_hqq(hd.W_q, hd.scale.reshape(-1), hd.zero.reshape(-1), bits, n, k, group=group).cpu().numpy()
    assert np.array_equal(w2.view(np.uint16), np.asarray(w_ref, np.float16).view(np.uint16))
    x = torch.randn(2, k, generator=torch.Generator().manual_seed(1)).to(torch.float16)
    mod = HIPQuantLinear.from_hqq(h, device=dev)
    assert mod.group_size == group
    _assert_close(mod(x.to(dev)).cpu().numpy(), linear_ref.linear_f16(x.numpy(), w_ref), f"group {group}")
    # GPTQ int32 buffers of the same layer (the reference's own pack from W_deq + meta), then through the module
    s_ng = h.scale.numpy().reshape(n, k // group)
    z_ng = h.zero.numpy().reshape(n, k // group)
    qweight, scales, zeros = gptq_ref.pack(np.asarray(w_ref, np.float16), s_ng, z_ng, bits, group_size=group)
    want = gptq_ref.dequant_kernel(qweight, scales, zeros, bits, group_size=group)        # [N, K] fp16, the kernels' fma arithmetic
    m2 = HIPQuantLinear.from_gptq_buffers(torch.from_numpy(qweight).to(dev), torch.from_numpy(scales).to(dev),
                                          torch.from_numpy(zeros).to(dev), bits)
    assert m2.group_size == group
    got = ops.dequantize(m2.qweight, m2.meta, bits, ops.MODE_FMA, n, k).cpu().numpy()
    assert np.array_equal(got.view(np.uint16), np.asarray(want, np.float16).view(np.uint16))
    if bits == 4 and n % 4 == 0 and k % 64 == 0:
        qw, sc, szr = awq_ref.pack(np.asarray(w_ref, np.float16), s_ng, z_ng, group_size=group)
        want = awq_ref.dequant_kernel(qw, sc, szr, group_size=group)
        m3 = HIPQuantLinear.from_ft_buffers(torch.from_numpy(qw).to(dev), torch.from_numpy(sc).to(dev), torch.from_numpy(szr).to(dev))
        got = ops.dequantize(m3.qweight, m3.meta, 4, ops.MODE_FMA, n, k).cpu().numpy()
        assert np.array_equal(got.view(np.uint16), np.asarray(want, np.float16).view(np.uint16))
    with pytest.raises(ValueError):
        ops.repack_from_hqq(hd.W_q, hd.scale.reshape(-1), hd.zero.reshape(-1), bits, n, k, group=96)


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("n,k", [(64, 512), (4096, 4096), (1024, 11008)])
def test_fma1_mode_is_the_fma_mode_bit_for_bit(bits, n, k):
    """AMQ_MODE_FMA1 (reference-format buffers whose scales are within amq_fma1_scale_bound: the GEMV kernel unpacks a pair with ONE packed fma)
    gives the bits of AMQ_MODE_FMA on every kernel: GEMV (1 / 3 rows, bias, RMSNorm and SiLU-mul prologues, residual), GEMM, dequantize; the
    module constructors choose it from the scales, and a layer with one scale past the bound keeps AMQ_MODE_FMA"""
    from amq_amd import ops, _lib
    from amq_amd.hqq_format import random_hqq
    from amq_amd.quant_linear import HIPQuantLinear
    dev = _dev()
    h = random_hqq(n, k, bits, seed=5 * bits + 1, bias=True)
    w_ref = np.asarray(hqq_ref.dequantize(h.W_q.numpy(), h.scale.numpy(), h.zero.numpy(), bits, (n, k)), np.float16)
    s_ng, z_ng = h.scale.numpy().reshape(n, k // 128), h.zero.numpy().reshape(n, k // 128)
    qweight, scales, zeros = gptq_ref.pack(w_ref, s_ng, z_ng, bits)
    qn, mn = ops.repack_from_gptq(torch.from_numpy(qweight).to(dev), torch.from_numpy(scales).to(dev), torch.from_numpy(zeros).to(dev), bits, n, k)
    bound = float(_lib.load().amq_fma1_scale_bound(bits))
    assert abs(bound - 65504.0 / (2 ** 18 if bits == 4 else 2 ** 20)) < 1e-9
    assert ops.fma_mode_for(mn, bits) == ops.MODE_FMA1                     # (synthetic scales ~ 1e-2)
    gen = torch.Generator().manual_seed(2)
    bias = h.bias.to(dev)
    for m in (1, 3):
        x = torch.randn(m, k, generator=gen).to(torch.float16).to(dev)
        assert torch.equal(ops.gemv(x, qn, mn, bits, ops.MODE_FMA1, n, k, bias=bias), ops.gemv(x, qn, mn, bits, ops.MODE_FMA, n, k, bias=bias))
    x = torch.randn(2, k, generator=gen).to(torch.float16).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(k, generator=gen)).to(torch.float16).to(dev)
    res = torch.randn(2, n, generator=gen).to(torch.float16).to(dev)
    outs = []
    for mode in (ops.MODE_FMA1, ops.MODE_FMA):
        y0, y1 = torch.empty(2, n, dtype=torch.float16, device=dev), torch.empty(2, n, dtype=torch.float16, device=dev)
        ops.gemv_grouped(x, [dict(qn=qn, mn=mn, bits=bits, mode=mode, N=n, y=y0, residual=res), dict(qn=qn, mn=mn, bits=bits, mode=mode, N=n, y=y1)], k,
                         prologue=ops.PRO_RMSNORM, gamma=gamma, eps=1e-5)
        y2 = torch.empty(2, n, dtype=torch.float16, device=dev)
        ops.gemv_grouped(x, [dict(qn=qn, mn=mn, bits=bits, mode=mode, N=n, y=y2)], k, prologue=ops.PRO_SILU_MUL, x2=gamma.expand(2, k).contiguous())
        outs.append((y0, y1, y2))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    # mixed segments of one launch: FMA1 beside HQQ
    hq = h.to(dev)
    qh, mh = ops.repack_from_hqq(hq.W_q, hq.scale.reshape(-1), hq.zero.reshape(-1), bits, n, k)
    ya, yb = torch.empty(2, n, dtype=torch.float16, device=dev), torch.empty(2, n, dtype=torch.float16, device=dev)
    ops.gemv_grouped(x, [dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_FMA1, N=n, y=ya), dict(qn=qh, mn=mh, bits=bits, mode=ops.MODE_HQQ, N=n, y=yb)], k)
    assert torch.equal(ya, ops.gemv(x, qn, mn, bits, ops.MODE_FMA, n, k)) and torch.equal(yb, ops.gemv(x, qh, mh, bits, ops.MODE_HQQ, n, k))
    # the other kernels treat it as MODE_FMA
    xm = torch.randn(40, k, generator=gen).to(torch.float16).to(dev)
    assert torch.equal(ops.gemm(xm, qn, mn, bits, ops.MODE_FMA1, n, k), ops.gemm(xm, qn, mn, bits, ops.MODE_FMA, n, k))
    assert torch.equal(ops.dequantize(qn, mn, bits, ops.MODE_FMA1, n, k), ops.dequantize(qn, mn, bits, ops.MODE_FMA, n, k))
    # module constructors
    mod = HIPQuantLinear.from_gptq_buffers(torch.from_numpy(qweight).to(dev), torch.from_numpy(scales).to(dev), torch.from_numpy(zeros).to(dev), bits)
    assert mod.mode == ops.MODE_FMA1 and torch.equal(mod(x), ops.linear(x, qn, mn, bits, ops.MODE_FMA, n, k))     # (same dispatch: GEMV, or the few-row GEMM for long rows)
    m2 = HIPQuantLinear(bits, 128, k, n).to(dev)
    m2.load_state_dict(mod.state_dict())
    assert m2.mode == ops.MODE_FMA1 and torch.equal(m2(x), mod(x))
    big = scales.copy()
    big[0, 0] = 2.0 * bound                                               # one scale past the bound: the two-op form for the whole layer
    mod3 = HIPQuantLinear.from_gptq_buffers(torch.from_numpy(qweight).to(dev), torch.from_numpy(big).to(dev), torch.from_numpy(zeros).to(dev), bits)
    assert mod3.mode == ops.MODE_FMA
    want = np.asarray(gptq_ref.dequant_kernel(qweight, big, zeros, bits), np.float16)
    assert np.array_equal(mod3.dequantize().cpu().numpy().view(np.uint16), want.view(np.uint16))
    _assert_close(mod3(x).cpu().numpy(), linear_ref.linear_f16(x.cpu().numpy(), want), "past the bound")


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("group", [64, 32])
@pytest.mark.parametrize("n,k", [(16, 128), (64, 512), (48, 1536), (272, 384), (4096, 4096), (1024, 11008)])
def test_finer_groups(bits, group, n, k):
    """groups of 64 / 32 (128 / group (scale, zero) pairs per native tile row): repack from all three source formats -> dequantize == the
    oracle's dequant of the same buffers, bit for bit; the standalone HQQ dequant too; the GEMV kernel (1 / 3 / 16 rows, bias, the fused
    RMSNorm and SiLU-mul prologues, residual, grouped segments), the few-row GEMM (17 / 100 rows) and the dequantize-once GEMM (300 rows; bias /
    residual / gate) within the output tolerance; the module; entry points that read one pair per tile refuse them"""
    from amq_amd import ops
    from amq_amd.hqq_format import random_hqq
    from amq_amd.quant_linear import HIPQuantLinear
    dev = _dev()
    h = random_hqq(n, k, bits, seed=11 * bits + group, group=group, bias=True)
    w_ref = np.asarray(hqq_ref.dequantize(h.W_q.numpy(), h.scale.numpy(), h.zero.numpy(), bits, (n, k), group_size=group), np.float16)
    hd = h.to(dev)
    qn, mn = ops.repack_from_hqq(hd.W_q, hd.scale.reshape(-1), hd.zero.reshape(-1), bits, n, k, group=group)
    assert mn.numel() == n * k // group * 2
    w = ops.dequantize(qn, mn, bits, ops.MODE_HQQ, n, k).cpu().numpy()
    assert np.array_equal(w.view(np.uint16), w_ref.view(np.uint16))
    w2 = ops.dequantize_hqq(hd.W_q, hd.scale.reshape(-1), hd.zero.reshape(-1), bits, n, k, group=group).cpu().numpy()
    assert np.array_equal(w2.view(np.uint16), w_ref.view(np.uint16))
    gen = torch.Generator().manual_seed(3)
    bias = h.bias
    for m in (1, 3, min(16, ops.gemv_max_rows(k))):            # (the kernel stages its x rows in LDS: fewer than 16 for long rows)
        x = torch.randn(m, k, generator=gen).to(torch.float16)
        y = ops.gemv(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias.to(dev)).cpu().numpy()
        _assert_close_biased(y, linear_ref.linear_f16(x.numpy(), w_ref, bias.numpy()), f"gemv M={m}, group {group}")
    # prologues + residual + two segments of one launch (the second: the same weights again)
    x = torch.randn(2, k, generator=gen).to(torch.float16)
    gamma = (1.0 + 0.1 * torch.randn(k, generator=gen)).to(torch.float16)
    res = torch.randn(2, n, generator=gen).to(torch.float16)
    y0, y1 = torch.empty(2, n, dtype=torch.float16, device=dev), torch.empty(2, n, dtype=torch.float16, device=dev)
    ops.gemv_grouped(x.to(dev), [dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=n, y=y0, residual=res.to(dev)),
                                 dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=n, y=y1)], k,
                     prologue=ops.PRO_RMSNORM, gamma=gamma.to(dev), eps=1e-5)
    xn = ops.rmsnorm(x.to(dev), gamma.to(dev), 1e-5).cpu()
    want = linear_ref.linear_f16(xn.numpy(), w_ref)
    _assert_close(y1.cpu().numpy(), want, f"rmsnorm prologue, group {group}")
    _assert_close(y0.cpu().numpy(), (res.float() + torch.from_numpy(np.asarray(want, np.float16)).float()).to(torch.float16).numpy(), f"residual, group {group}")
    up = torch.randn(2, k, generator=gen).to(torch.float16)
    y2 = torch.empty(2, n, dtype=torch.float16, device=dev)
    ops.gemv_grouped(x.to(dev), [dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=n, y=y2)], k, prologue=ops.PRO_SILU_MUL, x2=up.to(dev))
    act = ops.silu_mul(x.to(dev).reshape(-1), up.to(dev).reshape(-1)).reshape(2, k).cpu()
    _assert_close(y2.cpu().numpy(), linear_ref.linear_f16(act.numpy(), w_ref), f"silu-mul prologue, group {group}")
    # more rows: the pair-aware few-row kernel up to 256 rows (grid.y blocks of 64), the pair-aware tiled kernel beyond it; dequantize once +
    # the fp16 GEMM (forced here) is what AUTO takes once a launch fills 256 x 256 tiles
    for m in (17, 100, 300):
        x = torch.randn(m, k, generator=gen).to(torch.float16)
        y0 = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k)
        _assert_close(y0.cpu().numpy(), linear_ref.linear_f16(x.numpy(), w_ref), f"gemm M={m}, group {group}")
        y = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias.to(dev))
        assert torch.equal(y, y0 + bias.to(dev))                   # fp16(x . W^T), then the bias as a separate fp16 add (the unfused reference's roundings)
        yd = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias.to(dev), route=ops.GEMM_DEQ)
        # AUTO: the pair-aware few-row kernel up to 256 rows, the pair-aware tiled kernel beyond (until the launch fills 256 x 256 tiles: dequantize-once);
        # same weights as the dequantize-once route, another summation order
        yd0 = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, route=ops.GEMM_DEQ)
        _assert_close(yd0.cpu().numpy(), linear_ref.linear_f16(x.numpy(), w_ref), f"gemm DEQ M={m}, group {group}")
        assert torch.equal(yd, yd0 + bias.to(dev))
        assert torch.equal(y, ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias.to(dev), route=ops.GEMM_SKINNY if m <= 256 else ops.GEMM_TILED))
        r = torch.randn(m, n, generator=gen).to(torch.float16)
        yr = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias.to(dev), residual=r.to(dev))
        assert torch.equal(yr.cpu(), (r.float() + torch.from_numpy(y.cpu().numpy()).float()).to(torch.float16))
        if n % 8 == 0:
            g = torch.randn(m, n, generator=gen).to(torch.float16)
            yg = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, gate=g.to(dev))
            up_ = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k)
            assert torch.equal(yg.reshape(-1), ops.silu_mul(g.to(dev).reshape(-1), up_.reshape(-1)))
        with pytest.raises(Exception, match="dequantize-once"):
            ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, route=ops.GEMM_RING)
    if n * 2048 >= 128 * 65536:                                     # a launch that fills 256 x 256 tiles: AUTO is the dequantize-once route
        x = torch.randn(2048, k, generator=gen).to(torch.float16).to(dev)
        ya = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k)
        assert torch.equal(ya, ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, route=ops.GEMM_DEQ))
        ref = x.float() @ torch.from_numpy(w_ref).to(dev).float().t()
        assert ((ya.float() - ref).abs() <= 2.0 ** -9 * ref.abs() + 2e-3 * ref.pow(2).mean().sqrt()).all()
    # the module (plain forwards: GEMV kernel / few-row GEMM), state_dict round trip
    mod = HIPQuantLinear.from_hqq(h, device=dev)
    assert mod.group_size == group and mod.native_group == group
    for m in (1, 5, 40):
        x = torch.randn(m, k, generator=gen).to(torch.float16)
        _assert_close_biased(mod(x.to(dev)).cpu().numpy(), linear_ref.linear_f16(x.numpy(), w_ref, bias.numpy()), f"module M={m}, group {group}")
    m2 = HIPQuantLinear(bits, group, k, n, bias=True).to(dev)
    m2.load_state_dict(mod.state_dict())
    assert torch.equal(m2(x.to(dev)), mod(x.to(dev)))
    # GPTQ int32 / AWQ int16 buffers of the same layer
    s_ng, z_ng = h.scale.numpy().reshape(n, k // group), h.zero.numpy().reshape(n, k // group)
    qweight, scales, zeros = gptq_ref.pack(w_ref, s_ng, z_ng, bits, group_size=group)
    want = np.asarray(gptq_ref.dequant_kernel(qweight, scales, zeros, bits, group_size=group), np.float16)
    m3 = HIPQuantLinear.from_gptq_buffers(torch.from_numpy(qweight).to(dev), torch.from_numpy(scales).to(dev), torch.from_numpy(zeros).to(dev), bits)
    assert m3.group_size == group
    got = ops.dequantize(m3.qweight, m3.meta, bits, ops.MODE_FMA, n, k).cpu().numpy()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    x = torch.randn(2, k, generator=gen).to(torch.float16)
    _assert_close(m3(x.to(dev)).cpu().numpy(), linear_ref.linear_f16(x.numpy(), want), f"gptq module, group {group}")
    if bits == 4 and n % 4 == 0 and k % 64 == 0:
        qw, sc, szr = awq_ref.pack(w_ref, s_ng, z_ng, group_size=group)
        want = np.asarray(awq_ref.dequant_kernel(qw, sc, szr, group_size=group), np.float16)
        m4 = HIPQuantLinear.from_ft_buffers(torch.from_numpy(qw).to(dev), torch.from_numpy(sc).to(dev), torch.from_numpy(szr).to(dev))
        got = ops.dequantize(m4.qweight, m4.meta, 4, ops.MODE_FMA, n, k).cpu().numpy()
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    # entry points that read one pair per tile
    with pytest.raises(ValueError, match="groups of 128"):
        ops.gemm_xfrag_grouped(torch.empty(64 * k, dtype=torch.float16, device=dev), 17,
                               [dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=n, y=torch.empty(17, n, dtype=torch.float16, device=dev))], k)
    with pytest.raises(Exception, match="default form"):
        ops.gemv(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, opts=ops.GemvOpts(math=ops.MATH_LINEAR))


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("n,k", [(16, 128), (48, 384), (256, 1024), (1024, 4096), (4096, 11008)])
def test_random_dequant_bit_exact(bits, n, k):
    from amq_amd import ops
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=100 + bits)
    w = ops.dequantize(qn, mn, bits, ops.MODE_HQQ, n, k).cpu().numpy()
    assert np.array_equal(w.view(np.uint16), w_ref.view(np.uint16))


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_integer_roundtrip_all_codes(bits):
    """scale = 1, zero = 0 makes dequantize return the integers themselves:
    checks every code value through repack + unpack, bit-exact."""
    from amq_amd import ops
    from amq_amd.hqq_format import HQQWeights, pack_rows
    n, k = 64, 512
    r = n * k // 128
    q = (torch.arange(r * 128, dtype=torch.int64) * 2654435761 % (2 ** bits)).reshape(r, 128).to(torch.int32)
    h = HQQWeights(pack_rows(q, bits), torch.ones(r, 1, dtype=torch.float16), torch.zeros(r, 1, dtype=torch.float16), bits, (n, k)).to(_dev())
    qn, mn = ops.repack_from_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, n, k)
    w = ops.dequantize(qn, mn, bits, ops.MODE_HQQ, n, k).cpu()
    assert torch.equal(w.to(torch.int32), q.reshape(n, k))


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("n,k,m", [(16, 128, 1), (256, 1024, 1), (4096, 4096, 1), (1024, 8192, 1), (4096, 11008, 1),
                                    (11008, 4096, 1), (256, 1024, 2), (4096, 4096, 4), (4096, 4096, 7), (512, 2048, 8), (512, 1024, 16)])
def test_gemv_random(bits, n, k, m):
    from amq_amd import ops
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=7 * bits + m, bias=(m == 4))
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(n + k + m)).to(torch.float16)
    bias = None if h.bias is None else h.bias.to(_dev())
    y = ops.gemv(x.to(_dev()), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias).cpu().numpy()
    y_ref = linear_ref.linear_f16(x.numpy(), w_ref, None if h.bias is None else h.bias.numpy())
    _assert_close(y, y_ref, f"gemv {bits}b {n}x{k} M={m}")
    # and against an fp64-accumulated product of the same fp16 weights: the
    # kernel's own error (fp32 accumulate + one fp16 rounding) stays at fp16 rounding level
    if h.bias is None:
        y64 = linear_ref.matmul_f64(x.numpy(), w_ref.T)
        scale = np.sqrt(np.mean(y64 ** 2))
        assert np.max(np.abs(y.astype(np.float64) - y64) - 2.0 ** -10 * np.abs(y64)) <= 2e-3 * scale * 2.0 ** -3
    # an explicit AMQ_MATH_EXACT is the default arithmetic of this build
    if ops.default_gemv_math() == ops.MATH_EXACT:
        y_ex = ops.gemv(x.to(_dev()), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, opts=ops.GemvOpts(math=ops.MATH_EXACT)).cpu().numpy()
        assert np.array_equal(y_ex.view(np.uint16), y.view(np.uint16))


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("n,k,m", [(256, 1024, 1), (4096, 4096, 1), (4096, 11008, 1), (11008, 4096, 1), (4096, 4096, 4), (4096, 4096, 7), (512, 1024, 16)])
def test_gemv_groupscale_math(bits, n, k, m):
    """opt-in AMQ_MATH_GROUPSCALE: the first of the reference's two fp16 roundings per weight is taken exactly, the scale is applied once per
    (row, group) in fp32 after the tile's MFMAs -- the second rounding (<= 2^-11 relative per weight) is not taken.  Measured distance from the
    oracle (profiles/r05_gemv_groupscale.txt): rms 3.2e-4 of rms(y) (half of it the interplay with y's own fp16 rounding), worst element 0.93 of
    the parity bar over 27 layer cases -- and with a bias, whose separate fp16 add rounds a second time, a few elements per 10^4 land 2 ulps
    off, beyond the bar: why this arithmetic is opt-in and not the default.  Bounds asserted here: 2 fp16 ulps + 1e-3 rms per element,
    4e-4 rms overall, and a mean error (the dropped roundings are zero-mean) below 1e-4 rms."""
    from amq_amd import ops
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=7 * bits + m, bias=(m == 4))
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(n + k + m)).to(torch.float16)
    bias = None if h.bias is None else h.bias.to(_dev())
    y = ops.gemv(x.to(_dev()), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, opts=ops.GemvOpts(math=ops.MATH_GROUPSCALE)).cpu().numpy()
    y_ref = linear_ref.linear_f16(x.numpy(), w_ref, None if h.bias is None else h.bias.numpy()).astype(np.float64)
    rms = float(np.sqrt(np.mean(y_ref ** 2)))
    err = y.astype(np.float64) - y_ref
    assert np.all(np.abs(err) <= 2.0 ** -9 * np.abs(y_ref) + 1e-3 * rms), np.abs(err).max()
    assert np.sqrt(np.mean(err ** 2)) <= 4e-4 * rms
    assert abs(np.mean(err)) <= 1e-4 * rms
    # segments whose dequant has ONE rounding by definition (reference-format buffers) run their exact bodies under this option: same bits
    mn_f = mn.clone()
    mt = mn_f.view(-1, 2)
    mt[:, 1] = (-(mt[:, 1].float() * mt[:, 0].float())).to(torch.float16)
    y_f = ops.gemv(x.to(_dev()), qn, mn_f, bits, ops.MODE_FMA, n, k, bias=bias)
    y_fg = ops.gemv(x.to(_dev()), qn, mn_f, bits, ops.MODE_FMA, n, k, bias=bias, opts=ops.GemvOpts(math=ops.MATH_GROUPSCALE))
    assert torch.equal(y_f, y_fg)


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("n,k,m", [(128, 256, 9), (256, 1024, 64), (384, 512, 65), (1024, 4096, 128), (1024, 4096, 300), (176, 384, 130)])
def test_gemm_random(bits, n, k, m):
    from amq_amd import ops
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=31 * bits + m, bias=(m == 64))
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(n + k + m)).to(torch.float16)
    bias = None if h.bias is None else h.bias.to(_dev())
    y = ops.gemm(x.to(_dev()), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias).cpu().numpy()
    y_ref = linear_ref.linear_f16(x.numpy(), w_ref, None if h.bias is None else h.bias.numpy())
    _assert_close(y, y_ref, f"gemm {bits}b {n}x{k} M={m}")
    # reference-style dispatch goes through the same kernels
    y2 = ops.linear(x.to(_dev()).reshape(1, m, k), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias)
    assert y2.shape == (1, m, n)
    assert np.array_equal(y2.reshape(m, n).cpu().numpy().view(np.uint16), y.view(np.uint16))


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_matmul_weights_equal_oracle_weights(bits):
    """x = I makes y = W^T: recovers the weights exactly as the matmul kernels
    see them (fast scaled-subnormal unpack).  They must equal the reference's
    two-rounding dequant bit for bit, except where |zero| or |q - zero| is
    below 2^-9 (an intermediate is an fp16 subnormal there).  Where |q - zero|
    is, they may differ by <= 2^-19 * scale; where only |zero| is, by one fp16
    ulp of (q - zero) times scale when q - zero sits next to a rounding tie
    (tests/metadomain_ref.py derives it) -- THESE inputs meet no such tie, so
    the 2^-19 * scale asserted below holds for them.  The general statement,
    every kernel family and the whole fp16 range of scale / zero:
    tests/test_gpu_metadomain.py."""
    from amq_amd import ops
    from amq_amd.hqq_format import HQQWeights, pack_rows
    n, k = 256, 512
    r = n * k // 128
    gen = torch.Generator().manual_seed(bits)
    q = torch.randint(0, 2 ** bits, (r, 128), generator=gen, dtype=torch.int32)
    scale = ((torch.rand(r, 1, generator=gen) + 0.5) * 2.7e-3).to(torch.float16)
    zero = (torch.rand(r, 1, generator=gen) * (2 ** bits - 1)).to(torch.float16)
    zero[::5] = torch.round(zero[::5].float()).to(torch.float16)          # integer zeros: q - z == 0 cases
    zero[1::7] = (torch.round(zero[1::7].float()) + 0.01).to(torch.float16)   # |q - z| small
    zero[2::11] = (torch.rand(zero[2::11].shape, generator=gen) * 0.03).to(torch.float16)   # small zero points
    zero[3::13] = (torch.round(zero[3::13].float()) + 3e-4).to(torch.float16)  # |q - z| below 2^-9
    h = HQQWeights(pack_rows(q, bits), scale, zero, bits, (n, k))
    hd = h.to(_dev())
    qn, mn = ops.repack_from_hqq(hd.W_q, hd.scale.reshape(-1), hd.zero.reshape(-1), bits, n, k)
    w_ref = hqq_ref.dequantize(h.W_q.numpy(), scale.numpy(), zero.numpy(), bits, (n, k))
    eye = torch.eye(k, dtype=torch.float16, device=_dev())
    w_mm = ops.gemm(eye, qn, mn, bits, ops.MODE_HQQ, n, k).cpu().numpy().T        # [N, K]
    w_mv = torch.cat([ops.gemv(eye[i:i + 16], qn, mn, bits, ops.MODE_HQQ, n, k, opts=ops.GemvOpts(math=ops.MATH_EXACT))
                      for i in range(0, k, 16)]).cpu().numpy().T
    d = np.abs(q.reshape(n, k).numpy().astype(np.float64) - np.repeat(zero.numpy().astype(np.float64).reshape(n, -1), 128, axis=1))
    s_full = np.repeat(scale.numpy().astype(np.float64).reshape(n, -1), 128, axis=1)
    for w in (w_mm, w_mv):
        same = w.view(np.uint16) == w_ref.view(np.uint16)
        same |= (w == 0) & (w_ref == 0)                                           # +0 / -0
        zabs = np.repeat(np.abs(zero.numpy().astype(np.float64)).reshape(n, -1), 128, axis=1)
        safe = (d >= 2.0 ** -9) & (zabs >= 2.0 ** -9)
        assert same[safe].all()
        err = np.abs(w.astype(np.float64) - w_ref.astype(np.float64))
        assert np.all(err[~same] <= np.maximum(2.0 ** -19 * s_full[~same], 2.0 ** -24) * 1.0001)   # 2^-24: one fp16 subnormal ulp
    # the default (group-scale) arithmetic takes the FIRST rounding exactly like the oracle, d = fp16((q - z) 2^-9), and applies the scale
    # to the fp32 sum: with x = I the sum is one product, d * s exactly, and its single rounding to fp16 IS the oracle's second rounding --
    # the same weights bit for bit wherever (q - z) 2^-9 and z 2^-9 are normal halves (|q - z|, |z| >= 2^-5); below that, z or q - z is
    # taken to a multiple of 2^-15 first: 2^-16 of a step off, which at worst moves the first rounding by one fp16 ulp of (q - z)
    w_gs = torch.cat([ops.gemv(eye[i:i + 16], qn, mn, bits, ops.MODE_HQQ, n, k, opts=ops.GemvOpts(math=ops.MATH_GROUPSCALE))
                      for i in range(0, k, 16)]).cpu().numpy().T
    same = (w_gs.view(np.uint16) == w_ref.view(np.uint16)) | ((w_gs == 0) & (w_ref == 0))
    safe = (d >= 2.0 ** -5) & (zabs >= 2.0 ** -5)
    assert same[safe].all()
    err = np.abs(w_gs.astype(np.float64) - w_ref.astype(np.float64))
    assert np.all(err[~same] <= np.maximum((2.0 ** -9 * d[~same] + 2.0 ** -15) * s_full[~same], 2.0 ** -24) * 1.0001)
    assert (~same).mean() < 0.02


@pytest.mark.parametrize("opt", ["dot", "w4", "w8", "w16"])
def test_gemv_variants_agree(opt):
    """the A/B knobs (dot-product body, waves per workgroup) change scheduling, not results beyond fp32 summation order"""
    from amq_amd import ops
    h, qn, mn, w_ref = _random_case(3, 1024, 4096, seed=9)
    x = torch.randn(1, 4096, generator=torch.Generator().manual_seed(1)).to(torch.float16)
    y_ref = linear_ref.linear_f16(x.numpy(), w_ref)
    o = ops.GemvOpts(dot=1) if opt == "dot" else ops.GemvOpts(waves=int(opt[1:]))      # per-call options: no library state
    y = ops.gemv(x.to(_dev()), qn, mn, 3, ops.MODE_HQQ, 1024, 4096, opts=o).cpu().numpy()
    _assert_close(y, y_ref, f"gemv variant {opt}")


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("n,k,m,rpt", [(256, 1024, 1, 0), (4096, 4096, 1, 3), (512, 2048, 5, 2), (11008, 4096, 1, 0), (64, 384, 3, 0)])
def test_gemv_linear_math_and_persistent_rows(bits, n, k, m, rpt):
    """opt-in AMQ_MATH_LINEAR (scale/zero applied per group in fp32, no per-weight fp16 rounding) and
    several row-tiles per workgroup.  Linear math is compared (a) with the exact real-valued dequant
    sum_k x_k * (q_k - z) * s in fp64: fp32-accumulation accuracy; (b) with the reference's rounded-weight
    result: within 2e-3 of the output rms (the reference's own weight-rounding noise is ~3e-4 rms)."""
    from amq_amd import ops
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=11 * bits + m)
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(n + m)).to(torch.float16)
    q = hqq_ref.unpack(h.W_q.numpy(), bits, (n, k)).astype(np.float64)
    s64 = np.repeat(h.scale.numpy().astype(np.float64).reshape(n, -1), 128, axis=1)
    z64 = np.repeat(h.zero.numpy().astype(np.float64).reshape(n, -1), 128, axis=1)
    y_real = x.numpy().astype(np.float64) @ ((q - z64) * s64).T
    y_ref = linear_ref.linear_f16(x.numpy(), w_ref).astype(np.float64)
    rms = np.sqrt(np.mean(y_ref ** 2))
    y_exact = ops.gemv(x.to(_dev()), qn, mn, bits, ops.MODE_HQQ, n, k, opts=ops.GemvOpts(rpt=rpt)).cpu().numpy()
    y_lin = ops.gemv(x.to(_dev()), qn, mn, bits, ops.MODE_HQQ, n, k,
                     opts=ops.GemvOpts(rpt=rpt, math=ops.MATH_LINEAR)).cpu().numpy().astype(np.float64)
    # options are per call: a default launch afterwards is the exact-math one again
    assert np.array_equal(ops.gemv(x.to(_dev()), qn, mn, bits, ops.MODE_HQQ, n, k, opts=ops.GemvOpts(rpt=rpt)).cpu().numpy(), y_exact)
    _assert_close(y_exact, y_ref, "exact math, rpt=%d" % rpt)
    assert np.max(np.abs(y_lin - y_real) - 2.0 ** -10 * np.abs(y_real)) <= 1e-4 * rms      # (a)
    assert np.max(np.abs(y_lin - y_ref) - 2.0 ** -10 * np.abs(y_ref)) <= 2e-3 * rms   # (b) (+ one fp16 ulp of y: both are rounded)
    assert np.sqrt(np.mean((y_lin - y_ref) ** 2)) <= 6e-4 * rms


def test_gemv_is_deterministic():
    from amq_amd import ops
    h, qn, mn, _ = _random_case(3, 4096, 4096, seed=5)
    x = torch.randn(1, 4096).to(torch.float16).to(_dev())
    y0 = ops.gemv(x, qn, mn, 3, ops.MODE_HQQ, 4096, 4096)
    for _ in range(5):
        assert torch.equal(ops.gemv(x, qn, mn, 3, ops.MODE_HQQ, 4096, 4096), y0)


def _rmsnorm_ref(x, gamma, eps):
    xf = x.float()
    h = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(torch.float16)
    return gamma * h


@pytest.mark.parametrize("m", [1, 3])
def test_grouped_mixed_bits_with_prologues(m):
    """q/k/v-style launch: three segments of different bit-widths sharing a
    RMSNorm'ed x; then a SiLU*mul prologue with residual epilogue."""
    from amq_amd import ops
    k = 1024
    specs = [(4, 512), (2, 256), (3, 384)]
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(m, k, generator=gen).to(torch.float16)
    gamma = (1.0 + 0.1 * torch.randn(k, generator=gen)).to(torch.float16)
    eps = 1e-5
    xn = _rmsnorm_ref(x, gamma, eps)
    segs, refs = [], []
    for i, (bits, n) in enumerate(specs):
        h, qn, mn, w_ref = _random_case(bits, n, k, seed=50 + i)
        y = torch.empty(m, n, dtype=torch.float16, device=_dev())
        segs.append(dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=n, y=y))
        refs.append(linear_ref.linear_f16(xn.numpy(), w_ref))
    ops.gemv_grouped(x.to(_dev()), segs, k, prologue=ops.PRO_RMSNORM, gamma=gamma.to(_dev()), eps=eps)
    for s, r in zip(segs, refs):
        _assert_close(s["y"].cpu().numpy(), r, "grouped rmsnorm")
    # down_proj-style: x = silu(gate) * up ; y = residual + x W^T
    gate = torch.randn(m, k, generator=gen).to(torch.float16)
    up = torch.randn(m, k, generator=gen).to(torch.float16)
    act = torch.nn.functional.silu(gate.float()).to(torch.float16) * up
    h, qn, mn, w_ref = _random_case(3, 256, k, seed=77)
    res = torch.randn(m, 256, generator=gen).to(torch.float16)
    y = torch.empty(m, 256, dtype=torch.float16, device=_dev())
    ops.gemv_grouped(gate.to(_dev()), [dict(qn=qn, mn=mn, bits=3, mode=ops.MODE_HQQ, N=256, y=y, residual=res.to(_dev()))],
                     k, prologue=ops.PRO_SILU_MUL, x2=up.to(_dev()))
    ref = (res.numpy() + linear_ref.linear_f16(act.numpy(), w_ref)).astype(np.float16)
    _assert_close(y.cpu().numpy(), ref, "silu*mul + residual")


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("m,k,n", [(2, 4096, 512), (4, 4096, 512), (5, 4096, 256), (8, 4096, 256), (3, 11008, 256), (6, 11008, 256),
                                     (7, 11008, 512), (8, 11008, 4096), (8, 8192, 256)])
def test_gemv_rows_staged_by_dma(bits, m, k, n):
    """launches of 2 .. 8 rows (sequences decoded together): x goes into LDS by LDS-DMA ahead of the weight ring, the fused transform is applied in
    place (kernels RS = 64 / 128); 7 - 8 rows of K = 11008 (the 7B down_proj at batch 7 - 8: 8 x 11008 halves do not fit LDS) stage x in two K
    phases.  Every prologue against the oracle; every row bit-identical to the same row launched alone (a sequence's result does not depend
    on its batch); strided x takes the generic path with the same bits."""
    from amq_amd import ops
    dev = _dev()
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=13 * bits + m)
    gen = torch.Generator().manual_seed(m * 1000 + k)
    x = torch.randn(m, k, generator=gen).to(torch.float16)
    up = torch.randn(m, k, generator=gen).to(torch.float16)
    gamma = (1.0 + 0.1 * torch.randn(k, generator=gen)).to(torch.float16)
    res = torch.randn(m, n, generator=gen).to(torch.float16)
    eps = 1e-5
    seg = lambda y, r=None: [dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=n, y=y, residual=r)]

    def run(xx, pro, **kw):
        y = torch.empty(xx.shape[0], n, dtype=torch.float16, device=dev)
        r = kw.pop("res", None)
        ops.gemv_grouped(xx, seg(y, r), k, prologue=pro, **kw)
        return y

    xd, upd, gd, rd = x.to(dev), up.to(dev), gamma.to(dev), res.to(dev)
    max_rows_norm, max_rows = ops.gemv_max_rows(k, plain=True), ops.gemv_max_rows(k, plain=True, norm=False)
    assert max_rows >= m, (m, k, max_rows)
    # no prologue + residual
    y0 = run(xd, ops.PRO_NONE, res=rd)
    _assert_close(y0.cpu().numpy(), (res.numpy() + linear_ref.linear_f16(x.numpy(), w_ref)).astype(np.float16), "rows, no prologue")
    # SiLU * mul
    act = torch.nn.functional.silu(x.float()).to(torch.float16) * up
    y2 = run(xd, ops.PRO_SILU_MUL, x2=upd)
    _assert_close(y2.cpu().numpy(), linear_ref.linear_f16(act.numpy(), w_ref), "rows, silu*mul")
    # RMSNorm (needs the whole row in LDS: as many rows as fit)
    if m <= max_rows_norm:
        y1 = run(xd, ops.PRO_RMSNORM, gamma=gd, eps=eps)
        _assert_close(y1.cpu().numpy(), linear_ref.linear_f16(_rmsnorm_ref(x, gamma, eps).numpy(), w_ref), "rows, rmsnorm")
    # a row alone == the row in the batch (K phases deal the tiles to the waves differently: same sums in another order, within fp32 rounding)
    # (so does a launch geometry that differs between one row and several: 4096 < K <= 8192 runs 8-wave workgroups at one row, 16-wave at several)
    phased = m > max_rows_norm or 4096 < k <= 8192
    same = (lambda a_, b_: _assert_close(a_.cpu().numpy(), b_.cpu().numpy(), "row alone vs in a phased batch")) if phased else \
           (lambda a_, b_: (_ for _ in ()).throw(AssertionError("row differs from its batch")) if not torch.equal(a_, b_) else None)
    for i in (0, m - 1):
        same(run(xd[i:i + 1], ops.PRO_NONE, res=rd[i:i + 1]), y0[i:i + 1])
        same(run(xd[i:i + 1].contiguous(), ops.PRO_SILU_MUL, x2=upd[i:i + 1].contiguous()), y2[i:i + 1])
        if m <= max_rows_norm:
            same(run(xd[i:i + 1], ops.PRO_RMSNORM, gamma=gd, eps=eps), y1[i:i + 1])
    # deterministic
    assert torch.equal(run(xd, ops.PRO_SILU_MUL, x2=upd), y2)
    # ... also when x comes from HBM (a cache-flushing fill in front of the launch: the LDS-DMA transfers then take microseconds to land, and a wait
    # that does not cover them -- the K-phased restage once used the initial staging's counted wait -- shows as a wrong row-tile)
    junk = torch.empty(320 << 20, dtype=torch.uint8, device=dev)
    for rep in range(4):
        junk.fill_(rep)
        assert torch.equal(run(xd, ops.PRO_NONE, res=rd), y0), "rows path: result changes with x cold"
    del junk


@pytest.mark.parametrize("m,k,ok", [(2, 4096, True), (6, 4096, True), (8, 4096, True), (6, 11008, True), (8, 11008, False), (7, 11008, False)])
def test_gemv_strided_x_through_the_c_abi(m, k, ok):
    """x rows that are not K apart (include/amq_hip.h: x_stride): the row kernels' LDS-DMA staging takes dense rows only, so a strided launch runs
    the generic staging with the same bits -- and where rows would only fit LDS in two K phases (7 - 8 rows of K = 11008), which needs dense rows,
    the call is refused with AMQ_ESHAPE instead of returning AMQ_OK with y unwritten."""
    from amq_amd import ops, _lib
    dev = _dev()
    bits, n = 3, 512
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=3 * m + 1)
    xs = k + 64
    xbuf = torch.randn(m, xs, generator=torch.Generator().manual_seed(m + k)).to(torch.float16).to(dev)
    y = torch.full((m, n), float("nan"), dtype=torch.float16, device=dev)
    lib = _lib.load()
    rc = lib.amq_gemv_f16(bits, ops.MODE_HQQ, _lib.ptr(xbuf), _lib.ptr(qn), _lib.ptr(mn), None, _lib.ptr(y), m, n, k, 128, xs, n, _lib.current_stream())
    if not ok:
        assert rc == -2 and b"strided" in lib.amq_last_error()
        assert torch.isnan(y).all()
        return
    assert rc == 0, lib.amq_last_error()
    xd = xbuf[:, :k].contiguous()
    yd = torch.empty(m, n, dtype=torch.float16, device=dev)
    ops.gemv_grouped(xd, [dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=n, y=yd)], k)
    assert not torch.isnan(y).any()
    _assert_close(y.cpu().numpy(), linear_ref.linear_f16(xd.cpu().numpy(), w_ref), "strided x")
    _assert_close(y.cpu().numpy(), yd.cpu().numpy(), "strided vs dense")


@pytest.mark.parametrize("m", [2, 3, 4, 5, 6, 8])
@pytest.mark.parametrize("k,n_prod", [(4096, 4096), (3584, 3584), (8192, 8192)])
def test_gemv_rmsnorm_from_partial_sums(m, k, n_prod):
    """amq_gemv_grouped_sums_f16 (2 .. 8 sequences): a launch that writes a hidden state leaves one sum of squares per row and 16 output columns
    (sums_out); the launch that normalises it adds them in a fixed order and applies gamma * fp16(x * rstd) while staging x (sums_in) -- against
    the oracle on LlamaRMSNorm's formula, against the unfused pair (amq_rmsnorm_f16 + plain GEMV: same value up to the order of the fp32 mean), and
    bit for bit against itself; grouped consumers of several bit-widths; K = 3584 (224 partials: not a multiple of 64) and 8192 (512: the limit)."""
    from amq_amd import ops
    dev = _dev()
    if m > ops.gemv_max_rows(k, plain=True):
        pytest.skip("rows do not fit LDS whole")
    gen = torch.Generator().manual_seed(m * 100 + k)
    # producer: o_proj-like, ONE segment with a residual: y = res + W1 . a
    h1, q1, m1, w1 = _random_case(3, n_prod, k, seed=m)
    a_in = torch.randn(m, k, generator=gen).to(torch.float16)
    res = torch.randn(m, n_prod, generator=gen).to(torch.float16)
    y1 = torch.empty(m, n_prod, dtype=torch.float16, device=dev)
    ss = torch.full((m, n_prod // 16), float("nan"), dtype=torch.float32, device=dev)
    ops.gemv_grouped_sums(a_in.to(dev), [dict(qn=q1, mn=m1, bits=3, mode=ops.MODE_HQQ, N=n_prod, y=y1, residual=res.to(dev))], k, sums_out=ss)
    y1_plain = torch.empty_like(y1)
    ops.gemv_grouped(a_in.to(dev), [dict(qn=q1, mn=m1, bits=3, mode=ops.MODE_HQQ, N=n_prod, y=y1_plain, residual=res.to(dev))], k)
    assert torch.equal(y1, y1_plain)                                              # the epilogue's extra output changes nothing else
    want_ss = y1.float().pow(2).view(m, n_prod // 16, 16).sum(-1)
    assert not torch.isnan(ss).any() and torch.allclose(ss, want_ss, rtol=1e-5, atol=1e-6)
    # consumer: gate/up-like, two segments of different bit-widths over x = y1 (K of the consumer = N of the producer)
    kc = n_prod
    gamma = (1.0 + 0.1 * torch.randn(kc, generator=gen)).to(torch.float16)
    segs = [(b,) + _random_case(b, nn, kc, seed=7 * b + m)[1:] + (nn,) for b, nn in ((2, 512), (4, 256))]
    eps = 1e-6

    def consumer(sums):
        ys = [torch.empty(m, nn, dtype=torch.float16, device=dev) for *_, nn in segs]
        sg = [dict(qn=q, mn=mt, bits=b, mode=ops.MODE_HQQ, N=nn, y=y) for (b, q, mt, _, nn), y in zip(segs, ys)]
        if sums is not None:
            ops.gemv_grouped_sums(y1, sg, kc, gamma=gamma.to(dev), eps=eps, sums_in=sums)
        else:
            ops.gemv_grouped(ops.rmsnorm(y1, gamma.to(dev), eps), sg, kc)
        return ys
    got = consumer(ss)
    unfused = consumer(None)
    xin = _rmsnorm_ref(y1.cpu(), gamma, eps)
    for (b, q, mt, w_ref, nn), y, yu in zip(segs, got, unfused):
        ref = linear_ref.linear_f16(xin.numpy(), w_ref)
        _assert_close(y.cpu().numpy(), ref, f"partial-sum rmsnorm, {b} bit")
        _assert_close(y.cpu().numpy(), yu.cpu().numpy(), "partial sums vs rmsnorm launch + GEMV")
    again = consumer(ss)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(got, again))
    # what the entry point refuses
    from amq_amd import _lib
    with pytest.raises(_lib.AmqError):
        ops.gemv_grouped_sums(y1[:1], [dict(qn=segs[0][1], mn=segs[0][2], bits=2, mode=ops.MODE_HQQ, N=512, y=got[0][:1])], kc, gamma=gamma.to(dev),
                              eps=eps, sums_in=ss[:1])                               # one row: the fused AMQ_PRO_RMSNORM prologue serves it
    with pytest.raises(_lib.AmqError):
        ops.gemv_grouped_sums(y1, [dict(qn=q, mn=mt, bits=b, mode=ops.MODE_HQQ, N=nn, y=y) for (b, q, mt, _, nn), y in zip(segs, got)], kc,
                              sums_out=torch.empty(m, 512 // 16, dtype=torch.float32, device=dev))      # sums_out describes ONE output


def test_results_do_not_depend_on_cache_state():
    """every kernel that waits for its loads with COUNTED waits (register rings, LDS-DMA pieces) against operands that are cold in HBM: a cache-flushing
    fill in front of each launch makes every transfer take microseconds to land, so a wait that does not cover what the next instruction reads shows
    as a changed result (how the K-phased GEMV's restage wait was caught).  Results must equal the warm run's bit for bit."""
    from amq_amd import ops
    dev = _dev()
    junk = torch.empty(320 << 20, dtype=torch.uint8, device=dev)
    gen = torch.Generator().manual_seed(99)

    def cold(fn, what, reps=3):
        warm = fn()
        for rep in range(reps):
            junk.fill_(rep + 1)
            got = fn()
            assert torch.equal(got, warm), f"{what}: result changes with cold operands"

    # GEMV: one row (register-held x), rows by LDS-DMA with each prologue, generic staging (9 rows, strided)
    k, n = 4096, 2048
    h, qn, mn, w_ref = _random_case(3, n, k, seed=5)
    gamma = (1.0 + 0.1 * torch.randn(k, generator=gen)).to(torch.float16).to(dev)
    for m in (1, 3, 8, 9):
        x = torch.randn(m, k, generator=gen).to(torch.float16).to(dev)
        up = torch.randn(m, k, generator=gen).to(torch.float16).to(dev)

        def gv(pro, **kw):
            y = torch.empty(m, n, dtype=torch.float16, device=dev)
            ops.gemv_grouped(x, [dict(qn=qn, mn=mn, bits=3, mode=ops.MODE_HQQ, N=n, y=y)], k, prologue=pro, **kw)
            return y
        cold(lambda: gv(ops.PRO_NONE), f"gemv {m} rows")
        cold(lambda: gv(ops.PRO_RMSNORM, gamma=gamma, eps=1e-5), f"gemv {m} rows, rmsnorm")
        cold(lambda: gv(ops.PRO_SILU_MUL, x2=up), f"gemv {m} rows, silu*mul")
    # GEMM: every hand-written route
    n2, k2 = 2048, 4096
    h2, qn2, mn2, _ = _random_case(4, n2, k2, seed=6)
    for m, routes in ((64, (ops.GEMM_AUTO, ops.GEMM_SKINNY, ops.GEMM_TILED)), (1024, (ops.GEMM_TILED, ops.GEMM_RING, ops.GEMM_RING128, ops.GEMM_WS, ops.GEMM_DEQ))):
        x = torch.randn(m, k2, generator=gen).to(torch.float16).to(dev)
        for route in routes:
            cold(lambda: ops.gemm(x, qn2, mn2, 4, ops.MODE_HQQ, n2, k2, route=route), f"gemm {m} rows route {route}", reps=2)
    # grouped few-row launch over fragment-ordered x, both forms
    x = torch.randn(64, k2, generator=gen).to(torch.float16).to(dev)
    xf = ops.xfrag(x, 64, k2)
    for form, blocks in ((1, 0), (2, 3), (2, 6)):
        def grouped():
            y = torch.empty(64, n2, dtype=torch.float16, device=dev)
            ops.gemm_xfrag_grouped(xf, 64, [dict(qn=qn2, mn=mn2, bits=4, mode=ops.MODE_HQQ, N=n2, y=y)], k2, form=form, blocks_per_wg=blocks)
            return y
        cold(grouped, f"few-row grouped form {form}/{blocks}", reps=2)
    # dense fp16 GEMM (the dequantize-once route's second half)
    xd = (torch.randn(512, 1024, generator=gen) * 0.5).to(torch.float16).to(dev)
    wd = (torch.randn(768, 1024, generator=gen) * 0.05).to(torch.float16).to(dev)
    cold(lambda: ops.gemm_f16w(xd, wd), "gemm_f16w", reps=2)


def test_error_paths_raise():
    from amq_amd import ops, _lib
    h, qn, mn, _ = _random_case(4, 64, 256, seed=1)
    x = torch.randn(1, 256).to(torch.float16).to(_dev())
    with pytest.raises(ValueError):
        ops.gemv(x.float(), qn, mn, 4, ops.MODE_HQQ, 64, 256)          # wrong dtype
    with pytest.raises(ValueError):
        ops.gemv(x, qn[:-1], mn, 4, ops.MODE_HQQ, 64, 256)             # short buffer
    with pytest.raises(ValueError):
        ops.gemv(x, qn, mn, 5, ops.MODE_HQQ, 64, 256)                  # bits
    with pytest.raises(_lib.AmqError):
        ops.gemv(torch.randn(60, 256).half().to(_dev()), qn, mn, 4, 9, 64, 256)   # bad mode reaches the C ABI


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("m,n,k", [(80, 256, 1024), (128, 512, 4096), (100, 1280, 2048), (96, 4096, 11008)])
def test_gemm_splitk_matches_single_pass(bits, m, n, k):
    """few-row GEMMs take the split-K path (fp32 partial slices + ordered reduce): same result as the dequantized-weight
    matmul, deterministic, and the C entry point rejects a short workspace"""
    import ctypes
    from amq_amd import _lib, ops
    from amq_amd.hqq_format import random_hqq
    dev = torch.device("cuda:0")
    h = random_hqq(n, k, bits, seed=3 * bits + m).to(dev)
    qn, mn = ops.repack_from_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, n, k)
    x = torch.randn(m, k, device=dev, generator=torch.Generator(device=dev).manual_seed(m)).half()
    bias = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(n)).half()
    lib = _lib.load()
    need = lib.amq_gemm_splitk_workspace_bytes(m, n, k)
    assert need > 0, "shape expected to split"
    y = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias)
    w = ops.dequantize(qn, mn, bits, ops.MODE_HQQ, n, k)
    ref = x.float() @ w.float().t()
    rms = ref.pow(2).mean().sqrt()
    yref = (ref.half() + bias).float()
    # y = fp16(fp16(acc) + bias) with acc within fp32-accumulation distance of ref: either rounding may land on the
    # neighbouring fp16 value (one ulp of the product, one ulp of the sum)
    assert torch.all((y.float() - yref).abs() <= 2.0 ** -10 * ref.abs() + 2.0 ** -10 * yref.abs() + 1e-3 * rms)
    assert torch.equal(ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias), y)
    ws = torch.empty(need // 4 - 1, dtype=torch.float32, device=dev)
    rc = lib.amq_gemm_splitk_f16(bits, ops.MODE_HQQ, _lib.ptr(x), _lib.ptr(qn), _lib.ptr(mn), None, _lib.ptr(y), m, n, k, 128, 0, 0,
                                 _lib.ptr(ws), ws.numel() * 4, _lib.current_stream())
    assert rc != 0 and b"workspace" in lib.amq_last_error()


@pytest.mark.parametrize("bits,m,n,k", [(3, 64, 4096, 4096), (4, 24, 1024, 512), (2, 300, 1536, 1024)])
def test_gemm_residual_epilogue(bits, m, n, k):
    """y = residual + fp16(x . W^T + bias) fused into the GEMM / split-K reduce epilogue is bit-identical to the
    separate add (same two roundings), also when the residual buffer is the output buffer"""
    from amq_amd import ops
    from amq_amd.hqq_format import random_hqq
    dev = torch.device("cuda:0")
    h = random_hqq(n, k, bits, seed=7 * bits + m).to(dev)
    qn, mn = ops.repack_from_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, n, k)
    gen = torch.Generator(device=dev).manual_seed(m + n)
    x = torch.randn(m, k, device=dev, generator=gen).half()
    bias = torch.randn(n, device=dev, generator=gen).half()
    res = torch.randn(m, n, device=dev, generator=gen).half()
    plain = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias)
    fused = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, residual=res)
    assert torch.equal(fused, res + plain)
    inplace = res.clone()
    ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, residual=inplace, out=inplace)
    assert torch.equal(inplace, fused)


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("m,n,k", [(9, 48, 128), (16, 256, 384), (17, 1040, 1024), (33, 512, 4096), (64, 4096, 4096),
                                   (50, 11008, 4096), (64, 4096, 11008), (40, 16400, 256)])
def test_gemm_skinny(bits, m, n, k):
    """few-row GEMMs (9..32 rows by default; 64 forced here) run the barrier-free kernel (waves split K, register ring, cross-wave sum in LDS): checked against the
    oracle linear on the reference's dequantized weights, against the tiled kernel (same fp16 weights, different fp32
    summation order), for determinism, and with bias + residual; K tiles < 4 waves, ragged column-block pairs."""
    from amq_amd import _lib, ops
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=17 * bits + m, bias=True)
    dev = _dev()
    gen = torch.Generator().manual_seed(n + k + m)
    x = torch.randn(m, k, generator=gen).to(torch.float16)
    res = torch.randn(m, n, generator=gen).to(torch.float16)
    bias = h.bias.to(dev)
    lib = _lib.load()
    SK = ops.GEMM_SKINNY                      # the default route takes this kernel up to 32 rows; forced here to cover the 4-block variant too
    assert lib.amq_gemm_route_workspace_bytes(SK, m, n, k) == 0
    y = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, route=SK)
    _assert_close(y.cpu().numpy(), linear_ref.linear_f16(x.numpy(), w_ref, h.bias.numpy()), f"skinny {bits}b {n}x{k} M={m}")
    assert torch.equal(ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, route=SK), y)
    yr = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, residual=res.to(dev), route=SK)
    assert torch.equal(yr, res.to(dev) + y)
    tiled = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, route=ops.GEMM_TILED)
    ref = x.to(dev).float() @ ops.dequantize(qn, mn, bits, ops.MODE_HQQ, n, k).float().t()
    tol = 2.0 ** -9 * ref.abs() + 2.0 ** -9 * y.float().abs() + 1e-3 * ref.pow(2).mean().sqrt()
    assert torch.all((y.float() - tiled.float()).abs() <= tol)


@pytest.mark.parametrize("m,k", [(1, 128), (9, 384), (64, 4096), (65, 1024), (200, 512)])
def test_xfrag_layout(m, k):
    """fragment order = xf[g][kt][mb*4 + t][16*o + r][8] <- x[g*64 + mb*16 + r][kt*128 + 32t + 8o ..+8], rows >= M zero;
    strided sources (an attention output [heads, M, 128]) and the fused RMSNorm writer produce the same image"""
    from amq_amd import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(m + k)
    x = torch.randn(m, k, generator=gen).half().to(dev)
    g, ny = k // 128, (m + 63) // 64
    xp = torch.zeros(ny * 64, k, dtype=torch.float16, device=dev)
    xp[:m] = x
    ref = xp.view(ny, 4, 16, g, 4, 4, 8).permute(0, 3, 1, 4, 5, 2, 6).contiguous().reshape(-1)   # gy, kt, mb, t, o, r, 8
    xf = ops.xfrag(x, m, k)
    assert torch.equal(xf, ref)
    heads = x.view(m, g, 128).transpose(0, 1).contiguous()                                       # [heads, M, 128]
    assert torch.equal(ops.xfrag(heads, m, k, stride_m=heads.stride(1), stride_kt=heads.stride(0)), ref)
    gamma = torch.randn(k, generator=gen).half().to(dev)
    assert torch.equal(ops.rmsnorm_xfrag(x, gamma, 1e-5), ops.xfrag(ops.rmsnorm(x, gamma, 1e-5), m, k))


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("m,n,k", [(9, 48, 128), (64, 4096, 4096), (100, 1040, 1024), (130, 11008, 512), (256, 4096, 1024),
                                   (40, 16400, 256)])
def test_gemm_xfrag(bits, m, n, k):
    """few-row GEMM over fragment-ordered x (1, 2 or 4 column blocks per workgroup by launch size): oracle linear on the
    reference's dequantized weights, determinism, bias + residual (in place)"""
    from amq_amd import ops
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=13 * bits + m, bias=True)
    dev = _dev()
    gen = torch.Generator().manual_seed(n + k + m)
    x = torch.randn(m, k, generator=gen).to(torch.float16)
    res = torch.randn(m, n, generator=gen).to(torch.float16).to(dev)
    bias = h.bias.to(dev)
    xf = ops.xfrag(x.to(dev), m, k)
    y0 = ops.gemm_xfrag(xf, m, qn, mn, bits, ops.MODE_HQQ, n, k)
    _assert_close(y0.cpu().numpy(), linear_ref.linear_f16(x.numpy(), w_ref, None), f"xfrag {bits}b {n}x{k} M={m}")
    y = ops.gemm_xfrag(xf, m, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias)
    assert torch.equal(y, y0 + bias)                       # y = fp16(fp16(acc) + bias), like the other kernels
    assert torch.equal(ops.gemm_xfrag(xf, m, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias), y)
    inplace = res.clone()
    ops.gemm_xfrag(xf, m, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, residual=inplace, out=inplace)
    assert torch.equal(inplace, res + y)
    gate = (3 * torch.randn(m, n, generator=gen)).to(torch.float16).to(dev)
    act = ops.gemm_xfrag(xf, m, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, gate=gate)
    assert torch.equal(act, ops.silu_mul(gate, y))            # the fused epilogue = the separate launch, bit for bit
    gio = gate.clone()
    ops.gemm_xfrag(xf, m, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, gate=gio, out=gio)
    assert torch.equal(gio, act)


@pytest.mark.parametrize("bits,m,n,k", [(3, 1024, 1024, 2048), (4, 1500, 512, 1024), (2, 2048, 1280, 512)])
def test_gemm_library_path_matches_fused_kernel(bits, m, n, k, monkeypatch):
    """opt-in: from ops.LIB_GEMM_ROWS rows `gemm` runs dequantize kernel + library GEMM: same fp16 weights, fp32 accumulation,
    so it agrees with the fused unpack + MFMA kernel to summation-order / rounding-order distance; bias and residual
    (separate and in place) included"""
    from amq_amd import ops
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=5 * bits + m, bias=True)
    dev = _dev()
    gen = torch.Generator().manual_seed(m)
    x = torch.randn(m, k, generator=gen).half().to(dev)
    res = torch.randn(m, n, generator=gen).half().to(dev)
    bias = h.bias.to(dev)
    assert ops.LIB_GEMM_ROWS == 0                           # the product default: hand-written kernels at every size
    monkeypatch.setattr(ops, "LIB_GEMM_ROWS", 1024)
    lib = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k)
    lib_b = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias)
    lib_r = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, residual=res)
    inplace = res.clone()
    ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, residual=inplace, out=inplace)
    assert torch.equal(inplace, lib_r)
    monkeypatch.setattr(ops, "LIB_GEMM_ROWS", 0)
    own = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k)
    own_r = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, residual=res)
    ref = x.float() @ ops.dequantize(qn, mn, bits, ops.MODE_HQQ, n, k).float().t()
    rms = ref.pow(2).mean().sqrt()
    assert torch.all((lib.float() - own.float()).abs() <= 2.0 ** -10 * ref.abs() + 1e-3 * rms)
    _assert_close(lib.cpu().numpy(), linear_ref.linear_f16(x.cpu().numpy(), w_ref, None), f"library path {bits}b M={m}")
    full = ref + bias.float() + res.float()
    for got in (lib_r, own_r):                              # one rounding (library) / three roundings (fused), same target
        assert torch.all((got.float() - full).abs() <= 3 * 2.0 ** -10 * (ref.abs() + bias.float().abs() + res.float().abs()) + 1e-3 * rms)
    assert torch.all((lib_b.float() - (ref + bias.float())).abs() <= 2.0 ** -10 * (ref.abs() + bias.float().abs()) + 1e-3 * rms)


def _sampled_rows_check(y, x, w_dev, rows, what):
    """CPU oracle linear (fp16 x . fp16 W^T in fp32 -> fp16) on a row sample; W = the bit-exact dequantized weights"""
    w = w_dev.cpu().numpy()
    xs = x[rows].cpu().numpy()
    _assert_close(y[rows].cpu().numpy(), linear_ref.linear_f16(xs, w), what)


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("m,n,k,route", [(640, 12288, 512, 1), (2048, 3072, 256, 1), (517, 6144, 384, 1),
                                         (640, 12288, 512, 3), (2048, 3072, 256, 3), (517, 6144, 384, 3), (300, 1040, 1152, 3),
                                         (640, 12288, 512, 4), (517, 6144, 384, 4), (300, 1040, 1152, 4), (129, 2048, 256, 4),
                                         (640, 12288, 512, 5), (517, 6144, 384, 5), (300, 1040, 1152, 5), (129, 2048, 256, 5), (2048, 3072, 128, 5),
                                         (640, 12288, 512, 6), (517, 6144, 384, 6), (300, 1040, 1152, 6), (129, 2048, 256, 6), (2048, 3072, 128, 6),
                                         (2600, 6144, 256, 6)])
def test_gemm_big_tiles(bits, m, n, k, route):
    """the many-row MFMA kernels on shapes that select their LARGE tiles (route 1: gemm_kernel<.,.,128,2> needs
    ceil(M/128) * ceil(N/128) >= 384 workgroups; route 3: the ring kernel, 256-row tiles when they fill the chip; route 4: the
    ring kernel forced to 128-row tiles; route 5: the wave-specialised kernel, amq_gemm_ws.hip, 256 x 128 tiles -- N = 1040 leaves a
    ragged last column tile, K = 128 a single group; route 6: dequantize once + the ping-pong fp16 kernel, amq_gemm_f16.hip, whose
    persistent workgroups walk two tiles each at 2600 x 6144), ragged M tails, bias and an in-place
    residual, against the CPU oracle linear on the reference's dequantized weights."""
    from amq_amd import ops
    h, qn, mn, w_ref = _random_case(bits, n, k, seed=31 * bits + m, bias=True)
    dev = _dev()
    gen = torch.Generator().manual_seed(m + n)
    x = torch.randn(m, k, generator=gen).to(torch.float16)
    res = torch.randn(m, n, generator=gen).to(torch.float16)
    bias = h.bias.to(dev)
    y = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, route=route)
    # the bar is one fp16 rounding of the MATMUL result (1e-3 relative); the bias is then added in fp16 by both sides, so
    # the comparison is made on the un-biased values (with millions of outputs some bias nearly cancels its matmul term)
    y_mm = ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, route=route)
    _assert_close(y_mm.cpu().numpy(), linear_ref.linear_f16(x.numpy(), w_ref), f"route {route} {bits}b {m}x{n}x{k}")
    assert torch.equal(y, y_mm + bias)
    assert torch.equal(ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, route=route), y)     # deterministic
    inplace = res.to(dev).clone()
    ops.gemm(x.to(dev), qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, residual=inplace, out=inplace, route=route)
    assert torch.equal(inplace, res.to(dev) + y)


@pytest.mark.parametrize("m,n,k,bits,bias", [(64, 4096, 11008, 3, False),        # 7B down_proj at the reference protocol's 64 prompt rows: split-K, one launch
                                              (40, 1024, 2816, 4, True),           # ragged last row group (rows 40 .. 63 of the fragments are zeros), bias
                                              (150, 5120, 1024, 2, False),         # three row groups, 2.5 chunks per thread
                                              (64, 8192, 1024, 3, False),          # widest row the fused kernel takes
                                              (64, 8320, 1024, 4, False),          # wider: the two launches
                                              (600, 512, 512, 3, True)])           # no split-K (the rows fill the chip): GEMM, then the norm as its own launch
def test_gemm_splitk_norm_xfrag_equals_two_launches(m, n, k, bits, bias):
    """amq_gemm_res_norm_xfrag_f16 (a split-K GEMM whose reduce launch also takes the RMSNorm of the result rows into fragment order -- down_proj into the
    next block's input norm on a short prompt pass) == amq_gemm_res_f16 followed by amq_rmsnorm_xfrag_f16, bit for bit: y and the fragments."""
    from amq_amd import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(m + n + k)
    x = torch.randn(m, k, generator=gen).to(torch.float16).to(dev)
    res = torch.randn(m, n, generator=gen).to(torch.float16).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(n, generator=gen)).to(torch.float16).to(dev)
    h, qn, mn, _ = _random_case(bits, n, k, seed=7 * bits + n % 13, bias=bias)
    b = h.bias.to(dev) if bias else None
    y_two = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=b, residual=res.clone())
    xf_two = ops.rmsnorm_xfrag(y_two, gamma, 1e-5)
    y_one = res.clone()
    y_ret, xf_one = ops.gemm_res_norm_xfrag(x, qn, mn, bits, ops.MODE_HQQ, n, k, gamma, 1e-5, bias=b, residual=y_one, out=y_one)
    assert y_ret.data_ptr() == y_one.data_ptr()
    assert torch.equal(y_one, y_two)
    assert torch.equal(xf_one, xf_two)
    # no residual, fresh output
    y2, xf2 = ops.gemm_res_norm_xfrag(x, qn, mn, bits, ops.MODE_HQQ, n, k, gamma, 1e-5, bias=b)
    y2_two = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=b)
    assert torch.equal(y2, y2_two) and torch.equal(xf2, ops.rmsnorm_xfrag(y2_two, gamma, 1e-5))
    with pytest.raises(Exception):
        ops.gemm_res_norm_xfrag(x, qn, mn, bits, ops.MODE_HQQ, n, k, gamma[: n - 1], 1e-5)


@pytest.mark.parametrize("m,k,specs", [(64, 1024, [(4, 512), (2, 256), (3, 384)]),            # q/k/v-like, one column block per workgroup
                                       (40, 512, [(3, 4096), (4, 4096)]),                       # 512 blocks: two per workgroup
                                       (200, 768, [(2, 3072), (3, 1040), (4, 2064)]),           # four per workgroup, ragged last groups, 4 row groups
                                       (33, 256, [(4, 16)])])
def test_gemm_xfrag_grouped_equals_single_launches(m, k, specs):
    """several linears over one fragment-ordered x as segments of ONE few-row launch == the same linears launched one by one
    (amq_gemm_xfrag_f16), bit for bit, with bias and an in-place residual on one segment; and == the oracle linear."""
    from amq_amd import ops
    dev = _dev()
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(m + k)).to(torch.float16)
    xf = ops.xfrag(x.to(dev), m, k)
    segs, singles, refs = [], [], []
    for i, (bits, n) in enumerate(specs):
        h, qn, mn, w_ref = _random_case(bits, n, k, seed=100 * i + bits, bias=(i == 0))
        bias = h.bias.to(dev) if i == 0 else None
        res = torch.randn(m, n, generator=torch.Generator().manual_seed(i)).to(torch.float16).to(dev) if i == len(specs) - 1 else None
        y = res.clone() if res is not None else torch.empty(m, n, dtype=torch.float16, device=dev)
        segs.append(dict(qn=qn, mn=mn, bits=bits, mode=ops.MODE_HQQ, N=n, y=y, bias=bias, residual=y if res is not None else None))
        singles.append(ops.gemm_xfrag(xf, m, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, residual=res.clone() if res is not None else None))
        refs.append((w_ref, h.bias.numpy() if i == 0 else None, res))
    ops.gemm_xfrag_grouped(xf, m, segs, k)
    for s, one, (w_ref, b, res) in zip(segs, singles, refs):
        assert torch.equal(s["y"], one)
        if res is None:
            _assert_close(s["y"].cpu().numpy(), linear_ref.linear_f16(x.numpy(), w_ref, b), "grouped few-row segment")
    # every kernel form of the launch gives the same bits: x fragments a K tile at a time, and the streaming form (one MFMA step at a time,
    # amq_gemm_fewrow.hip) at each of its block counts -- ragged last workgroups, segment boundaries inside the grid, several row groups
    from amq_amd import _lib
    for form, blocks in [(_lib.FEWROW_TILE, 0), (_lib.FEWROW_STREAM, 0)] + [(_lib.FEWROW_STREAM, b) for b in (1, 2, 3, 4, 6)]:
        for s, (w_ref, b, res) in zip(segs, refs):
            if res is not None:
                s["y"].copy_(res)                          # (the residual segment accumulates in place)
            else:
                s["y"].zero_()
        ops.gemm_xfrag_grouped(xf, m, segs, k, form=form, blocks_per_wg=blocks)
        for s, one in zip(segs, singles):
            assert torch.equal(s["y"], one), (form, blocks)
    # ... and the one-rounding (reference-format) bodies: the first segment's buffers in MODE_FMA form, streaming form against the single launch
    s0 = segs[0]
    mt = s0["mn"].clone().view(-1, 2)
    mt[:, 1] = -(mt[:, 1] * mt[:, 0])
    fseg = dict(s0, mn=mt.reshape(-1), mode=ops.MODE_FMA, y=torch.empty_like(s0["y"]), residual=None)
    one = ops.gemm_xfrag(xf, m, fseg["qn"], fseg["mn"], fseg["bits"], ops.MODE_FMA, fseg["N"], k, bias=fseg["bias"])
    for blocks in (1, 3, 6):
        fseg["y"].zero_()
        ops.gemm_xfrag_grouped(xf, m, [fseg], k, form=_lib.FEWROW_STREAM, blocks_per_wg=blocks)
        assert torch.equal(fseg["y"], one), blocks


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("m,n,k,route", [(20, 1024, 512, 0), (64, 2048, 256, 2), (300, 1040, 1152, 0), (300, 1040, 1152, 1),
                                         (200, 2048, 4096, 0),                       # tiled kernel + split-K, then the element-wise launch
                                         (2048, 3072, 256, 3), (517, 6144, 384, 4), (2500, 4096, 512, 0), (517, 1040, 384, 5),
                                         (2048, 3072, 256, 6), (517, 1040, 384, 6)])
def test_gemm_gated_equals_separate_silu_mul(bits, m, n, k, route):
    """y = fp16(silu(gate)) * fp16(x . W^T + bias) formed by the GEMM (ring / few-row epilogue, or the element-wise launch
    behind the tiled kernel) == amq_silu_mul_f16 on the separately computed projection, bit for bit; in place on the gate."""
    from amq_amd import ops
    h, qn, mn, _ = _random_case(bits, n, k, seed=17 * bits + m, bias=True)
    dev = _dev()
    gen = torch.Generator().manual_seed(m * 3 + n)
    x = torch.randn(m, k, generator=gen).to(torch.float16).to(dev)
    gate = (torch.randn(m, n, generator=gen) * 2).to(torch.float16).to(dev)
    bias = h.bias.to(dev)
    up = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, route=route)
    want = ops.silu_mul(gate, up)
    got = ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, gate=gate, route=route)
    assert torch.equal(got, want)
    inplace = gate.clone()
    ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, bias=bias, gate=inplace, out=inplace, route=route)
    assert torch.equal(inplace, want)
    with pytest.raises(ValueError):
        ops.gemm(x, qn, mn, bits, ops.MODE_HQQ, n, k, gate=gate, residual=gate)


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("n,k", [(5120, 5120), (13824, 5120), (5120, 13824)])
@pytest.mark.parametrize("m", [512, 2048, 8192])
def test_gemm_13b_shapes_at_size(bits, n, k, m):
    """BASELINE.json configs[3] shapes (Llama-2-13B linears) at many rows through every hand-written many-row kernel
    (the library hop disabled): a row sample against the CPU oracle linear on the bit-exactly dequantized weights, all
    rows against an fp32 matmul on the same weights, and the two kernel families against each other."""
    from amq_amd import ops
    from amq_amd.llama import _synthetic_linear
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(n + k + bits + m)
    l = _synthetic_linear(n, k, bits, g, dev)
    x = (torch.randn(m, k, device=dev, generator=g) * 0.5).half()
    w = ops.dequantize(l.qn, l.mn, bits, l.mode, n, k)
    ref = x.float() @ w.float().t()
    rms = ref.pow(2).mean().sqrt()
    rows = torch.tensor(sorted({0, 1, m // 3, m // 2, m - 2, m - 1}), device=dev)
    outs = {}
    for route in (ops.GEMM_TILED, ops.GEMM_RING, ops.GEMM_RING128, ops.GEMM_WS, ops.GEMM_DEQ):
        y = ops.gemm(x, l.qn, l.mn, bits, l.mode, n, k, route=route)
        assert torch.all((y.float() - ref).abs() <= 1e-3 * ref.abs() + 1e-3 * rms), route
        _sampled_rows_check(y, x, w, rows, f"13B {n}x{k} {bits}b M={m} route {route}")
        outs[route] = y
    d = (outs[ops.GEMM_TILED].float() - outs[ops.GEMM_RING].float()).abs()
    assert torch.all(d <= 2.0 ** -9 * ref.abs() + 1e-3 * rms)
    # the wave-specialised kernel accumulates every output over k in the ring kernel's order (same MFMA chain): same bits
    assert torch.equal(outs[ops.GEMM_WS], outs[ops.GEMM_RING])
    # the dequantize-once route = the dense fp16 kernel on amq_dequantize_f16's weights, bit for bit; and the ring kernel's bits too
    # (same MFMA chain over k, and the in-loop unpack forms the same fp16 weights as the dequantize kernel on these layers)
    assert torch.equal(outs[ops.GEMM_DEQ], ops.gemm_f16w(x, w))
    assert torch.equal(outs[ops.GEMM_DEQ], outs[ops.GEMM_RING])
    # what GEMM_AUTO runs: the dequantize-once route from AMQ_DEQ_MIN_ROWS rows on (a workspace of N * K * 2 bytes), a fused kernel below
    from amq_amd import _lib as _lib_mod
    need = _lib_mod.load().amq_gemm_route_workspace_bytes(ops.GEMM_AUTO, m, n, k)
    assert need == (n * k * 2 if m >= 6144 else 0)
    auto = ops.gemm(x, l.qn, l.mn, bits, l.mode, n, k)
    if m >= 6144:
        assert torch.equal(auto, outs[ops.GEMM_DEQ])
    else:
        assert any(torch.equal(auto, outs[r]) for r in (ops.GEMM_TILED, ops.GEMM_RING, ops.GEMM_RING128, ops.GEMM_WS))


@pytest.mark.parametrize("m,n,k", [(256, 256, 128), (300, 272, 384), (1000, 1040, 1152), (257, 16, 128), (4096, 5120, 1024), (70000, 256, 128)])
def test_gemm_f16w_dense(m, n, k):
    """amq_gemm_f16w_f16 (amq_gemm_f16.hip: the matmul of GPTQLinear.forward's many-row branch, hqq/backends/autogptq.py:283, on dense
    fp16 weights): every output against an fp32 product within 2 fp16 ulps + 2e-3 rms, ragged M / N tiles, one to several tiles
    per persistent workgroup, bias / residual / SiLU-gate epilogues (the separate fp16 expressions, bit for bit), in place, repeatable."""
    from amq_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(m + n + k)
    x = (torch.randn(m, k, device=dev, generator=g) * 0.5).half()
    w = (torch.randn(n, k, device=dev, generator=g) * 0.05).half()
    bias = (torch.randn(n, device=dev, generator=g) * 0.1).half()
    res = torch.randn(m, n, device=dev, generator=g).half()
    gate = torch.randn(m, n, device=dev, generator=g).half()
    ref = x.float() @ w.float().t()
    y = ops.gemm_f16w(x, w)
    bar = ref.abs() * 2.0 ** -9 + 2e-3 * ref.pow(2).mean().sqrt()
    assert torch.all((y.float() - ref).abs() <= bar)
    assert torch.equal(ops.gemm_f16w(x, w), y)
    assert torch.equal(ops.gemm_f16w(x, w, bias=bias), y + bias)
    assert torch.equal(ops.gemm_f16w(x, w, bias=bias, residual=res), res + (y + bias))
    assert torch.equal(ops.gemm_f16w(x, w, gate=gate), ops.silu_mul(gate.view(-1), y.view(-1)).view(m, n))
    r2 = res.clone()
    ops.gemm_f16w(x, w, residual=r2, out=r2)
    assert torch.equal(r2, res + y)
    g2 = gate.clone()
    ops.gemm_f16w(x, w, gate=g2, out=g2)
    assert torch.equal(g2, ops.silu_mul(gate.view(-1), y.view(-1)).view(m, n))
    with pytest.raises(Exception):
        ops.gemm_f16w(x, w, residual=res, gate=gate)
    with pytest.raises(Exception):
        ops.gemm_f16w(x[:, :k - 64].contiguous(), w[:, :k - 64].contiguous())        # K % 128 != 0


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("m,n,k", [(300, 1040, 1152), (1024, 4096, 256)])
def test_gemm_ring_fma_mode(bits, m, n, k):
    """the ring kernel on MODE_FMA weights (w = fma(q, s, c): what GPTQ / AWQ imports carry): against an fp32 product on the
    bit-exactly dequantized weights and against the tiled kernel (same fp16 weights, different summation order)"""
    from amq_amd import ops
    h, qn, mn, _ = _random_case(bits, n, k, seed=3 * bits + m)
    dev = _dev()
    meta = mn.view(-1, 2).clone()
    meta[:, 1] = -(meta[:, 1] * meta[:, 0])                 # (s, z) -> (s, c = -z*s), the FMA form
    mf = meta.reshape(-1).contiguous()
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(m + k)).half().to(dev)
    w = ops.dequantize(qn, mf, bits, ops.MODE_FMA, n, k)
    ref = x.float() @ w.float().t()
    rms = ref.pow(2).mean().sqrt()
    ring = ops.gemm(x, qn, mf, bits, ops.MODE_FMA, n, k, route=ops.GEMM_RING)
    tiled = ops.gemm(x, qn, mf, bits, ops.MODE_FMA, n, k, route=ops.GEMM_TILED)
    assert torch.all((ring.float() - ref).abs() <= 1e-3 * ref.abs() + 1e-3 * rms)
    assert torch.all((ring.float() - tiled.float()).abs() <= 2.0 ** -9 * ref.abs() + 1e-3 * rms)
    assert torch.equal(ops.gemm(x, qn, mf, bits, ops.MODE_FMA, n, k, route=ops.GEMM_RING), ring)
    assert torch.equal(ops.gemm(x, qn, mf, bits, ops.MODE_FMA, n, k, route=ops.GEMM_WS), ring)      # (amq_gemm_ws.hip: same accumulation order)
