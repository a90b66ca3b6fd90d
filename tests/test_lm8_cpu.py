"""CPU-only: the 8-bit lm_head ("LM8") as far as it goes without a device -- the quantizer hqq_format.quantize_lm8 against the
restatement tests/lm8_ref.py, against a derived error bound and against what the reference's own
``Quantizer.quantize(nbits=8, optimize=False, axis=1, group_size=128)`` returned for one input (tests/golden/lm8_rtn_16x256.npz: data recorded from a
CPU run of it); what the two C entry points refuse, one call per rule through the C ABI (made-up pointers: an accepted call would launch); the
``lm_head_bits`` plumbing that needs no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lm8_ref
from amq_amd import _lib, hqq_format

EINVAL, ESHAPE = -1, -2
one = ctypes.c_void_p(16)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm8_rtn_16x256.npz")


def _cases():
    g = torch.Generator().manual_seed(11)
    rnd = (torch.randn(32, 256, generator=g) * 0.02).to(torch.float16)
    edge = (torch.randn(8, 256, generator=g) * 0.02).to(torch.float16)
    edge[0, :128] = 0.0                         # an all-zero group
    edge[1, 128:] = 0.37                        # constant groups
    edge[2, :128] = -3.0
    edge[3, 128:] = 65504.0
    edge[4, :128] = -65504.0
    edge[5, 0], edge[5, 1] = 65504.0, -65504.0  # the whole fp16 range in one group
    edge[6, 128:] = torch.where(torch.arange(128) % 2 == 0, 65504.0, -65504.0).to(torch.float16)
    return {"random": rnd, "edge": edge}


@pytest.mark.parametrize("name", ["random", "edge"])
def test_quantizer_equals_restatement_and_meets_the_bound(name):
    W = _cases()[name]
    q = hqq_format.quantize_lm8(W)
    assert q.codes.dtype == torch.uint8 and tuple(q.codes.shape) == tuple(W.shape) and q.codes.is_contiguous()
    assert q.meta.dtype == torch.float16 and tuple(q.meta.shape) == (W.shape[0], W.shape[1] // 128, 2)
    assert tuple(q.shape) == tuple(W.shape) and q.nbits == 8 and q.group_size == 128
    assert q.nbytes() == W.numel() + W.numel() // 128 * 4
    codes, meta = lm8_ref.quantize(W)
    assert torch.equal(q.codes, codes)
    assert torch.equal(q.meta.view(torch.int16), meta.view(torch.int16))
    assert int(q.codes.min()) >= 0 and int(q.codes.max()) <= 255
    assert bool(torch.isfinite(q.meta).all())
    deq = lm8_ref.dequantize(q.codes, q.meta).to(torch.float64)
    # the product in front of its rounding: where it reaches 65520 the fp16 result is inf, by the format's own rule (a group spanning -65504 .. 65504
    # has the multiplier 513.756, which rounds UP to 514 in fp16: 127.5 * 514 = 65535) -- the bound is then held by the product itself
    c = q.codes.to(torch.float64).reshape(W.shape[0], -1, 128)
    pre = ((c - q.meta[..., 1:2].to(torch.float64)).to(torch.float16).to(torch.float64) * q.meta[..., 0:1].to(torch.float64)).reshape(W.shape)
    over = pre.abs() >= 65520.0
    assert torch.equal(torch.isinf(deq), over) and torch.equal(torch.sign(deq[over]), torch.sign(pre[over]))
    err = (torch.where(over, pre, deq) - W.to(torch.float64)).abs()
    bound = lm8_ref.step_bound(W, q.meta).to(torch.float64)
    worst = float((err - bound).max())
    print(f"{name}: max err {float(err.max()):.6g}, max err - bound {worst:.6g}, {int(over.sum())} products past the fp16 range")
    assert name == "edge" or not bool(over.any())
    assert worst <= 0.0


def test_constant_and_zero_groups_come_back_exactly():
    W = _cases()["edge"]
    q = hqq_format.quantize_lm8(W)
    deq = lm8_ref.dequantize(q.codes, q.meta)
    for row, cols in ((0, slice(0, 128)), (1, slice(128, 256)), (2, slice(0, 128)), (3, slice(128, 256)), (4, slice(0, 128))):
        assert torch.equal(deq[row, cols], W[row, cols])


def test_quantizer_equals_the_reference_quantizer():
    z = np.load(GOLDEN)
    W = torch.from_numpy(z["W"])
    q = hqq_format.quantize_lm8(W)
    assert np.array_equal(q.codes.numpy().reshape(-1, 128), z["W_q"])                       # 8bit_u8 packing: the codes as they are, [N K / 128, 128]
    assert np.array_equal(q.meta[..., 0].reshape(-1).numpy(), z["scale"].reshape(-1).astype(np.float16))
    assert np.array_equal(q.meta[..., 1].reshape(-1).numpy(), z["zero"].reshape(-1).astype(np.float16))
    # ... and the reference's dequantize() of them with the meta in fp16 is the restated weight rule, bit for bit
    assert np.array_equal(lm8_ref.dequantize(q.codes, q.meta).numpy().view(np.uint16), z["deq"].view(np.uint16))


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_quantizer_refuses_nonfinite(bad):
    W = _cases()["random"].clone()
    W[7, 200] = bad
    with pytest.raises(ValueError, match="inf or NaN"):
        hqq_format.quantize_lm8(W)


def test_quantizer_refuses_other_shapes_and_the_old_entry_points_keep_refusing_8_bits():
    with pytest.raises(ValueError):
        hqq_format.quantize_lm8(torch.zeros(4, 192, dtype=torch.float16))
    with pytest.raises(ValueError):
        hqq_format.quantize_lm8(torch.zeros(256, dtype=torch.float16))
    with pytest.raises(ValueError):
        hqq_format.pack_rows(torch.zeros(2, 128, dtype=torch.int32), 8)
    with pytest.raises((ValueError, KeyError)):
        hqq_format.quantize_rtn(torch.zeros(2, 128, dtype=torch.float16), 8)


# ---------------------------------------------------------------------------------------------------------------- the C ABI, no device
GEMV_ARGS = "x codes meta y gamma eps M N K group stream"
GEMV_OK = dict(x=one, codes=one, meta=one, y=one, gamma=None, eps=ctypes.c_float(1e-5), M=3, N=1000, K=640, group=128, stream=None)
DEQ_ARGS = "codes meta out row0 rows N K group stream"
DEQ_OK = dict(codes=one, meta=one, out=one, row0=10, rows=20, N=1000, K=640, group=128, stream=None)
_SHAPE_RULES = [("K % 128", dict(K=648), ESHAPE), ("K 0", dict(K=0), ESHAPE), ("group 64", dict(group=64), ESHAPE), ("group 256", dict(group=256), ESHAPE),
                ("N 0", dict(N=0, row0=0), ESHAPE)]
REFUSED = {
    "amq_lm8_gemv_f16": (GEMV_ARGS, GEMV_OK, [(f"{n} null", {n: None}, EINVAL) for n in ("x", "codes", "meta", "y")] + [
        (f"{n} not {a}-byte aligned", {n: ctypes.c_void_p(16 + a // 2)}, EINVAL) for n, a in (("x", 16), ("codes", 16), ("meta", 4), ("gamma", 16), ("y", 2))] + [
        ("M 0", dict(M=0), ESHAPE), ("M 9", dict(M=9), ESHAPE)] + [(n, {k: v for k, v in d.items() if k != "row0"}, rc) for n, d, rc in _SHAPE_RULES] + [
        ("8 rows of K = 10368 past LDS", dict(M=8, K=10368), ESHAPE)]),
    "amq_lm8_dequantize_f16": (DEQ_ARGS, DEQ_OK, [(f"{n} null", {n: None}, EINVAL) for n in ("codes", "meta", "out")] + [
        (f"{n} not {a}-byte aligned", {n: ctypes.c_void_p(16 + a // 2)}, EINVAL) for n, a in (("codes", 16), ("meta", 4), ("out", 16))] + _SHAPE_RULES + [
        ("row0 -1", dict(row0=-1), ESHAPE), ("rows 0", dict(rows=0), ESHAPE), ("one row past the last", dict(row0=981), ESHAPE),
        ("row0 = N", dict(row0=1000, rows=1), ESHAPE)]),
}
CASES = [(name, why, change, rc) for name, (_, _, rules) in REFUSED.items() for why, change, rc in rules]


@pytest.mark.parametrize("name,why,change,rc", CASES, ids=[f"{n}-{w}" for n, w, _, _ in CASES])
def test_entry_point_refuses(name, why, change, rc):
    order, ok, _ = REFUSED[name]
    args = dict(ok, **change)
    lib = _lib.load()
    got = getattr(lib, name)(*[args[a] for a in order.split()])
    msg = lib.amq_last_error().decode()
    assert got == rc, (why, got, msg)
    assert name in msg, msg                                 # the message names the entry point


# ---------------------------------------------------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("bits", [0, 2, 3, 12, 32, "8", None])
def test_runner_refuses_other_lm_head_bits(bits):
    from amq_amd.llama import QuantLlama
    with pytest.raises(ValueError, match="lm_head_bits"):
        QuantLlama("Llama-2-7b-hf", device="cpu", lm_head_bits=bits)      # (refused before anything is built)


def test_convert_refuses_other_lm_head_bits():
    from amq_amd import hf_fast

    class Fake:
        lm_head = object()

        class model:
            layers = []

    with pytest.raises(ValueError, match="lm_head_bits"):
        hf_fast.convert_model_to_hip(Fake(), lm_head_bits=2)


def test_speed_benchmark_flag_parses():
    from amq_amd import speed_benchmark
    p = speed_benchmark.build_parser()
    assert p.parse_args([]).lm_head_bits == 16
    assert p.parse_args(["--lm_head_bits", "8"]).lm_head_bits == 8
    assert p.parse_args(["--lm_head_bits", "4", "--kv_bits", "8"]).lm_head_bits == 4
    with pytest.raises(SystemExit):
        p.parse_args(["--lm_head_bits", "3"])


def test_signatures_take_the_argument():
    import inspect
    from amq_amd import checkpoint, hf_fast, speed
    from amq_amd.llama import QuantLlama
    for fn in (QuantLlama.__init__, QuantLlama.from_hf, checkpoint.load_mixed, hf_fast.convert_model_to_hip, speed.benchmark_speed):
        assert inspect.signature(fn).parameters["lm_head_bits"].default == 16
