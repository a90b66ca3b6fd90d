"""CPU-only: the 8-bit lm_head's matrix-core entry point (amq_lm8_gemm_f16) as far as it goes without a device -- what it refuses,
one call per rule through the C ABI (made-up pointers: an accepted call would launch), and the ``lm8_kernel`` plumbing that needs no GPU."""
import ctypes
import inspect

import pytest

from amq_amd import _lib

EINVAL, ESHAPE = -1, -2
one = ctypes.c_void_p(16)
NAME = "amq_lm8_gemm_f16"
ARGS = "x codes meta y gamma eps M N K group stream"
OK = dict(x=one, codes=one, meta=one, y=one, gamma=None, eps=ctypes.c_float(1e-5), M=3, N=1000, K=640, group=128, stream=None)
REFUSED = [(f"{n} null", {n: None}, EINVAL) for n in ("x", "codes", "meta", "y")] + [
    (f"{n} not {a}-byte aligned", {n: ctypes.c_void_p(16 + a // 2)}, EINVAL) for n, a in (("x", 16), ("codes", 16), ("meta", 4), ("gamma", 16), ("y", 2))] + [
    ("M 0", dict(M=0), ESHAPE), ("M 17", dict(M=17), ESHAPE), ("K % 128", dict(K=648), ESHAPE), ("K 0", dict(K=0), ESHAPE),
    ("group 64", dict(group=64), ESHAPE), ("N 0", dict(N=0), ESHAPE), ("16 rows of K = 8192 past LDS", dict(M=16, K=8192), ESHAPE)]


@pytest.mark.parametrize("why,change,rc", REFUSED, ids=[w for w, _, _ in REFUSED])
def test_entry_point_refuses(why, change, rc):
    args = dict(OK, **change)
    lib = _lib.load()
    got = getattr(lib, NAME)(*[args[a] for a in ARGS.split()])
    msg = lib.amq_last_error().decode()
    assert got == rc, (why, got, msg)
    assert NAME in msg, msg                                 # the message names the entry point


def test_ops_wrapper_refuses_before_the_library_is_called(monkeypatch):
    import torch
    from amq_amd import ops
    from amq_amd.hqq_format import LM8Weights
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    layer = lambda k: LM8Weights(torch.zeros(32, k, dtype=torch.uint8), torch.zeros(32, k // 128, 2, dtype=torch.float16), (32, k))
    assert (ops.lm8_gemm_max_rows(4096), ops.lm8_gemm_max_rows(8192)) == (16, 9)
    for rows, k in ((17, 128), (0, 128), (16, 8192)):
        with pytest.raises(ValueError, match="rows"):
            ops.lm8_gemm(torch.zeros(rows, k, dtype=torch.float16), layer(k))


def test_option_defaults_and_refusals():
    from amq_amd import hf_fast, speed, speed_benchmark
    from amq_amd.llama import QuantLlama
    for fn in (QuantLlama.__init__, QuantLlama.from_hf, hf_fast.convert_model_to_hip, speed.benchmark_speed):
        assert inspect.signature(fn).parameters["lm8_kernel"].default == "dot"
    with pytest.raises(ValueError, match="lm_head_bits=8"):
        QuantLlama("Llama-2-7b-hf", device="cpu", lm8_kernel="mfma")                       # (refused before anything is built)
    with pytest.raises(ValueError, match="lm8_kernel"):
        QuantLlama("Llama-2-7b-hf", device="cpu", lm_head_bits=8, lm8_kernel="x")
    p = speed_benchmark.build_parser()
    assert p.parse_args([]).lm8_kernel == "dot"
    assert p.parse_args(["--lm_head_bits", "8", "--lm8_kernel", "mfma"]).lm8_kernel == "mfma"
    with pytest.raises(SystemExit):
        p.parse_args(["--lm8_kernel", "x"])
