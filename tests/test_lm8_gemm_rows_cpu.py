"""CPU-only: the 8-bit lm_head's tiled many-row entry point (amq_lm8_gemm_rows_f16) as far as it goes without a device -- what it
refuses, one call per rule through the C ABI (made-up pointers: an accepted call would launch), and the ``lm8_kernel="tiled"`` plumbing."""
import ctypes
import inspect

import pytest

from amq_amd import _lib

EINVAL, ESHAPE = -1, -2
one = ctypes.c_void_p(16)
NAME = "amq_lm8_gemm_rows_f16"
ARGS = "x codes meta y M N K group stream"
OK = dict(x=one, codes=one, meta=one, y=one, M=300, N=1000, K=640, group=128, stream=None)
REFUSED = [(f"{n} null", {n: None}, EINVAL) for n in ("x", "codes", "meta", "y")] + [
    (f"{n} not {a}-byte aligned", {n: ctypes.c_void_p(16 + a // 2)}, EINVAL) for n, a in (("x", 16), ("codes", 16), ("meta", 4), ("y", 2))] + [
    ("M 0", dict(M=0), ESHAPE), ("K % 128", dict(K=648), ESHAPE), ("K 0", dict(K=0), ESHAPE), ("group 64", dict(group=64), ESHAPE),
    ("N 0", dict(N=0), ESHAPE), ("x spans 2^32 bytes", dict(M=2 ** 19, K=4096), ESHAPE), ("codes span 2^32 bytes", dict(N=2 ** 20, K=4096), ESHAPE),
    ("2^31 tiles", dict(M=2 ** 23, N=2 ** 24, K=128), ESHAPE)]


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
    layer = LM8Weights(torch.zeros(32, 256, dtype=torch.uint8), torch.zeros(32, 2, 2, dtype=torch.float16), (32, 256))
    for x in (torch.zeros(256, dtype=torch.float16), torch.zeros(0, 256, dtype=torch.float16), torch.zeros(20, 128, dtype=torch.float16),
              torch.zeros(20, 256, dtype=torch.float32), torch.zeros(20, 256, dtype=torch.float16)):       # (the last: right, but not on the GPU)
        with pytest.raises(ValueError, match="x: "):
            ops.lm8_gemm_rows(x, layer)


def test_option_values_defaults_and_refusals():
    from amq_amd import hf_fast, ops, speed, speed_benchmark
    from amq_amd.llama import QuantLlama
    assert "tiled" in ops.LM8_KERNELS
    for fn in (QuantLlama.__init__, QuantLlama.from_hf, hf_fast.convert_model_to_hip, speed.benchmark_speed):
        assert inspect.signature(fn).parameters["lm8_kernel"].default == "dot"
    with pytest.raises(ValueError, match="lm_head_bits=8"):
        QuantLlama("Llama-2-7b-hf", device="cpu", lm8_kernel="tiled")                      # (refused before anything is built)
    p = speed_benchmark.build_parser()
    assert p.parse_args([]).lm8_kernel == "dot"
    assert p.parse_args(["--lm_head_bits", "8", "--lm8_kernel", "tiled"]).lm8_kernel == "tiled"
