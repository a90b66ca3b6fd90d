"""ops.GPTQHessian(method="hip") / amq_gptq_hessian_f16, host side: the validator's refusals in the order include/amq_hip.h states (made-up
pointers: an accepted call would launch), the workspace query (the kernel needs none), and the keywords' behaviour without a GPU."""
import ctypes

import pytest
import torch

from amq_amd import _lib, ops, patching

EINVAL = -1


def _call(x=256, stride=96, T=8, K=96, H=512, n=0, b=1):
    lib = _lib.load()
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    rc = lib.amq_gptq_hessian_f16(p(x), stride, T, K, p(H), n, b, None, 0, None)
    return rc, lib.amq_last_error().decode()


# each call breaks its own rule and every rule after it: the message names the first
@pytest.mark.parametrize("args,says", [
    (dict(H=None, K=0, b=0), "null pointer"),
    (dict(x=264, K=40, T=0, stride=7), "16-byte aligned"),
    (dict(K=40, T=0, stride=7), "multiple of 32"),
    (dict(K=65536, stride=65536, T=0), "multiple of 32"),
    (dict(T=0, stride=7), "T >= 1"),
    (dict(n=-1, b=0, stride=100), "T >= 1"),
    (dict(stride=88), "x_row_stride"),
    (dict(stride=100), "x_row_stride"),
])
def test_refusals_in_the_stated_order(args, says):
    rc, msg = _call(**args)
    assert rc == EINVAL and says in msg, (rc, msg)


def test_the_keywords_on_the_host():
    assert all(_lib.load().amq_gptq_hessian_workspace_bytes(T, K) == 0 for T, K in ((2048, 4096), (8, 40), (0, 96)))      # the kernel needs none
    with pytest.raises(ValueError, match="method='torch'"):
        ops.GPTQHessian(96, "cpu", method="hip")
    with pytest.raises(ValueError, match="method='torch'"):
        ops.GPTQHessian(40, "cuda:0", method="hip")
    with pytest.raises(ValueError, match="'torch' or 'hip'"):
        ops.GPTQHessian(96, "cpu", method="rocblas")
    for quantize in (patching.quantize_model_gptq, patching.quantize_model_owq):
        with pytest.raises(ValueError, match="hessian must be 'torch'"):
            quantize(None, 3, [], hessian="rocblas")
    # method="torch" is the accumulation as it was: the reference's running form, restated
    g = torch.Generator().manual_seed(11)
    calls = [torch.randn(b, T, 96, generator=g).to(dt) for b, T, dt in ((1, 40, torch.float16), (2, 9, torch.float32), (1, 1, torch.float16))]
    acc, H, n = ops.GPTQHessian(96, "cpu", method="torch"), torch.zeros(96, 96), 0
    for x in calls:
        acc.add_batch(x)
        H *= n / (n + x.shape[0])
        n += x.shape[0]
        xt = (2.0 / n) ** 0.5 * x.reshape(-1, 96).t().float()
        H += xt.matmul(xt.t())
    assert acc.nsamples == n == 4 and torch.equal(acc.H, H) and torch.equal(ops.GPTQHessian(96, "cpu").H, torch.zeros(96, 96))
