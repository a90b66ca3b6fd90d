"""ops.gptq_hinv(method="hip") / amq_gptq_hinv_f32, host side: the validator's refusals in the order include/amq_hip.h states (made-up pointers: an
accepted call would launch), the workspace formula, and the keyword's behaviour without a GPU."""
import ctypes

import pytest
import torch

from amq_amd import _lib, ops

EINVAL = -1


def _call(H=256, perm=None, K=96, U=256, dead=256, info=256, work=256, nbytes=None):
    lib = _lib.load()
    nbytes = lib.amq_gptq_hinv_workspace_bytes(K) if nbytes is None else nbytes
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    rc = lib.amq_gptq_hinv_f32(p(H), p(perm), K, 0.01, p(U), p(dead), p(info), p(work), nbytes, None)
    return rc, lib.amq_last_error().decode()


# each call breaks its own rule and every rule after it: the message names the first
@pytest.mark.parametrize("args,says", [
    (dict(H=None, U=258, K=40, nbytes=0), "null pointer"),
    (dict(info=None, K=0), "null pointer"),
    (dict(U=258, K=40, nbytes=0), "aligned"),
    (dict(perm=2, K=-32), "aligned"),
    (dict(work=264, K=96, nbytes=0), "aligned"),
    (dict(K=40, nbytes=0), "multiple of 32"),
    (dict(K=0, nbytes=0), "multiple of 32"),
    (dict(K=-64, nbytes=0), "multiple of 32"),
    (dict(K=96, nbytes=8 * 128 * 128 + 63), "workspace too small"),
])
def test_refusals_in_the_stated_order(args, says):
    rc, msg = _call(**args)
    assert rc == EINVAL and says in msg, (rc, msg)


@pytest.mark.parametrize("K,Kp", [(32, 64), (64, 64), (96, 128), (288, 320), (11008, 11008), (28672, 28672)])
def test_workspace_formula(K, Kp):
    lib = _lib.load()
    assert lib.amq_gptq_hinv_workspace_bytes(K) == 8 * Kp * Kp + 64
    assert lib.amq_gptq_hinv_workspace_bytes(K + 8) == 0 == lib.amq_gptq_hinv_workspace_bytes(-K) == lib.amq_gptq_hinv_workspace_bytes(0)


def test_the_keyword_on_the_host():
    g = torch.Generator().manual_seed(3)
    X = torch.randn(192, 96, generator=g)
    X[:, 5] = 0
    H = X.t() @ X
    with pytest.raises(ValueError, match="GPU"):
        ops.gptq_hinv(H, method="hip")
    with pytest.raises(ValueError, match="method"):
        ops.gptq_hinv(H, method="rocsolver")
    perm = torch.randperm(96, generator=g)
    U, dead, where = ops.gptq_hinv(H, 0.01, perm=perm, return_where=True)
    U2, dead2 = ops.gptq_hinv(H[perm][:, perm], 0.01)
    assert where == "host" and torch.equal(U, U2) and torch.equal(dead, dead2) and int(dead.sum()) == 1
