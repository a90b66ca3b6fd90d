"""ops.gptq_hinv(method="hip") -- the upper Cholesky factor of the damped inverse Hessian as HIP kernels (csrc/amq_hinv.hip) --
against fp64: E(U) = max |U^T U A - I| with A the damped matrix lifted to fp64, for the kernels' U and for the existing route's U computed on the
host in fp32 (the reference arithmetic, no device library involved).  Same precision, another operation order: E(kernel) <= 4 E(host).  Then the
variants (dead columns, perm, determinism, a replayed graph, guard bands), the failures, and the quantizers on top of the kernels' factor."""
import copy

import pytest
import torch

import gptq_solver_ref as ref
from test_gptq_quantize_cpu import fixture, rtn_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NB = 64                                             # csrc/amq_kernels.h HINV_NB: block = tile
SIZES = [32, NB, NB + 32, 4 * NB + 32, 1408]        # below a block; one block; a partial block at the top-left; several panel steps; 22 blocks
VARIANTS = [NB + 32, 4 * NB + 32]
_H = {}


def hessian(K, dead=()):
    """H of X random [2 K, K] (the columns ``dead`` zeroed) through ops.GPTQHessian on the device; computed once, never written"""
    if (K, dead) not in _H:
        from amq_amd import ops
        X = torch.randn(2 * K, K, generator=torch.Generator().manual_seed(K))
        X[:, list(dead)] = 0
        acc = ops.GPTQHessian(K, DEV)
        for lo in range(0, 2 * K, 64):
            acc.add_batch(X[lo:lo + 64].unsqueeze(0).to(DEV))
        _H[(K, dead)] = acc.H
    return _H[(K, dead)]


def residual(U, H):
    """E(U) in fp64, A = the preamble of gptq_solver_ref.hinv_upper restated in torch fp32 on the host"""
    A = H.cpu().clone()
    dead = torch.diag(A) == 0
    A[dead, dead] = 1
    idx = torch.arange(A.shape[0])
    A[idx, idx] += 0.01 * torch.mean(torch.diag(A))
    U = U.cpu().double()
    return float((U.t() @ U @ A.double() - torch.eye(A.shape[0], dtype=torch.float64)).abs().max())


@pytest.mark.parametrize("K", SIZES)
def test_against_fp64(K):
    from amq_amd import ops
    H = hessian(K)
    U, dead, where = ops.gptq_hinv(H, 0.01, return_where=True, method="hip")
    host = ops.gptq_hinv(H.cpu(), 0.01)[0]
    e_kernel, e_host = residual(U, H), residual(host, H)
    print(f"K={K}: E(kernel) {e_kernel:.3e}, E(host fp32 route) {e_host:.3e}, ratio {e_kernel / e_host:.3f}")
    assert where == "kernel" and U.dtype == torch.float32 and tuple(U.shape) == (K, K)
    assert e_kernel <= 4 * e_host
    assert torch.equal(U.tril(-1), torch.zeros_like(U)) and bool((U.diagonal() > 0).all())
    assert dead.dtype == torch.bool and torch.equal(dead, torch.diag(H) == 0)


@pytest.mark.parametrize("K", VARIANTS)
def test_dead_columns_perm_and_determinism(K):
    from amq_amd import ops
    H = hessian(K, (0, 17, K - 1))                  # 17: inside the partial block
    U, dead = ops.gptq_hinv(H, 0.01, method="hip")
    assert dead.nonzero().flatten().tolist() == [0, 17, K - 1]
    assert residual(U, H) <= 4 * residual(ops.gptq_hinv(H.cpu(), 0.01)[0], H)
    again, _ = ops.gptq_hinv(H, 0.01, method="hip")
    assert torch.equal(again, U)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K)).to(DEV)
    Up, dead_p = ops.gptq_hinv(H, 0.01, perm=perm, method="hip")
    Ui, dead_i = ops.gptq_hinv(H[perm][:, perm].contiguous(), 0.01, method="hip")
    assert torch.equal(Up, Ui) and torch.equal(dead_p, dead_i) and torch.equal(dead_p, dead[perm])


@pytest.mark.parametrize("K", VARIANTS)
def test_guard_bands_and_a_replayed_graph(K):
    from amq_amd import ops
    eager = [ops.gptq_hinv(h, 0.01, method="hip")[0] for h in (hessian(K), hessian(K, (0, 17, K - 1)))]
    flat = torch.full((2 * K * K + 2 * 4096,), 55.0, device=DEV)       # H, its band, U, its band
    Hbuf, Ubuf = flat[:K * K].view(K, K), flat[K * K + 4096:2 * K * K + 4096].view(K, K)
    bands = (flat[K * K:K * K + 4096], flat[2 * K * K + 4096:])
    _, dead, info, work = ops.gptq_hinv_buffers(K, flat.device)
    Hbuf.copy_(hessian(K))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gptq_hinv_launch(Hbuf, None, 0.01, Ubuf, dead, info, work)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gptq_hinv_launch(Hbuf, None, 0.01, Ubuf, dead, info, work)
    for h, want in ((hessian(K, (0, 17, K - 1)), eager[1]), (hessian(K), eager[0]), (hessian(K), eager[0])):
        Hbuf.copy_(h)
        Ubuf.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(Ubuf, want) and info.cpu().tolist() == [0, 0, 0, 0]
        assert torch.equal(Hbuf, h) and all(bool((b == 55.0).all()) for b in bands)


def test_failures_raise_and_leave_nothing_behind():
    from amq_amd import ops
    K = 4 * NB + 32
    H = hessian(K)
    good = ops.gptq_hinv(H, 0.01, method="hip")[0]
    bad = H.clone()
    bad[100, 100] = -bad[100, 100]                  # indefinite, and 1 % of the mean diagonal does not cure it
    with pytest.raises(ValueError, match="layer 3.down_proj is not positive definite"):
        ops.gptq_hinv(bad, 0.01, name="3.down_proj", method="hip")
    assert torch.equal(ops.gptq_hinv(H, 0.01, method="hip")[0], good)
    bad = H.clone()
    bad[3, 70] = float("nan")
    with pytest.raises(ValueError, match="layer 3.down_proj holds inf or NaN"):
        ops.gptq_hinv(bad, 0.01, name="3.down_proj", method="hip")
    assert torch.equal(ops.gptq_hinv(H, 0.01, method="hip")[0], good)


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_the_solve_on_the_kernels_factor(bits):
    """the band of tests/test_gpu_gptq_quantize.py (device loss against the reference's, and against round-to-nearest), with the kernels' U"""
    from amq_amd import ops
    f = fixture("gptqsolve_64x256_g128")
    W, H = f["W"].to(DEV), f["H"].to(DEV)
    loss = {}
    for method in ("hip", "torch"):
        U, _ = ops.gptq_hinv(H, 0.01, method=method)
        h = ops.gptq_quantize(W, U, bits, 128)
        W_hat = ops.dequantize_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, *W.shape, 128).cpu()
        loss[method] = ref.proxy_loss(f["W"], W_hat, f["H"])
    theirs = ref.proxy_loss(f["W"], f[f"Q_b{bits}"], f["H"])
    rtn = ref.proxy_loss(f["W"], rtn_weights(f["W"], bits, 128), f["H"])
    print(f"b{bits}: proxy loss on the kernels' U / on the existing route's U {loss['hip'] / loss['torch']:.5f}, / reference {loss['hip'] / theirs:.4f}")
    assert loss["hip"] <= 1.05 * theirs and loss["hip"] < 0.5 * rtn


@pytest.mark.parametrize("quantizer", ["gptq", "gptq_act_order", "owq"])
def test_the_model_quantizers_take_the_kernel_route(quantizer):
    pytest.importorskip("transformers")
    from test_gpu_hf import _tiny_llama
    from amq_amd.patching import quantize_model_gptq, quantize_model_owq
    dense = _tiny_llama(2)
    prompts = torch.randint(0, 1000, (8, 8), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        text = dense.generate(prompts, min_new_tokens=56, max_new_tokens=56, do_sample=False, num_beams=1)
    samples = [text[i:i + 1].cpu() for i in range(8)]
    if quantizer == "owq":
        _, report = quantize_model_owq(copy.deepcopy(dense), 3, samples, hinv="hip")
    else:
        order = quantizer == "gptq_act_order"
        _, report = quantize_model_gptq(copy.deepcopy(dense), 3, samples, act_order=order, static_groups=order, hinv="hip")
    print({f"{b}.{n}": round(v["loss"] / v["rtn_loss"], 3) for (b, n), v in report.items()})
    assert len(report) == 14 and all(v["hinv"] == "kernel" for v in report.values())
    assert all(v["loss"] < v["rtn_loss"] for v in report.values())
