"""ops.GPTQHessian(method="hip") -- the Hessian accumulation as one fp16 matrix-core kernel (csrc/amq_hessian.hip) -- against
fp64 under a derived bound.  For an accumulator fed c calls of T_total rows and n sequences in all, H64 = (2 / n) sum X^T X and
A = (2 / n) sum |X|^T |X| in fp64 from the same fp16 rows: |H - H64| <= (T_total + 3 c) 2^-24 A element-wise (exact products, an fp32 summation
chain over the rows, three roundings per call; the kernel does not split T, so nothing is added to the count)."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = [32, 96, 160, 288]          # below a tile; a partial tile; a full tile + partial edge tiles both ways; several tiles with mirrors
CALLS = {"short": ((40, 1, 77), 1), "long": ((130, 64, 200, 9), 1), "b2": ((33, 20), 2)}      # (rows per sequence of each call, b)


@functools.lru_cache(maxsize=None)
def rows(K, calls):
    """the fp16 inputs [b, seqlen, K] of every call (hot columns: every 64th x 12), H64 and A; computed once, never written"""
    seqs, b = CALLS[calls]
    g = torch.Generator().manual_seed(K + len(seqs))
    hot = torch.where(torch.arange(K) % 64 == 0, 12.0, 1.0)
    xs = [(torch.randn(b, T, K, generator=g) * hot).to(torch.float16) for T in seqs]
    flat = torch.cat([x.reshape(-1, K) for x in xs]).double()
    n = b * len(seqs)
    return xs, (2.0 / n) * flat.t() @ flat, (2.0 / n) * flat.abs().t() @ flat.abs()


def accumulate(K, calls, method="hip", twin=False):
    from amq_amd import _lib, ops
    acc = ops.GPTQHessian(K, DEV, method=method)
    if method == "hip":
        acc.H.fill_(float("nan"))                   # n_before == 0: the first call does not read H
    with _lib.routed_to(_lib.open_twin() if twin else _lib.load()):
        for x in rows(K, calls)[0]:
            acc.add_batch(x.to(DEV))
    return acc


@pytest.mark.parametrize("calls", list(CALLS))
@pytest.mark.parametrize("K", KS)
def test_against_fp64_under_the_derived_bound(K, calls):
    xs, H64, A = rows(K, calls)
    acc = accumulate(K, calls)
    H = acc.H.cpu()
    assert acc.nsamples == sum(x.shape[0] for x in xs) and bool(torch.isfinite(H).all())
    bound = (sum(x.shape[0] * x.shape[1] for x in xs) + 3 * len(xs)) * 2.0 ** -24 * A
    share = {m: float(((h.double() - H64).abs() / bound).max()) for m, h in (("kernel", H), ("torch", accumulate(K, calls, "torch").H.cpu()))}
    print(f"K={K} {calls}: largest error / bound, kernel {share['kernel']:.4f}, torch route {share['torch']:.4f}")
    assert bool(((H.double() - H64).abs() <= bound).all())
    assert torch.equal(H, H.t())
    assert torch.equal(accumulate(K, calls).H.cpu(), H) and torch.equal(accumulate(K, calls, twin=True).H.cpu(), H)      # run to run; the waits twin


@pytest.mark.parametrize("K", [160, 288])
def test_guard_bands_a_strided_x_and_a_replayed_graph(K):
    # rows of a wider buffer, n_before > 0 (H is read): the contiguous eager call's bits from every replay, nothing else touched
    from amq_amd import ops
    T, wide = 77, K + 24
    g = torch.Generator().manual_seed(K)
    inputs = [(torch.randn(T, K, generator=g).to(torch.float16).to(DEV), torch.randn(K, K, generator=g).to(DEV)) for _ in range(2)]
    eager = [H0.clone() for _, H0 in inputs]
    for (x, _), H in zip(inputs, eager):
        ops.gptq_hessian_launch(x, H, 3, 2)
    xbuf = torch.full((T + 8, wide), 55.0, dtype=torch.float16, device=DEV)
    hbuf = torch.full((K * K + 4096,), 55.0, device=DEV)
    xv, Hv = xbuf[:T, :K], hbuf[:K * K].view(K, K)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gptq_hessian_launch(xv, Hv, 3, 2)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        ops.gptq_hessian_launch(xv, Hv, 3, 2)
    for i in (1, 0, 0):
        xv.copy_(inputs[i][0])
        Hv.copy_(inputs[i][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(Hv, eager[i]) and torch.equal(xv, inputs[i][0])
        assert bool((xbuf[:T, K:] == 55.0).all()) and bool((xbuf[T:] == 55.0).all()) and bool((hbuf[K * K:] == 55.0).all())


@pytest.mark.parametrize("quantizer", ["gptq", "owq"])
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
        _, report = quantize_model_owq(copy.deepcopy(dense), 3, samples, hessian="hip")
    else:
        _, report = quantize_model_gptq(copy.deepcopy(dense), 3, samples, hessian="hip", hinv="hip")
    assert len(report) == 14 and all(v["hessian"] == "kernel" for v in report.values())
    assert all(v["loss"] < v["rtn_loss"] for v in report.values())
