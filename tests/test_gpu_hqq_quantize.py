"""ops.hqq_quantize -- HQQ's quantizer with its proximal solver as HIP kernels (csrc/amq_quantize.hip) -- against what the reference's
own quantizer produced on the CPU (tests/golden/hqq_*.npz, hqq_quant_edge.npz), against the torch restatement with the kernels' summation orders
(tests/hqq_solver_ref.py), and through every layer above it (repack, the drop-in module, a quantized HF model that generates and is scored).

The conditions on codes and zeros are caps, not measurements: the device's powf is not libm's, so a value may land on the other side of a rounding
boundary.  Per case at most 1 % of the groups may differ at all, a differing code differs by exactly one step, |d zero| <= 0.5; scale is bit-identical
(it does not depend on the solver).  What the device really gives is printed and written to profiles/hqq_quantize.json ("parity")."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import hqq_solver_ref as ref
from quantize_common import HQQ_DIGEST_CASES, assert_codes, hqq_digest, hqq_digest_key, unpack_rows
from test_hqq_quantize_cpu import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "hqq_quantize.json")
OBSERVED = {}
_REF = {}


def restated(key, W, nbits, group):
    """the CPU restatement, computed once per case and left unchanged"""
    if key not in _REF:
        _REF[key] = ref.solve(W, nbits, group)
    return _REF[key]


def multi_w(N, K):
    g = torch.Generator().manual_seed(N * 7 + K)
    W = torch.randn(N, K, generator=g) * 0.02
    W[::5, ::11] *= 4.0
    return W.half()


def compare(name, h, info, q_ref, scale_ref, zero_ref, ref_trace=None):
    """the caps of the module docstring between a device result and (codes [R, G], scale, zero); notes what was observed"""
    R = q_ref.shape[0]
    q = unpack_rows(h.W_q.cpu(), h.nbits, R)
    dq = (q - q_ref.to(torch.int32)).abs()
    z, zr = h.zero.cpu().float().reshape(-1), zero_ref.float().reshape(-1)
    dz = (z - zr).abs()
    differing = (dq.max(dim=1)[0] > 0) | (dz > 0)
    OBSERVED[name] = {"groups": R, "groups_differing": int(differing.sum()), "codes_differing": int((dq > 0).sum()),
                      "zeros_differing": int((dz > 0).sum()), "max_abs_dzero": float(dz.max()), "max_code_step": int(dq.max()), "stop": info.stop}
    if ref_trace is not None:
        OBSERVED[name]["ref_stop"] = ref_trace["stop"]
        OBSERVED[name]["mean_err_max_rel"] = float(((info.mean_err - ref_trace["mean_err"]).abs() / ref_trace["mean_err"].abs().clamp_min(1e-30)).max())
    print(name, OBSERVED[name])
    assert torch.equal(h.scale.cpu().reshape(-1).view(torch.int16), scale_ref.reshape(-1).view(torch.int16)), "scale is not bit-identical"
    assert int(differing.sum()) <= 0.01 * R, f"{int(differing.sum())} of {R} groups differ"
    assert int(dq.max()) <= 1, "a code differs by more than one step"
    assert float(dz.max()) <= 0.5, "|d zero| > 0.5"
    if ref_trace is not None:
        assert OBSERVED[name]["mean_err_max_rel"] <= 1e-5, "mean_err trace"
        if ref_trace["gap"] > 1e-4:
            assert info.stop == ref_trace["stop"]
        else:
            assert abs(info.stop - ref_trace["stop"]) <= 1
    assert info.nonfinite == 0


def mean_abs_err(W, W_hat):
    return float((W.double() - W_hat.double()).abs().mean())


def device_dequant(h):
    from amq_amd import ops
    n, k = h.shape
    return ops.dequantize_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), h.nbits, n, k, group=h.group_size).cpu()


# ---------------------------------------------------------------------------------------------------------------- fixtures and quality
@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_fixture_through_the_device_quantizer(name):
    from amq_amd import ops
    d = dict(CASES)[name]()
    W = torch.from_numpy(d["W"])
    bits, group = d["nbits"], d["group_size"]
    h, info = ops.hqq_quantize(W.to(DEV), bits, group, return_info=True)
    assert h.W_q.dtype == torch.from_numpy(d["W_q"]).dtype and tuple(h.W_q.shape) == tuple(d["W_q"].shape)
    assert h.scale.shape == h.zero.shape == (W.numel() // group, 1)
    R = W.numel() // group
    q_ref = unpack_rows(torch.from_numpy(d["W_q"]), bits, R)
    compare(name, h, info, q_ref, torch.from_numpy(d["scale"]), torch.from_numpy(d["zero"]), restated(name, W, bits, group))
    # quality: the solver ran and stopped where it should -- 1e-3 is 1/25 of its smallest gain over round-to-nearest on these fixtures
    ours, theirs = mean_abs_err(W, device_dequant(h)), mean_abs_err(W, torch.from_numpy(d["W_deq"]))
    OBSERVED[name]["mean_abs_err"], OBSERVED[name]["reference_mean_abs_err"] = ours, theirs
    print(name, "mean |W - W^|", ours, "reference", theirs)
    assert ours <= theirs * (1 + 1e-3)


# ---------------------------------------------------------------------------------------------------------------- several workgroups
@pytest.mark.parametrize("group", [64, 128])
@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("N,K", [(256, 1024), (48, 11008)])      # 48 x 11008 / 64: 8256 groups = 3 passes per wave, 688 workgroups (3 chunks of the stop kernel); R % 10 != 0
def test_several_workgroups_against_the_restatement(N, K, bits, group):
    from amq_amd import _lib, ops
    W = multi_w(N, K)
    name = f"multi_{N}x{K}_b{bits}_g{group}"
    r = restated(name, W, bits, group)
    Wd = W.to(DEV)
    h, info = ops.hqq_quantize(Wd, bits, group, return_info=True)
    compare(name, h, info, r["q"], r["scale"], r["zero"], r)
    again, info2 = ops.hqq_quantize(Wd, bits, group, return_info=True)
    assert torch.equal(again.W_q, h.W_q) and torch.equal(again.scale, h.scale) and torch.equal(again.zero, h.zero)
    assert_codes(again, unpack_rows(h.W_q.cpu(), bits, N * K // group))
    assert info2.stop == info.stop and torch.equal(info2.mean_err, info.mean_err)
    with _lib.routed_to(_lib.open_twin()):
        twin, info3 = ops.hqq_quantize(Wd, bits, group, return_info=True)
    assert torch.equal(twin.W_q, h.W_q) and torch.equal(twin.scale, h.scale) and torch.equal(twin.zero, h.zero)
    assert info3.stop == info.stop and torch.equal(info3.mean_err, info.mean_err)


@pytest.mark.parametrize("N,K,group,bits", HQQ_DIGEST_CASES)
def test_bits_of_the_recorded_commit(N, K, group, bits):
    """W_q, scale, zero and the info block are, byte for byte, what the commit recorded in tests/golden/hqq_digests.json gave (the restatement
    holds the solver within 1 % of the groups only, which a changed rounding could pass): tests/golden/gen_hqq_digests.py wrote the file"""
    from amq_amd import ops
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "hqq_digests.json")))
    h, info = ops.hqq_quantize(multi_w(N, K).to(DEV), bits, group, return_info=True)
    got, want = hqq_digest(h, info), doc["cases"][hqq_digest_key(N, K, group, bits)]
    assert got == want, (f"{[k for k in want if got[k] != want[k]]} differ from commit {doc['commit'][:7]}; recorded under HIP {doc['hip']}, "
                         f"this run under HIP {torch.version.hip}")


def test_round_zero_option_and_wider_dtypes():
    from amq_amd import ops
    W = multi_w(64, 512)
    for bits, rz in ((4, False), (3, True)):
        r = ref.solve(W, bits, 128, round_zero=rz)
        h, info = ops.hqq_quantize(W.to(DEV), bits, 128, round_zero=rz, return_info=True)
        compare(f"round_zero_{rz}_b{bits}", h, info, r["q"], r["scale"], r["zero"], r)
    base = ops.hqq_quantize(W.to(DEV), 3, 128)
    wide = ops.hqq_quantize(W.to(DEV).float(), 3, 128)             # cast to fp16 at the boundary: W holds fp16 values, so the same result
    assert torch.equal(wide.W_q, base.W_q) and torch.equal(wide.zero, base.zero) and torch.equal(wide.scale, base.scale)
    b16 = ops.hqq_quantize(W.to(torch.bfloat16).to(DEV), 3, 128)
    same = ops.hqq_quantize(W.to(torch.bfloat16).to(torch.float16).to(DEV), 3, 128)
    assert torch.equal(b16.W_q, same.W_q) and b16.scale.dtype == torch.float16 and torch.equal(b16.scale, same.scale)
    with pytest.raises(ValueError):
        ops.hqq_quantize(W.to(DEV), 3, 384)
    with pytest.raises(ValueError):
        ops.hqq_quantize(W, 3, 128)                                 # not on the GPU


# ---------------------------------------------------------------------------------------------------------------- through the layers
@pytest.mark.parametrize("bits,group", [(2, 128), (3, 128), (4, 128), (3, 64), (4, 32), (2, 256)])
def test_repacked_result_dequantizes_to_format_a(bits, group):
    from amq_amd import ops
    from amq_amd.hqq_format import quantize_hqq
    N, K = 64, 512
    W = multi_w(N, K).to(DEV)
    h = quantize_hqq(W, bits, group)
    qn, mn = ops.repack_from_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, N, K, group=group)
    got = ops.dequantize(qn, mn, bits, ops.MODE_HQQ, N, K)
    q = unpack_rows(h.W_q, bits, N * K // group).to(torch.float16)
    want = ((q - h.zero) * h.scale).reshape(N, K)                    # fp16: two roundings, as HQQ dequantizes
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_from_linear_matches_f_linear_on_its_weights(bits):
    from amq_amd.quant_linear import HIPQuantLinear
    torch.manual_seed(bits)
    lin = torch.nn.Linear(512, 256, bias=True).to(DEV).half()
    mod = HIPQuantLinear.from_linear(lin, bits)
    assert mod.bits == bits and mod.group_size == 128 and mod.bias is not None
    w = mod.dequantize()
    # the weights are the layer's, quantized: every group's mean error is below half a step of its range (rounding alone gives a quarter)
    wl = lin.weight.detach().float().reshape(-1, 128)
    step = (wl.amax(1) - wl.amin(1)) / (2 ** bits - 1)
    assert bool(((w.float().reshape(-1, 128) - wl).abs().mean(1) <= 0.5 * step).all())
    for rows in (1, 5, 40):
        x = torch.randn(rows, 512, device=DEV).half()
        y = mod(x)
        want = torch.nn.functional.linear(x.double(), w.double(), lin.bias.detach().double())
        # the matmul bar of tests/test_gpu_kernels.py for outputs behind a bias add (_assert_close_biased)
        tol = (1e-3 + 2.0 ** -10) * want.abs() + 1e-3 * want.pow(2).mean().sqrt()
        assert bool(((y.double() - want).abs() <= tol).all()), float(((y.double() - want).abs() / tol).max())


def test_nan_and_inf_raise():
    from amq_amd import ops
    for bad in (float("nan"), float("inf"), -float("inf")):
        W = multi_w(64, 512)
        W[33, 257] = bad
        with pytest.raises(ValueError, match="inf or NaN"):
            ops.hqq_quantize(W.to(DEV), 4, 128)


def test_entry_point_replays_from_a_captured_graph():
    from amq_amd import ops
    N, K, bits, group = 256, 1024, 3, 128
    W1, W2 = multi_w(N, K).to(DEV), (multi_w(N, K).flip(0) * 1.5).half().to(DEV)
    eager = [ops.hqq_quantize(w, bits, group, return_info=True) for w in (W1, W2)]
    Wbuf = W1.clone()
    W_q, scale, zero, info, _ = ops.hqq_quantize_buffers(N, K, bits, group, Wbuf.device)
    work = torch.empty(ref.workspace_bytes(N, K, group) // 4, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.hqq_quantize_launch(Wbuf, bits, group, False, W_q, scale, zero, info, work)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.hqq_quantize_launch(Wbuf, bits, group, False, W_q, scale, zero, info, work)
    for w, (h, i) in ((W2, eager[1]), (W1, eager[0])):
        Wbuf.copy_(w)
        graph.replay()
        torch.cuda.synchronize()
        got = ops.HQQQuantizeInfo(info.cpu())
        assert torch.equal(W_q, h.W_q) and torch.equal(scale, h.scale) and torch.equal(zero, h.zero)
        assert got.stop == i.stop and torch.equal(got.mean_err, i.mean_err)


def test_quantize_model_generates_and_scores_below_round_to_nearest():
    pytest.importorskip("transformers")
    from test_gpu_hf import _tiny_llama
    from amq_amd import evaluate
    from amq_amd.arch import LINEARS
    from amq_amd.hqq_format import quantize_rtn
    from amq_amd.patching import HQQWeightsModule, prepare_for_inference, quantize_bank, quantize_model
    from amq_amd.quant_linear import HIPQuantLinear
    dense = _tiny_llama(2)
    cycle = (4, 2, 3, 3, 2, 4, 3)
    bits = {name: [cycle[(i + b) % 7] for b in range(2)] for i, name in enumerate(LINEARS)}       # a mixed per-linear assignment
    # windows the dense model wrote itself (greedy continuations of random prompts): text it is sure about, so weight error costs likelihood
    g = torch.Generator().manual_seed(5)
    prompts = torch.randint(0, 1000, (8, 8), generator=g).to(DEV)
    with torch.no_grad():
        text = dense.generate(prompts, min_new_tokens=56, max_new_tokens=56, do_sample=False, num_beams=1)
    windows = [text[:4].cpu(), text[4:].cpu()]

    rtn = copy.deepcopy(dense)
    for b, layer in enumerate(rtn.model.layers):
        for full in LINEARS:
            parent, attr = full.split(".")
            lin = getattr(getattr(layer, parent), attr)
            setattr(getattr(layer, parent), attr, HQQWeightsModule(quantize_rtn(lin.weight.detach(), bits[full][b], 128)))
    prepare_for_inference(rtn, backend="hip")

    bank = quantize_bank(dense, bits=(2, 3))
    assert set(bank) == {2, 3} and len(bank[2]) == 14 and bank[3][(1, "mlp.down_proj")].nbits == 3
    assert isinstance(dense.model.layers[0].mlp.down_proj, torch.nn.Linear)                       # the bank leaves the model as it was

    ours = quantize_model(copy.deepcopy(dense), {"linear": bits})
    for b, layer in enumerate(ours.model.layers):
        for full in LINEARS:
            parent, attr = full.split(".")
            mod = getattr(getattr(layer, parent), attr)
            assert isinstance(mod, HIPQuantLinear) and mod.bits == bits[full][b], (b, full)
    assert isinstance(ours.lm_head, torch.nn.Linear) and ours.lm_head.weight.dtype == torch.float16
    with pytest.raises(TypeError):
        quantize_model(ours, 4)                                                                    # already quantized
    prepare_for_inference(ours, backend="hip")
    with torch.no_grad():
        out = ours.generate(prompts[:2], min_new_tokens=6, max_new_tokens=6, do_sample=False, num_beams=1)
    assert out.shape == (2, 14)
    ppl_dense = float(np.exp(np.mean([torch.nn.functional.cross_entropy(dense(w.to(DEV)).logits[:, :-1].float().reshape(-1, 1000),
                                                                        w[:, 1:].reshape(-1).to(DEV)).item() for w in windows])))
    # (eval_ppl keeps the reference's window arithmetic: with B = 4 sequences per window it returns the per-token perplexity to the 4th power)
    ppl_ours = evaluate.eval_ppl(ours, None, windows, seqlen=64)
    ppl_rtn = evaluate.eval_ppl(rtn, None, windows, seqlen=64)
    OBSERVED["tiny_llama_ppl"] = {"dense": ppl_dense, "hqq_quantize": ppl_ours, "quantize_rtn": ppl_rtn}
    print("perplexity: dense", ppl_dense, "hqq_quantize", ppl_ours, "quantize_rtn", ppl_rtn)
    assert ppl_ours < ppl_rtn


def test_zz_observed_counts_are_recorded():
    """last in the file: what the device gave in the tests above goes to profiles/hqq_quantize.json under "parity" (the timings of
    tools/quantize_bench.py live beside it)"""
    if not OBSERVED:                        # (run alone: nothing to record)
        return
    try:
        doc = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        doc["parity"] = {"device": torch.cuda.get_device_name(0), "cases": OBSERVED}
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError as e:                    # a read-only checkout: the assertions above are what counts
        print("not recorded:", e)
