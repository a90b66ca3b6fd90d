"""ops.gptq_quantize -- GPTQ's error-feedback solve as HIP kernels (csrc/amq_gptq.hip) -- against the torch restatement of its
arithmetic (tests/gptq_solver_ref.py): codes, scale, zero and the rows' losses BIT FOR BIT (every operation is a basic IEEE fp32 operation in a
fixed order, so no tolerance is granted), on the reference's fixtures (tests/golden/gptqsolve_*.npz) and on shapes beyond them; the loss against
the reference's own result; and through every layer above it up to a calibrated, packed HF model that generates.  What the device gives is
printed and written to profiles/gptq_quantize.json ("parity")."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import gptq_solver_ref as ref
from quantize_common import assert_codes, assert_format_a, same_bits
from test_gptq_quantize_cpu import CASES, IDS, fixture, restated, rtn_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "gptq_quantize.json")
OBSERVED = {}
_SEEDED = {}


def seeded(N, K, group, bits):
    """(W fp16, U fp32, the restatement) of a shape beyond the fixtures: W and X from a seeded generator, U on the CPU; computed once"""
    key = (N, K, group, bits)
    if key not in _SEEDED:
        from amq_amd import ops
        g = torch.Generator().manual_seed(N * 13 + K + group + bits)
        W = (torch.randn(N, K, generator=g) * 0.02).half()
        W[::5, ::11] *= 4.0
        r = K // 8
        X = torch.randn(2 * K, r, generator=g) @ (torch.randn(r, K, generator=g) / r ** 0.5) + 0.3 * torch.randn(2 * K, K, generator=g)
        X[:, ::37] *= 10.0
        acc = ops.GPTQHessian(K, "cpu")
        for lo in range(0, 2 * K, 64):
            acc.add_batch(X[lo:lo + 64].half().unsqueeze(0))
        U, dead = ops.gptq_hinv(acc.H, 0.01)
        assert not bool(dead.any())
        _SEEDED[key] = (W, U, ref.solve(W, U, bits, group, deploy=True))
    return _SEEDED[key]


def identical(h, info, want, nbits, group, shape):
    """codes, scale, zero and row_loss of a device result equal the restatement's, bit for bit; Format A's shapes and dtypes"""
    N = shape[0]
    assert_format_a(h, nbits, group, shape)
    assert info.nonfinite == 0 and want["nonfinite"] == 0
    assert_codes(h, want["q"])
    assert same_bits(h.scale.cpu(), want["scale"]), "scale"
    assert same_bits(h.zero.cpu(), want["zero"]), "zero"
    assert info.row_loss.dtype == torch.float32 and tuple(info.row_loss.shape) == (N,)
    assert same_bits(info.row_loss.cpu(), want["row_loss"]), "row_loss"
    assert info.loss == pytest.approx(want["loss"], rel=1e-12)         # (fp64 sums of the same fp32 values, in the device's and the host's order)


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_fixtures_bit_for_bit_and_the_loss_against_the_reference(name, bits):
    from amq_amd import ops
    f = fixture(name)
    group = int(f["group"])
    want = restated(name, bits, True)
    h, info = ops.gptq_quantize(f["W"].to(DEV), f["U"].to(DEV), bits, group, return_info=True)
    identical(h, info, want, bits, group, f["W"].shape)
    N, K = f["W"].shape
    W_hat = ops.dequantize_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, N, K, group).cpu()
    assert torch.equal(W_hat.float(), want["W_hat"]), "the error feedback saw another weight than the packed layer dequantizes to"
    ours = ref.proxy_loss(f["W"], W_hat, f["H"])
    theirs = ref.proxy_loss(f["W"], f[f"Q_b{bits}"], f["H"])
    rtn = ref.proxy_loss(f["W"], rtn_weights(f["W"], bits, group), f["H"])
    OBSERVED[f"{name}_b{bits}"] = {"loss": ours, "reference_loss": theirs, "rtn_loss": rtn, "over_reference": ours / theirs, "over_rtn": ours / rtn,
                                   "solver_loss": info.loss, "reference_solver_loss": float(f[f"loss_b{bits}"])}
    print(f"{name} b{bits}: device / reference {ours / theirs:.4f}, device / round-to-nearest {ours / rtn:.4f}")
    assert ours <= 1.05 * theirs
    assert ours < 0.5 * rtn


# one block and a quarter of a wave's rows; groups of 64 over two blocks; groups of 32 over four; several workgroups with N % 64 != 0; eleven
# blocks: long trailing chains
BEYOND = [(16, 128, 128, 4), (48, 256, 64, 3), (80, 512, 32, 2), (272, 384, 128, 3), (64, 1408, 128, 4)]


@pytest.mark.parametrize("N,K,group,bits", BEYOND)
def test_shapes_beyond_the_fixtures_bit_for_bit(N, K, group, bits):
    from amq_amd import ops
    W, U, want = seeded(N, K, group, bits)
    h, info = ops.gptq_quantize(W.to(DEV), U.to(DEV), bits, group, return_info=True)
    identical(h, info, want, bits, group, (N, K))


def test_run_to_run_and_the_conservative_twin_give_the_same_bits():
    from amq_amd import _lib, ops
    W, U, _ = seeded(272, 384, 128, 3)
    Wd, Ud = W.to(DEV), U.to(DEV)
    h, info = ops.gptq_quantize(Wd, Ud, 3, 128, return_info=True)
    again, info2 = ops.gptq_quantize(Wd, Ud, 3, 128, return_info=True)
    with _lib.routed_to(_lib.open_twin()):
        twin, info3 = ops.gptq_quantize(Wd, Ud, 3, 128, return_info=True)
    for other, i in ((again, info2), (twin, info3)):
        assert torch.equal(other.W_q, h.W_q) and torch.equal(other.scale, h.scale) and torch.equal(other.zero, h.zero)
        assert torch.equal(i.row_loss, info.row_loss)


def test_entry_point_replays_from_a_captured_graph():
    from amq_amd import ops
    N, K, group, bits = 48, 256, 64, 3
    W1, U, _ = seeded(N, K, group, bits)
    W1, U = W1.to(DEV), U.to(DEV)
    W2 = (W1.flip(0) * 1.5).half()
    eager = [ops.gptq_quantize(w, U, bits, group, return_info=True) for w in (W1, W2)]
    Wbuf = W1.clone()
    W_q, scale, zero, row_loss, info, _ = ops.gptq_quantize_buffers(N, K, bits, group, Wbuf.device)
    work = torch.empty((ref.workspace_bytes(N, K, group) + 3) // 4, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gptq_quantize_launch(Wbuf, U, bits, group, W_q, scale, zero, row_loss, info, work)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gptq_quantize_launch(Wbuf, U, bits, group, W_q, scale, zero, row_loss, info, work)
    for w, (h, i) in ((W2, eager[1]), (W1, eager[0])):
        Wbuf.copy_(w)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(W_q, h.W_q) and torch.equal(scale, h.scale) and torch.equal(zero, h.zero)
        assert torch.equal(row_loss, i.row_loss) and int(info.cpu()[0]) == 0


def test_wider_dtypes_are_cast_at_the_boundary():
    from amq_amd import ops
    W, U, _ = seeded(48, 256, 64, 3)
    Ud = U.to(DEV)
    base = ops.gptq_quantize(W.to(DEV), Ud, 3, 64)
    wide = ops.gptq_quantize(W.to(DEV).float(), Ud, 3, 64)                 # W holds fp16 values, so the same result
    assert torch.equal(wide.W_q, base.W_q) and torch.equal(wide.scale, base.scale) and torch.equal(wide.zero, base.zero)
    b16 = ops.gptq_quantize(W.to(torch.bfloat16).to(DEV), Ud, 3, 64)
    same = ops.gptq_quantize(W.to(torch.bfloat16).to(torch.float16).to(DEV), Ud, 3, 64)
    assert torch.equal(b16.W_q, same.W_q) and torch.equal(b16.scale, same.scale) and torch.equal(b16.zero, same.zero)


def test_refusals():
    from amq_amd import ops
    W, U, _ = seeded(48, 256, 64, 3)
    Wd, Ud = W.to(DEV), U.to(DEV)
    with pytest.raises(ValueError, match="256"):
        ops.gptq_quantize(Wd, Ud, 3, 256)
    with pytest.raises(ValueError, match="32, 64 and 128"):
        ops.gptq_quantize(Wd, Ud, 3, 96)
    with pytest.raises(ValueError, match="K % 128"):
        ops.gptq_quantize(Wd[:, :192].contiguous(), Ud[:192, :192].contiguous(), 3, 64)
    with pytest.raises(ValueError, match="GPU"):
        ops.gptq_quantize(W, U, 3, 64)                                     # not on the GPU
    with pytest.raises(ValueError):
        ops.gptq_quantize(Wd, U, 3, 64)                                    # U not on W's device
    with pytest.raises(ValueError):
        ops.gptq_quantize(Wd, Ud.double(), 3, 64)
    bad = Wd.clone()
    bad[17, 130] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        ops.gptq_quantize(bad, Ud, 3, 64, name="q_proj")
    for value in (0.0, -1.0):
        Ub = Ud.clone()
        Ub[200, 200] = value
        W_q, scale, zero, row_loss, info, work = ops.gptq_quantize_buffers(48, 256, 3, 64, Wd.device)
        ops.gptq_quantize_launch(Wd, Ub, 3, 64, W_q, scale, zero, row_loss, info, work)
        assert int(info.cpu()[0]) == 1, f"U[200, 200] = {value} went unnoticed"
        with pytest.raises(ValueError, match="not finite"):
            ops.gptq_quantize(Wd, Ub, 3, 64)


def test_gptq_hinv_on_the_device():
    from amq_amd import ops
    f = fixture("gptqsolve_edge")
    acc = ops.GPTQHessian(f["X"].shape[1], DEV)
    for lo in range(0, f["X"].shape[0], 64):
        acc.add_batch(f["X"][lo:lo + 64].unsqueeze(0).to(DEV))
    U, dead, where = ops.gptq_hinv(acc.H, 0.01, return_where=True)
    OBSERVED["gptq_hinv_ran_on"] = where
    assert where in ("device", "host") and U.is_cuda and U.dtype == torch.float32
    assert torch.equal(dead.cpu(), f["dead"])
    assert torch.allclose(U.cpu().diagonal(), f["U"].diagonal(), rtol=1e-4, atol=0)


def _calibrated(true_sequential):
    from test_gpu_hf import _tiny_llama
    from amq_amd.arch import LINEARS
    from amq_amd.patching import quantize_model_gptq
    from amq_amd.quant_linear import HIPQuantLinear
    dense = _tiny_llama(2)
    cycle = (4, 2, 3, 3, 2, 4, 3)
    bits = {name: [cycle[(i + b) % 7] for b in range(2)] for i, name in enumerate(LINEARS)}       # a mixed per-linear assignment
    g = torch.Generator().manual_seed(5)
    prompts = torch.randint(0, 1000, (8, 8), generator=g).to(DEV)
    with torch.no_grad():
        text = dense.generate(prompts, min_new_tokens=56, max_new_tokens=56, do_sample=False, num_beams=1)      # 8 windows of 64 tokens
    samples = [text[i:i + 1].cpu() for i in range(8)]
    ours, report = quantize_model_gptq(copy.deepcopy(dense), {"linear": bits}, samples, true_sequential=true_sequential)
    assert len(report) == 14
    for b, layer in enumerate(ours.model.layers):
        for full in LINEARS:
            parent, attr = full.split(".")
            mod = getattr(getattr(layer, parent), attr)
            assert isinstance(mod, HIPQuantLinear) and mod.bits == bits[full][b] == report[(b, full)]["bits"], (b, full)
    worse = {k: (v["loss"], v["rtn_loss"]) for k, v in report.items() if not v["loss"] < v["rtn_loss"]}
    key = "tiny_llama_true_sequential" if true_sequential else "tiny_llama"
    OBSERVED[key] = {f"{b}.{n}": {k: v[k] for k in ("bits", "loss", "rtn_loss", "solver_loss", "dead")} for (b, n), v in report.items()}
    print(key, {f"{b}.{n}": round(v["loss"] / v["rtn_loss"], 3) for (b, n), v in report.items()})
    assert not worse, f"(loss, rtn_loss) of linears the solve did not improve: {worse}"
    return dense, ours, bits, prompts, text


def test_quantize_model_gptq_packs_generates_and_beats_round_to_nearest_per_linear():
    pytest.importorskip("transformers")
    from amq_amd import evaluate
    from amq_amd.arch import LINEARS
    from amq_amd.hqq_format import quantize_rtn
    from amq_amd.patching import HQQWeightsModule, prepare_for_inference, quantize_model_gptq
    dense, ours, bits, prompts, text = _calibrated(False)
    assert isinstance(ours.lm_head, torch.nn.Linear)
    with pytest.raises(TypeError):
        quantize_model_gptq(ours, 4, [text[:1].cpu()])                                             # already quantized
    prepare_for_inference(ours, backend="hip")
    with torch.no_grad():
        out = ours.generate(prompts[:2], min_new_tokens=6, max_new_tokens=6, do_sample=False, num_beams=1)
    assert out.shape == (2, 14)
    rtn = copy.deepcopy(dense)
    for b, layer in enumerate(rtn.model.layers):
        for full in LINEARS:
            parent, attr = full.split(".")
            lin = getattr(getattr(layer, parent), attr)
            setattr(getattr(layer, parent), attr, HQQWeightsModule(quantize_rtn(lin.weight.detach(), bits[full][b], 128)))
    prepare_for_inference(rtn, backend="hip")
    windows = [text[:4].cpu(), text[4:].cpu()]
    ppl_dense = float(np.exp(np.mean([torch.nn.functional.cross_entropy(dense(w.to(DEV)).logits[:, :-1].float().reshape(-1, 1000),
                                                                        w[:, 1:].reshape(-1).to(DEV)).item() for w in windows])))
    # recorded, not asserted: on a random tiny model the ordering is not guaranteed (eval_ppl: per-token perplexity to the 4th power, B = 4)
    OBSERVED["tiny_llama_ppl"] = {"dense": ppl_dense, "gptq_quantize": evaluate.eval_ppl(ours, None, windows, seqlen=64),
                                  "quantize_rtn": evaluate.eval_ppl(rtn, None, windows, seqlen=64)}
    print("perplexity:", OBSERVED["tiny_llama_ppl"])


def test_quantize_model_gptq_true_sequential():
    pytest.importorskip("transformers")
    _calibrated(True)


def test_zz_observed_parity_is_recorded():
    """last in the file: what the device gave in the tests above goes to profiles/gptq_quantize.json under "parity" (the timings of
    tools/gptq_bench.py live beside it)"""
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
