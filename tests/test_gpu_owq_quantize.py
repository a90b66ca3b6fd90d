"""OWQ on the device (csrc/amq_owq.hip) against the host restatement of its arithmetic (tests/owq_ref.py).

The range search's score is the one place whose bits the host may miss (|d|^2.4 on the hardware's log2 / exp2, a fixed sum order), so it is held
to a criterion instead: the returned (scale, zero) are bit for bit the (d16, zp) of the returned candidate; that candidate's score, formed in fp64
on the host, is at most (1 + 1e-4) x the smallest fp64 score over all num x 2^bits candidates; the returned fp32 score is within 1e-4 relative of
the candidate's fp64 score.  Where 1e-4 comes from: about 2.4e-6 relative per term from a 1-ulp log2 / exp2 pair at |log2 d| <= 24, plus
L x 2^-24 for the sum at L <= 512, with a few times margin.

Everything else is basic IEEE fp32 arithmetic in a fixed order: ``owq_ref.solve(..., choices=the device's)`` replays the solve with the device's
(i, zp) per row and group and must reproduce codes, scale, zero, W_out and row_loss BIT FOR BIT, while every choice meets the criterion on the
replay's current values.  Then the layer, the column choice, and a calibrated HF model that generates.  What the device gives is printed and
written to profiles/owq_quantize.json ("parity")."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

import gptq_solver_ref as gref
import owq_ref as ref
from quantize_common import assert_codes, assert_format_a, same_bits
from test_owq_quantize_cpu import CASES, IDS, fixture, permuted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "owq_quantize.json")
OBSERVED = {"range_excess": 0.0, "score_error": 0.0, "wq_err_error": 0.0, "solve_choice_excess": 0.0}
TOL = 1e-4


def note(key, value):
    OBSERVED[key] = max(OBSERVED[key], float(value))


def meets_criterion(v, bits, choice, key, score=None):
    """the device's choice [N, 2] on the segments v fp32 [N, L]: (the candidates' fp64 scores, their steps)"""
    cand, least, d = ref.criterion(v, bits, choice.cpu())
    excess = float(((cand - least) / least.clamp(min=1e-300)).max())
    note(key, excess)
    assert bool((cand <= (1 + TOL) * least).all()), f"a choice misses the smallest fp64 score by {excess:.3g} relative"
    if score is not None:
        err = float(((score.cpu().double() - cand).abs() / cand.clamp(min=1e-300)).max())
        note("score_error", err)
        assert bool(((score.cpu().double() - cand).abs() <= TOL * cand).all()), f"the fp32 score is {err:.3g} relative from the candidate's"
    return cand, d


def weights(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).half()
    W[::5, ::11] *= 4.0
    return W


# ------------------------------------------------------------------------------------------------------------------ the range search
@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("K,col0,L", [(128, 0, 128), (128, 6, 122), (128, 64, 2), (256, 0, 256), (384, 0, 384)])
def test_range_search_meets_the_criterion(K, col0, L, bits):
    from amq_amd import ops
    W = weights(16, K, 3 * K + L + bits)
    scale, zero, info = ops.owq_range(W.to(DEV), bits, col0, L, return_info=True)
    assert scale.dtype == torch.float16 and zero.dtype == torch.float16 and tuple(scale.shape) == (16,) == tuple(zero.shape)
    assert info.choice.dtype == torch.int32 and tuple(info.choice.shape) == (16, 2) and info.score.dtype == torch.float32
    choice = info.choice.cpu()
    assert int(choice[:, 0].min()) >= 1 and int(choice[:, 0].max()) <= 40 and int(choice[:, 1].min()) >= 0 and int(choice[:, 1].max()) < 2 ** bits
    v = W[:, col0:col0 + L].float()
    _, d = meets_criterion(v, bits, choice, "range_excess", info.score)
    assert same_bits(scale.cpu(), d.to(torch.float16)), "scale is not the candidate's d16"
    assert same_bits(zero.cpu(), choice[:, 1].to(torch.float16)), "zero is not the candidate's zp"
    if col0 == 0 and L == K:
        _, wh = ref.deployed(v, d, choice[:, 1], float(2 ** bits - 1))
        want = ((v.double() - wh.double()) ** 2).sum(0)
        err = float(((info.wq_err.cpu().double() - want).abs() / want).max())
        note("wq_err_error", err)
        assert err <= TOL
    else:
        assert info.wq_err is None


def test_range_search_edges_and_refusals():
    from amq_amd import ops
    W = weights(16, 128, 9)
    W[0] = 0.0                                          # an all-zero row: the first candidate wins with a score of 0 at the 2^-24 floor
    W[1] = W[1].abs() + 0.004                           # all positive: 0 stays in the range
    scale, zero, info = ops.owq_range(W.to(DEV), 3, return_info=True)
    assert float(scale[0]) == 2.0 ** -24 and info.choice[0].tolist() == [1, 0] and float(info.score[0]) == 0.0
    meets_criterion(W.float(), 3, info.choice, "range_excess", info.score)
    again = ops.owq_range(W.to(DEV), 3)
    assert torch.equal(again[0], scale) and torch.equal(again[1], zero)
    bad = W.clone()
    bad[3, 17] = float("nan")
    with pytest.raises(ValueError, match="inf or NaN"):
        ops.owq_range(bad.to(DEV), 3)
    bad[3, 17] = float("inf")
    with pytest.raises(ValueError, match="inf or NaN"):
        ops.owq_range(bad.to(DEV), 3)
    with pytest.raises(ValueError, match="segment"):
        ops.owq_range(W.to(DEV), 3, 64, 128)
    with pytest.raises(ValueError, match="num"):
        ops.owq_range(W.to(DEV), 3, num=0)


# ------------------------------------------------------------------------------------------------------------------ the solve
@functools.lru_cache(maxsize=None)
def seeded(N, K, n_out):
    """(W_p fp16, U_p fp32, ids) of a shape beyond the fixtures: W and X from a seeded generator, a random set of outlier columns, U on the CPU"""
    from amq_amd import ops
    g = torch.Generator().manual_seed(N * 13 + K + n_out)
    W = weights(N, K, N + K + n_out)
    r = K // 8
    X = torch.randn(2 * K, r, generator=g) @ (torch.randn(r, K, generator=g) / r ** 0.5) + 0.3 * torch.randn(2 * K, K, generator=g)
    X[:, ::37] *= 10.0
    acc = ops.GPTQHessian(K, "cpu")
    for lo in range(0, 2 * K, 64):
        acc.add_batch(X[lo:lo + 64].half().unsqueeze(0))
    pick = torch.randperm(K, generator=g)
    ids = torch.cat([torch.sort(pick[n_out:])[0], pick[:n_out]])
    U, dead = ops.gptq_hinv(acc.H[ids][:, ids], 0.01)
    assert not bool(dead.any())
    return W[:, ids].contiguous(), U, ids, acc.H


def replayed(Wp, U, n_out, bits):
    """the device's result and the host's replay of it with the device's choices, compared bit for bit; every choice held to the criterion"""
    from amq_amd import ops
    N, K = Wp.shape
    Kp = ref.packed_columns(K, n_out)
    h, W_out, info = ops.owq_quantize(Wp.to(DEV), U.to(DEV), n_out, bits, return_info=True)
    assert_format_a(h, bits, 128, (N, Kp))
    assert info.nonfinite == 0 and info.choice.dtype == torch.int32 and tuple(info.choice.shape) == (N, Kp // 128, 2)
    assert W_out.dtype == torch.float16 and tuple(W_out.shape) == (N, n_out)
    want = ref.solve(Wp, U, n_out, bits, choices=info.choice.cpu())
    assert want["nonfinite"] == 0
    assert_codes(h, want["q"])
    assert same_bits(h.scale.cpu(), want["scale"]), "scale"
    assert same_bits(h.zero.cpu(), want["zero"]), "zero"
    assert same_bits(W_out.cpu(), want["W_out"]), "W_out"
    assert info.row_loss.dtype == torch.float32 and same_bits(info.row_loss.cpu(), want["row_loss"]), "row_loss"
    assert info.loss == pytest.approx(want["loss"], rel=1e-12)
    for g, seg in enumerate(want["segments"]):
        meets_criterion(seg, bits, info.choice[:, g], "solve_choice_excess")
    return h, W_out, info, want


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_fixtures_replay_bit_for_bit_and_the_loss_against_the_reference(name, bits):
    from amq_amd import ops
    f = fixture(name)
    Wp, U, ids, _, W0 = permuted(name, bits)
    n_out = int(f["n_out"])
    h, W_out, info, want = replayed(Wp, U, n_out, bits)
    N, K = Wp.shape
    Kp = ref.packed_columns(K, n_out)
    W_hat = ops.dequantize_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, N, Kp, 128).cpu().float()
    assert torch.equal(W_hat[:, :K - n_out], want["W_hat"]), "the error feedback saw another weight than the packed layer dequantizes to"
    assert bool((W_hat[:, K - n_out:] == 0).all()), "the padding columns do not dequantize to 0"
    dense = ref.unpermute(torch.cat([W_hat[:, :K - n_out], W_out.cpu().float()], 1), ids)
    ours = gref.proxy_loss(W0, dense, f["H"])
    theirs = gref.proxy_loss(W0, f[f"Q_b{bits}"], f["H"])
    OBSERVED[f"{name}_b{bits}"] = {"loss": ours, "reference_loss": theirs, "over_reference": ours / theirs, "solver_loss": info.loss}
    print(f"{name} b{bits}: device / reference {ours / theirs:.4f}")
    assert ours <= 1.05 * theirs


# one block without outliers; one block with a ragged group; a whole pass-through block; a ragged group and a pass-through block; several workgroups
# with N % 64 != 0 and a short tail; eleven blocks: long trailing chains
BEYOND = [(16, 128, 0), (16, 128, 2), (48, 256, 128), (80, 384, 130), (272, 512, 6), (64, 1408, 54)]


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("N,K,n_out", BEYOND)
def test_shapes_beyond_the_fixtures_replay_bit_for_bit(N, K, n_out, bits):
    Wp, U, _, _ = seeded(N, K, n_out)
    replayed(Wp, U, n_out, bits)


def test_run_to_run_and_a_replayed_graph_give_the_same_bits():
    from amq_amd import ops
    N, K, n_out, bits = 80, 384, 130, 3
    Wp, U, _, _ = seeded(N, K, n_out)
    W1, Ud = Wp.to(DEV), U.to(DEV)
    W2 = (W1.flip(0) * 1.5).half()
    eager = [ops.owq_quantize(w, Ud, n_out, bits, return_info=True) for w in (W1, W2)]
    h, W_out, info = ops.owq_quantize(W1, Ud, n_out, bits, return_info=True)
    assert torch.equal(h.W_q, eager[0][0].W_q) and torch.equal(h.scale, eager[0][0].scale) and torch.equal(h.zero, eager[0][0].zero)
    assert torch.equal(W_out, eager[0][1]) and torch.equal(info.row_loss, eager[0][2].row_loss) and torch.equal(info.choice, eager[0][2].choice)
    Wbuf = W1.clone()
    W_q, scale, zero, Wo, choice, row_loss, infob, _ = ops.owq_quantize_buffers(N, K, n_out, bits, 128, Wbuf.device)
    work = torch.empty((ref.workspace_bytes(N, K, n_out) + 3) // 4, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.owq_quantize_launch(Wbuf, Ud, n_out, bits, 128, 40, W_q, scale, zero, Wo, choice, row_loss, infob, work)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.owq_quantize_launch(Wbuf, Ud, n_out, bits, 128, 40, W_q, scale, zero, Wo, choice, row_loss, infob, work)
    for w, (eh, eo, ei) in ((W2, eager[1]), (W1, eager[0])):
        Wbuf.copy_(w)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(W_q, eh.W_q) and torch.equal(scale, eh.scale) and torch.equal(zero, eh.zero) and torch.equal(Wo, eo)
        assert torch.equal(row_loss, ei.row_loss) and torch.equal(choice, ei.choice) and int(infob.cpu()[0]) == 0


def test_refusals_and_the_nonfinite_flag():
    from amq_amd import ops
    Wp, U, _, _ = seeded(48, 256, 128)
    Wd, Ud = Wp.to(DEV), U.to(DEV)
    for group in (32, 64, 256):
        with pytest.raises(ValueError, match="groups of 128 only"):
            ops.owq_quantize(Wd, Ud, 128, 3, group)
    with pytest.raises(ValueError, match="n_out"):
        ops.owq_quantize(Wd, Ud, 5, 3)
    with pytest.raises(ValueError, match="n_out"):
        ops.owq_quantize(Wd, Ud, 256, 3)
    with pytest.raises(ValueError, match="GPU"):
        ops.owq_quantize(Wp, U, 128, 3)
    for col in (17, 200):                               # a quantized column; an outlier column
        bad = Wd.clone()
        bad[5, col] = float("nan")
        with pytest.raises(ValueError, match="not finite"):
            ops.owq_quantize(bad, Ud, 128, 3, name="q_proj")
    Ub = Ud.clone()
    Ub[100, 100] = 0.0
    with pytest.raises(ValueError, match="not finite"):
        ops.owq_quantize(Wd, Ub, 128, 3)


# ------------------------------------------------------------------------------------------------------------------ the column choice
@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_owq_select_returns_the_reference_s_columns(name, bits):
    from amq_amd import ops
    f = fixture(name)
    ids, out_ids = ops.owq_select(f["W"].to(DEV), f["H32"].to(DEV), int(f["n_out"]), bits)
    assert out_ids.dtype == torch.int32 and torch.equal(out_ids.cpu(), f[f"out_ids_b{bits}"])
    assert torch.equal(ids.cpu(), f[f"ids_b{bits}"])


# ------------------------------------------------------------------------------------------------------------------ the layer
@functools.lru_cache(maxsize=None)
def layer(which):
    """(HIPOWQLinear, the replay's dense matrix in the original column order) of the small fixture (64 x 256, n_out = 4, 3 bit) or of the seeded
    80 x 384 with n_out = 130 at 4 bit"""
    from amq_amd.quant_linear import HIPOWQLinear
    if which == "small":
        Wp, U, ids, _, _ = permuted("owqsolve_64x256_o4", 3)
        n_out, bits = 4, 3
    else:
        Wp, U, ids, _ = seeded(80, 384, 130)
        n_out, bits = 130, 4
    h, W_out, _, want = replayed(Wp, U, n_out, bits)
    return HIPOWQLinear.from_owq(h, W_out, ids.to(DEV)), ref.unpermute(want["dense_p"], ids)


@pytest.mark.parametrize("M", [1, 5, 16, 17, 200])
@pytest.mark.parametrize("which", ["small", "large"])
def test_layer_forward_against_an_fp64_matmul(which, M):
    mod, dense = layer(which)
    W = mod.dequantize()
    assert W.dtype == torch.float16 and same_bits(W.cpu(), dense.to(torch.float16)) and torch.equal(W.cpu().float(), dense)
    K, N = mod.infeatures, mod.outfeatures
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).half()
    y = mod(x.to(DEV))
    assert y.dtype == torch.float16 and tuple(y.shape) == (M, N)
    want = x.double() @ dense.double().t()
    tol = 1e-3 * want.abs() + 1e-3 * want.abs().max()              # the project's output parity (the smoke run's)
    assert bool(((y.cpu().double() - want).abs() <= tol).all()), float((y.cpu().double() - want).abs().max())
    lead = mod(x.to(DEV).reshape(1, M, K))                         # any leading dims
    assert tuple(lead.shape) == (1, M, N) and torch.equal(lead.reshape(M, N), y)


def test_layer_surface_state_dict_deepcopy_and_to():
    from amq_amd.quant_linear import HIPOWQLinear, HIPQuantLinear
    from amq_amd import ops
    mod, _ = layer("large")
    assert (mod.bits, mod.group_size, mod.infeatures, mod.outfeatures, mod.bias, mod.n_out) == (4, 128, 384, 80, None, 130)
    assert mod.perm.dtype == torch.int32 and tuple(mod.perm.shape) == (256,) and int((mod.perm < 0).sum()) == 2
    assert mod.out_ids.dtype == torch.int32 and bool((mod.out_ids[1:] > mod.out_ids[:-1]).all()) and tuple(mod.W_out.shape) == (80, 130)
    x = torch.randn(2, 3, 384, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    y = mod(x)
    assert tuple(y.shape) == (2, 3, 80)
    assert torch.equal(mod(x.float()), y.float())                  # other dtypes are cast, as HIPQuantLinear does
    twin = HIPOWQLinear(4, 128, 384, 80, 130).to(DEV)
    twin.load_state_dict(mod.state_dict())
    for other in (twin, copy.deepcopy(mod), copy.deepcopy(mod).to("cpu").to(DEV)):
        assert torch.equal(other(x), y) and torch.equal(other.dequantize(), mod.dequantize())
    broken = {k: v.clone() for k, v in mod.state_dict().items()}
    broken["out_ids"][0] = 384
    with pytest.raises(ValueError, match="outside"):
        HIPOWQLinear(4, 128, 384, 80, 130).to(DEV).load_state_dict(broken)
    xg = ops.owq_gather(x.reshape(-1, 384), mod.perm)              # the padding's gathered x is 0 whatever x holds: a 0 weight never meets an inf
    assert bool((xg[:, mod.perm < 0] == 0).all()) and torch.equal(xg[:, :254], x.reshape(-1, 384)[:, mod.perm[:254].long()])
    Wp, U, ids, _ = seeded(16, 128, 0)
    h, W_out = ops.owq_quantize(Wp.to(DEV), U.to(DEV), 0, 3)
    plain = HIPOWQLinear.from_owq(h, W_out, ids)
    assert type(plain) is HIPQuantLinear and W_out.numel() == 0


# ------------------------------------------------------------------------------------------------------------------ the model
def test_quantize_model_owq_packs_generates_and_beats_round_to_nearest_per_linear():
    pytest.importorskip("transformers")
    from test_gpu_hf import _tiny_llama
    from amq_amd.arch import LINEARS
    from amq_amd.hqq_format import quantize_rtn
    from amq_amd.patching import HQQWeightsModule, prepare_for_inference, quantize_model_gptq, quantize_model_owq
    from amq_amd.quant_linear import HIPOWQLinear
    dense = _tiny_llama(2)
    cycle = (4, 2, 3, 3, 2, 4, 3)
    bits = {name: [cycle[(i + b) % 7] for b in range(2)] for i, name in enumerate(LINEARS)}       # a mixed per-linear assignment
    g = torch.Generator().manual_seed(5)
    prompts = torch.randint(0, 1000, (8, 8), generator=g).to(DEV)
    with torch.no_grad():
        text = dense.generate(prompts, min_new_tokens=56, max_new_tokens=56, do_sample=False, num_beams=1)      # 8 windows of 64 tokens
    samples = [text[i:i + 1].cpu() for i in range(8)]
    ours, report = quantize_model_owq(copy.deepcopy(dense), {"linear": bits}, samples)
    assert len(report) == 14
    for b, block in enumerate(ours.model.layers):
        for full in LINEARS:
            parent, attr = full.split(".")
            mod = getattr(getattr(block, parent), attr)
            assert isinstance(mod, HIPOWQLinear) and mod.bits == bits[full][b] == report[(b, full)]["bits"], (b, full)
            assert mod.n_out == report[(b, full)]["n_out"] > 0 and torch.equal(mod.out_ids.cpu(), report[(b, full)]["out_ids"])
    worse = {k: (v["loss"], v["rtn_loss"]) for k, v in report.items() if not v["loss"] < v["rtn_loss"]}
    OBSERVED["tiny_llama"] = {f"{b}.{n}": {k: v[k] for k in ("bits", "n_out", "loss", "rtn_loss", "solver_loss", "dead")} for (b, n), v in report.items()}
    print({f"{b}.{n}": round(v["loss"] / v["rtn_loss"], 3) for (b, n), v in report.items()})
    assert not worse, f"(loss, rtn_loss) of linears the solve did not improve: {worse}"
    with pytest.raises(TypeError):
        quantize_model_owq(ours, 4, samples[:1])                                                   # already quantized
    with pytest.warns(RuntimeWarning, match="OWQ layers"):
        prepare_for_inference(ours, backend="hip")
    for block in ours.model.layers:
        for full in LINEARS:
            parent, attr = full.split(".")
            assert isinstance(getattr(getattr(block, parent), attr), HIPOWQLinear)
    with torch.no_grad():
        out = ours.generate(prompts[:2], min_new_tokens=6, max_new_tokens=6, do_sample=False, num_beams=1)
    assert out.shape == (2, 14)
    gptq, _ = quantize_model_gptq(copy.deepcopy(dense), {"linear": bits}, samples, true_sequential=True)
    rtn = copy.deepcopy(dense)
    for b, block in enumerate(rtn.model.layers):
        for full in LINEARS:
            parent, attr = full.split(".")
            lin = getattr(getattr(block, parent), attr)
            setattr(getattr(block, parent), attr, HQQWeightsModule(quantize_rtn(lin.weight.detach(), bits[full][b], 128)))
    prepare_for_inference(rtn, backend="hip")
    prepare_for_inference(gptq, backend="hip")
    windows = [text[:4], text[4:]]

    def ppl(model):
        with torch.no_grad():
            return float(np.exp(np.mean([torch.nn.functional.cross_entropy(model(w.to(DEV)).logits[:, :-1].float().reshape(-1, 1000),
                                                                           w[:, 1:].reshape(-1).to(DEV)).item() for w in windows])))

    # recorded, not asserted: on a random tiny model the ordering is not guaranteed (per-token perplexity under HF's own forward)
    OBSERVED["tiny_llama_ppl"] = {"dense": ppl(dense), "owq_quantize": ppl(ours), "gptq_quantize": ppl(gptq), "quantize_rtn": ppl(rtn)}
    print("perplexity:", OBSERVED["tiny_llama_ppl"])


def test_zz_observed_parity_is_recorded():
    """last in the file: what the device gave in the tests above goes to profiles/owq_quantize.json under "parity" (the timings of
    tools/owq_bench.py live beside it)"""
    if len(OBSERVED) <= 4:                  # (run alone: nothing to record)
        return
    try:
        doc = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        doc["parity"] = {"device": torch.cuda.get_device_name(0), "cases": OBSERVED}
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError as e:                    # a read-only checkout: the assertions above are what counts
        print("not recorded:", e)
