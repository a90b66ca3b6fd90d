"""ops.gptq_quantize(..., perm=..., static_groups=True) -- GPTQ's solve with an activation order and static groups as HIP kernels
(csrc/amq_gptq_static.hip) -- against the torch restatement of its arithmetic (tests/gptq_static_ref.py): codes, scale, zero and
the rows' losses BIT FOR BIT (every operation is a basic IEEE fp32 operation in a fixed order, so no tolerance is granted), on the reference's
fixtures (tests/golden/gptqact_*.npz) and on the shapes and orders where this kernel can go wrong; the packed layer dequantizes to the weights the
error feedback saw; the refusals fire before any launch; and through every layer above it up to a calibrated, packed HF model that generates
and is evaluated, with a lower summed layer loss than the default call's on the same model and samples."""
import copy

import pytest
import torch

import gptq_static_ref as ref
from quantize_common import assert_codes, assert_format_a, same_bits
from test_gptq_actorder_cpu import CASES, IDS, fixture, restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_SEEDED = {}


def perm_of(kind, K, group):
    if kind == "identity":                       # static groups alone
        return torch.arange(K)
    if kind == "reversal":
        return torch.arange(K - 1, -1, -1)
    i = torch.arange(K)                          # interleave: a lane's 8 walk columns lie in different groups, every block crosses all groups
    return (i % (K // group)) * group + i // (K // group)


def seeded(N, K, group, bits, kind):
    """(W fp16, U_p fp32, perm, the restatement) of a shape beyond the fixtures: W and X from a seeded generator, the factor of the permuted
    Hessian on the CPU; computed once"""
    key = (N, K, group, bits, kind)
    if key not in _SEEDED:
        from amq_amd import ops
        g = torch.Generator().manual_seed(N * 13 + K + group + bits)
        W = (torch.randn(N, K, generator=g) * 0.02).half()
        W[::5, ::11] *= 4.0
        r = max(K // 8, 1)
        X = torch.randn(2 * K, r, generator=g) @ (torch.randn(r, K, generator=g) / r ** 0.5) + 0.3 * torch.randn(2 * K, K, generator=g)
        X[:, ::37] *= 10.0
        acc = ops.GPTQHessian(K, "cpu")
        for lo in range(0, 2 * K, 64):
            acc.add_batch(X[lo:lo + 64].half().unsqueeze(0))
        perm = ops.gptq_act_order(acc.H) if kind == "act_order" else perm_of(kind, K, group)
        U, dead = ops.gptq_hinv(acc.H[perm][:, perm], 0.01)
        assert not bool(dead.any())
        _SEEDED[key] = (W, U, perm, ref.solve(W, U, perm, bits, group, deploy=True))
    return _SEEDED[key]


def identical(h, info, want, nbits, group, shape):
    """codes, scale, zero and row_loss of a device result equal the restatement's, bit for bit; Format A's shapes and dtypes"""
    N = shape[0]
    assert_format_a(h, nbits, group, shape)
    assert info.nonfinite == 0 and want["nonfinite"] == 0
    assert same_bits(h.scale.cpu(), want["scale"]), "scale"
    assert same_bits(h.zero.cpu(), want["zero"]), "zero"
    assert_codes(h, want["q"])
    assert info.row_loss.dtype == torch.float32 and tuple(info.row_loss.shape) == (N,)
    assert same_bits(info.row_loss.cpu(), want["row_loss"]), "row_loss"
    assert info.loss == pytest.approx(want["loss"], rel=1e-12)         # (fp64 sums of the same fp32 values, in the device's and the host's order)


def dequantized(h, nbits, group):
    from amq_amd import ops
    N, K = h.shape
    return ops.dequantize_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), nbits, N, K, group).cpu()


@pytest.mark.parametrize("name,bits", CASES, ids=IDS)
def test_fixtures_bit_for_bit_and_the_loss_against_the_reference(name, bits):
    from amq_amd import ops
    import gptq_solver_ref as plain
    f = fixture(name)
    group = int(f["group"])
    want = restated(name, bits, True)
    h, info = ops.gptq_quantize(f["W"].to(DEV), f["U_p"].to(DEV), bits, group, return_info=True, perm=f["perm"].to(DEV), static_groups=True)
    identical(h, info, want, bits, group, f["W"].shape)
    W_hat = dequantized(h, bits, group)
    assert torch.equal(W_hat.float(), want["W_hat"]), "the error feedback saw another weight than the packed layer dequantizes to"
    ours = plain.proxy_loss(f["W"], W_hat, f["H"])
    theirs = plain.proxy_loss(f["W"], f[f"Q_b{bits}"], f["H"])
    flat = plain.proxy_loss(f["W"], f[f"Qplain_b{bits}"], f["H"])
    print(f"{name} b{bits}: device / reference {ours / theirs:.4f}, device / the reference's plain result {ours / flat:.4f}")
    assert ours <= 1.05 * theirs


# one workgroup and no left-looking tile; many tiles and three workgroups -- under the identity (static groups alone), the reversal and the
# interleave; then finer groups and an activation order over several workgroups with N % 64 != 0
BEYOND = [(N, K, 128, bits, kind) for (N, K, bits) in ((16, 128, 4), (48, 1024, 3)) for kind in ("identity", "reversal", "interleave")] + [
    (48, 256, 32, 2, "interleave"), (48, 256, 64, 3, "reversal"), (80, 384, 64, 4, "act_order"), (272, 384, 128, 2, "act_order")]


@pytest.mark.parametrize("N,K,group,bits,kind", BEYOND)
def test_shapes_and_orders_beyond_the_fixtures_bit_for_bit(N, K, group, bits, kind):
    from amq_amd import ops
    W, U, perm, want = seeded(N, K, group, bits, kind)
    kw = {} if kind == "identity" else {"perm": perm.to(DEV)}                # (static_groups without perm: the identity)
    h, info = ops.gptq_quantize(W.to(DEV), U.to(DEV), bits, group, return_info=True, static_groups=True, **kw)
    identical(h, info, want, bits, group, (N, K))
    assert torch.equal(dequantized(h, bits, group).float(), want["W_hat"])
    if kind == "identity":
        again = ops.gptq_quantize(W.to(DEV), U.to(DEV), bits, group, static_groups=True, perm=perm.to(torch.int32).to(DEV))
        assert torch.equal(again.W_q, h.W_q) and torch.equal(again.scale, h.scale) and torch.equal(again.zero, h.zero)


def test_run_to_run_and_the_conservative_twin_give_the_same_bytes():
    from amq_amd import _lib, ops
    W, U, perm, _ = seeded(272, 384, 128, 2, "act_order")
    Wd, Ud, pd = W.to(DEV), U.to(DEV), perm.to(DEV)
    h, info = ops.gptq_quantize(Wd, Ud, 2, 128, return_info=True, perm=pd, static_groups=True)
    again, info2 = ops.gptq_quantize(Wd, Ud, 2, 128, return_info=True, perm=pd, static_groups=True)
    with _lib.routed_to(_lib.open_twin()):
        twin, info3 = ops.gptq_quantize(Wd, Ud, 2, 128, return_info=True, perm=pd, static_groups=True)
    for other, i in ((again, info2), (twin, info3)):
        assert torch.equal(other.W_q, h.W_q) and torch.equal(other.scale, h.scale) and torch.equal(other.zero, h.zero)
        assert torch.equal(i.row_loss, info.row_loss)


def test_the_defaults_are_the_plain_solve():
    from amq_amd import ops
    from test_gpu_gptq_quantize import seeded as plain_seeded
    W, U, want = plain_seeded(48, 256, 64, 3)
    h = ops.gptq_quantize(W.to(DEV), U.to(DEV), 3, 64, perm=None, static_groups=False)
    assert_codes(h, want["q"])
    assert same_bits(h.scale.cpu(), want["scale"]) and same_bits(h.zero.cpu(), want["zero"])


def test_refusals_fire_before_any_launch(monkeypatch):
    from amq_amd import ops
    W, U, perm, _ = seeded(48, 256, 64, 3, "reversal")
    Wd, Ud, pd = W.to(DEV), U.to(DEV), perm.to(DEV)
    launched = []
    monkeypatch.setattr(ops, "gptq_quantize_static_launch", lambda *a, **k: launched.append("static"))
    monkeypatch.setattr(ops, "gptq_quantize_launch", lambda *a, **k: launched.append("plain"))
    twice = pd.clone()
    twice[5] = twice[6]
    for label, bad in (("a repeated entry", twice), ("an entry of K", pd + 1), ("a negative entry", pd - 1), ("too short", pd[:-1]),
                       ("two-dimensional", pd.reshape(2, -1))):
        with pytest.raises(ValueError, match="perm"):
            ops.gptq_quantize(Wd, Ud, 3, 64, perm=bad, static_groups=True)
        assert not launched, label
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.gptq_quantize(Wd, Ud, 3, 64, perm=pd.float(), static_groups=True)
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.gptq_quantize(Wd, Ud, 3, 64, perm=pd.to(torch.int16), static_groups=True)
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.gptq_quantize(Wd, Ud, 3, 64, perm=perm.tolist(), static_groups=True)
    with pytest.raises(ValueError, match="W's GPU"):
        ops.gptq_quantize(Wd, Ud, 3, 64, perm=perm, static_groups=True)                       # perm on the host
    with pytest.raises(NotImplementedError, match="Format A"):
        ops.gptq_quantize(Wd, Ud, 3, 64, perm=pd)
    with pytest.raises(ValueError, match="256"):
        ops.gptq_quantize(Wd, Ud, 3, 256, perm=pd, static_groups=True)
    assert not launched


def test_an_entry_outside_the_columns_sets_the_flag():
    """the bare entry point cannot read perm: an entry outside 0 .. K - 1 is read as column 0 and reported through the info word"""
    from amq_amd import ops
    W, U, perm, _ = seeded(48, 256, 64, 3, "reversal")
    Wd, Ud = W.to(DEV), U.to(DEV)
    bad = perm.to(torch.int32).to(DEV)
    bad[9] = 256
    W_q, scale, zero, row_loss, info, work = ops.gptq_quantize_static_buffers(48, 256, 3, 64, Wd.device)
    ops.gptq_quantize_static_launch(Wd, Ud, bad, 3, 64, W_q, scale, zero, row_loss, info, work)
    assert int(info.cpu()[0]) == 1
    with pytest.raises(ValueError, match="perm"):                                             # ... and ops.gptq_quantize never gets that far
        ops.gptq_quantize(Wd, Ud, 3, 64, perm=bad, static_groups=True)


def test_quantize_model_gptq_act_order_packs_generates_evaluates_and_lowers_the_loss():
    pytest.importorskip("transformers")
    from test_gpu_hf import _tiny_llama
    from amq_amd import evaluate
    from amq_amd.arch import LINEARS
    from amq_amd.llama import QuantLlama
    from amq_amd.patching import prepare_for_inference, quantize_model_gptq
    from amq_amd.quant_linear import HIPQuantLinear
    dense = _tiny_llama(2)
    g = torch.Generator().manual_seed(11)
    samples = [torch.randint(0, 1000, (1, 32), generator=g) for _ in range(6)]             # a few 32-token windows
    default, rep0 = quantize_model_gptq(copy.deepcopy(dense), 2, samples)
    ours, rep1 = quantize_model_gptq(copy.deepcopy(dense), 2, samples, act_order=True, static_groups=True)
    assert set(rep0) == set(rep1) and len(rep1) == 14
    assert all(v["act_order"] and v["static_groups"] and v["bits"] == 2 for v in rep1.values())
    assert not any(v["act_order"] or v["static_groups"] for v in rep0.values())
    total0, total1 = sum(v["loss"] for v in rep0.values()), sum(v["loss"] for v in rep1.values())
    print(f"summed layer loss: act-order + static groups {total1:.6g}, default {total0:.6g}, ratio {total1 / total0:.4f}")
    assert total1 < total0
    with pytest.raises(NotImplementedError, match="Format A"):
        quantize_model_gptq(copy.deepcopy(dense), 2, samples, act_order=True)
    for layer in ours.model.layers:
        for full in LINEARS:
            parent, attr = full.split(".")
            assert isinstance(getattr(getattr(layer, parent), attr), HIPQuantLinear)
    prepare_for_inference(ours, backend="hip")
    r = QuantLlama.from_hf(ours, max_seq=64)
    out = r.generate(samples[0][0, :8].to(DEV), 6)
    assert out.numel() == 6
    windows = [torch.cat(samples[:3]), torch.cat(samples[3:])]
    ppl = evaluate.eval_ppl(ours, None, windows, seqlen=32)
    assert ppl == ppl and 0 < ppl < float("inf")
    print("perplexity (random tiny model, recorded only):", ppl)
