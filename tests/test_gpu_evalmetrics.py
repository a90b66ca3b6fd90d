"""The evaluation metrics on the GPU: the row kernels (amq_logit_nll_f16 / amq_logit_jsd_f16 through ops) against the fp64 restatement of
tests/evalmetrics_ref.py, their determinism, and the plumbing above them -- QuantLlama.score_rows, amq_amd.evaluate, the HF surface.

The bar, per row and case: |kernel - fp64| <= max(4 * e32, floor) with e32 the largest distance of torch's CPU fp32 evaluation of the same formula
from the same fp64 over the rows of the case (evalmetrics_ref: nll_expected / jsd_expected); arg-max is exact.  The kernel is never compared with
itself for accuracy -- only for determinism.  Shapes are chosen where the kernel can go wrong: fewer values than threads (V = 100), rows that are
only 2-byte aligned (V = 1001: the shifted-vector path with its value-by-value head and tail), the two real vocabularies; 1, 7 and 33 rows."""
import os

import numpy as np
import pytest
import torch

import evalmetrics_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATIOS = {}     # quantity -> largest observed |error| / bar (printed per test: run with -s to see them)


def _note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print(f"{name}: error / bar = {ratio:.3f} (largest so far {RATIOS[name]:.3f})")
    return ratio


def _case(V, M=33, std=3.0, seed=0):
    g = torch.Generator().manual_seed(1000 + V + seed)
    p = (torch.randn(M, V, generator=g) * std).to(torch.float16)
    q = (p.float() + 0.3 * torch.randn(M, V, generator=g)).to(torch.float16)
    labels = torch.randint(0, V, (M,), generator=g)
    return p, q, labels


def _check_nll(got, exp, tag):
    nll, lse, amax = got
    assert _note(f"nll[{tag}]", ref.worst_ratio(nll, exp["nll"], exp["nll_bar"])) <= 1.0
    assert _note(f"lse[{tag}]", ref.worst_ratio(lse, exp["lse"], exp["lse_bar"])) <= 1.0
    assert torch.equal(amax.cpu(), exp["argmax"])


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("V", [100, 1001, 32000, 152064])
def test_row_kernels_against_fp64_and_deterministic(V):
    from amq_amd import ops, _lib
    p, q, labels = _case(V)
    q32 = (q.float() + 1e-3 * torch.randn(q.shape, generator=torch.Generator().manual_seed(V))).contiguous()      # values fp16 cannot hold
    exp_nll = ref.nll_expected(p, labels)
    exp_j16, exp_j32 = ref.jsd_expected(p, q), ref.jsd_expected(p, q32)
    pd, qd, q32d, ld = p.to(DEV), q.to(DEV), q32.to(DEV), labels.to(DEV)
    full = ops.logit_nll(pd, ld)
    _check_nll(full, exp_nll, f"V={V}")
    j16, j32 = ops.logit_jsd(pd, qd), ops.logit_jsd(pd, q32d)
    assert _note(f"jsd fp16 q[V={V}]", ref.worst_ratio(j16, exp_j16["jsd"], exp_j16["jsd_bar"])) <= 1.0
    assert _note(f"jsd fp32 q[V={V}]", ref.worst_ratio(j32, exp_j32["jsd"], exp_j32["jsd_bar"])) <= 1.0
    # two launches: the same bits
    assert _same_bits(ops.logit_nll(pd, ld), full) and _same_bits([ops.logit_jsd(pd, qd), ops.logit_jsd(pd, q32d)], [j16, j32])
    # fewer rows: a launch of M rows gives the rows of the 33-row launch; a row launched alone -- in place, and copied to another address (for
    # V = 1001 another alignment) -- has the bits it has among the others
    for M in (1, 7):
        assert _same_bits(ops.logit_nll(pd[:M], ld[:M]), [t[:M] for t in full])
        assert _same_bits([ops.logit_jsd(pd[:M], qd[:M]), ops.logit_jsd(pd[:M], q32d[:M])], [j16[:M], j32[:M]])
    for r in (17, 32):
        assert _same_bits(ops.logit_nll(pd[r:r + 1], ld[r:r + 1]), [t[r:r + 1] for t in full])
        moved = torch.empty(V + 5, dtype=torch.float16, device=DEV)[5:].copy_(pd[r])[None]
        assert _same_bits(ops.logit_nll(moved, ld[r:r + 1]), [t[r:r + 1] for t in full])
        qmoved = torch.empty(V + 3, dtype=torch.float32, device=DEV)[3:].copy_(q32d[r])[None]
        assert _same_bits([ops.logit_jsd(moved, qmoved)], [j32[r:r + 1]])
    # the conservative-waits twin library computes the same
    with _lib.routed_to(_lib.open_twin()):
        twin = ops.logit_nll(pd, ld), ops.logit_jsd(pd, qd), ops.logit_jsd(pd, q32d)
    assert _same_bits(twin[0], full) and _same_bits(twin[1:], [j16, j32])
    # optional outputs
    lib = _lib.load()
    only = torch.empty(33, dtype=torch.float32, device=DEV)
    _lib.check(lib.amq_logit_nll_f16(_lib.ptr(pd), V, _lib.ptr(ld), 33, V, _lib.ptr(only), None, None, _lib.current_stream()))
    assert _same_bits([only], [full[0]])


def test_strided_rows_ignored_and_out_of_range_labels():
    from amq_amd import ops
    V, M = 1000, 7
    p, q, labels = _case(V, M)
    labels[2] = labels[5] = ref.IGNORE
    labels[4] = V                                              # one past the vocabulary: NaN for this row only, nothing read there
    exp = ref.nll_expected(p, labels)
    assert torch.isnan(exp["nll"][4]) and float(exp["nll"][2]) == 0.0
    # rows as a strided view: row stride V + 37, starting 3 values into the storage (rows 2-byte aligned, each at another alignment)
    store = torch.full((M, V + 37), float("nan"), dtype=torch.float16, device=DEV)
    view = store[:, 3:3 + V]
    view.copy_(p)
    qstore = torch.full((M, V + 11), float("nan"), dtype=torch.float32, device=DEV)
    qview = qstore[:, 1:1 + V]
    qview.copy_(q.float())
    assert view.stride(0) == V + 37 and not view.is_contiguous()
    got = ops.logit_nll(view, labels.to(DEV))
    _check_nll(got, exp, "strided")
    nll = got[0].cpu()
    assert torch.isnan(nll[4]) and int(torch.isnan(nll).sum()) == 1 and float(nll[2]) == 0.0 and float(nll[5]) == 0.0
    dense = ops.logit_nll(p.to(DEV), labels.to(DEV))
    assert _same_bits([t[[0, 1, 3, 6]] for t in got], [t[[0, 1, 3, 6]] for t in dense])     # the same bits as from dense rows
    assert torch.equal(got[2], dense[2])
    ej = ref.jsd_expected(p, q.float())
    j = ops.logit_jsd(view, qview)
    assert _note("jsd[strided]", ref.worst_ratio(j, ej["jsd"], ej["jsd_bar"])) <= 1.0
    assert _same_bits([j], [ops.logit_jsd(p.to(DEV), q.float().to(DEV))])
    # labels = None: every row counted out
    none = ops.logit_nll(view)
    assert float(none[0].abs().max()) == 0.0 and _same_bits(none[1:], got[1:])
    with pytest.raises(ValueError):
        ops.logit_nll(view.t())
    with pytest.raises(ValueError):
        ops.logit_jsd(view, qview[:, :-1])
    with pytest.raises(ValueError):
        ops.logit_nll(view.float())


def test_extreme_logits():
    from amq_amd import ops
    V = 1001
    big = 65504.0
    rows = torch.empty(5, V, dtype=torch.float16)
    rows[0] = 0.5                                              # all equal: lse = 0.5 + log V, arg-max 0
    rows[1] = torch.where(torch.arange(V) % 2 == 0, big, -big)  # the largest and the smallest finite values, mixed
    rows[2] = -big
    rows[2, 777] = big
    rows[3] = big
    rows[4] = torch.where(torch.arange(V) % 3 == 0, -big, big)  # first maximum at index 1
    labels = torch.tensor([10, 0, 777, 1000, 0])
    exp = ref.nll_expected(rows, labels)
    assert exp["argmax"].tolist() == [0, 0, 777, 0, 1]
    got = ops.logit_nll(rows.to(DEV), labels.to(DEV))
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    _check_nll(got, exp, "extreme")
    q = rows[[1, 0, 2, 4, 3]].contiguous()
    ej = ref.jsd_expected(rows, q)
    j = ops.logit_jsd(rows.to(DEV), q.to(DEV))
    assert bool(torch.isfinite(j).all())
    assert _note("jsd[extreme]", ref.worst_ratio(j, ej["jsd"], ej["jsd_bar"])) <= 1.0


@pytest.mark.parametrize("case", ["same", "wide", "near"])
def test_jsd_golden_cases(golden_dir, case):
    from amq_amd import ops
    g = np.load(os.path.join(golden_dir, "evalmetrics.npz"))
    p = ref.f16(g[f"jsd_{case}_p"])
    q = p if case == "same" else ref.f16(g[f"jsd_{case}_q"])
    for qq in (q, q.float()):
        e = ref.jsd_expected(p, qq)
        got = ops.logit_jsd(p.to(DEV), qq.to(DEV))
        assert _note(f"jsd[golden {case} {qq.dtype}]", ref.worst_ratio(got, e["jsd"], e["jsd_bar"])) <= 1.0
        # ... and the reference's own 'batchmean' value, at the tolerance its fp32 evaluation has (tests/test_evalmetrics_cpu.py)
        assert abs(float(got.double().mean()) - float(g[f"jsd_{case}"])) <= 2e-6
    if case == "same":
        assert float(got.max()) < 0.0                          # identical rows score slightly negative: the clamp is part of the definition


# ---------------------------------------------------------------- plumbing: score_rows, evaluate
def _runners(vocab, batch=1):
    from amq_amd import arch
    from amq_amd.llama import QuantLlama, DenseLlama
    cfg = dict(arch._cfg(2, 256, 512, 2, 1, 1, vocab=vocab))
    return QuantLlama(cfg, None, device=DEV, max_seq=64, seed=4, batch=batch), DenseLlama(cfg, device=DEV, max_seq=64, seed=5)


def _pass_logits(r, ids):
    """the runner's own all-logits rows for ``ids`` [B, S]: the prompt pass score_rows runs (no KV cache) through the all_logits finish"""
    B, S = ids.shape
    last = torch.empty(B, r.vocab, dtype=torch.float16, device=DEV)
    return r._logits_of_rows(r._rows_pass(ids.to(DEV), 0, cache=False), B, S, last)


@pytest.mark.parametrize("vocab", [1024, 1001])            # the fp16 GEMM lm_head, and the weight-streaming one (vocab % 16 != 0)
def test_score_rows_and_evaluate_end_to_end(vocab, monkeypatch):
    from amq_amd import ops, evaluate
    from amq_amd.llama import QuantLlama
    m, d = _runners(vocab)
    monkeypatch.setattr(QuantLlama, "SCORE_ROWS", 16)
    g = torch.Generator().manual_seed(vocab)
    S = 50
    windows = [torch.randint(0, vocab, (B, S), generator=g) for B in (1, 3, 1)]
    pos_before, tok_before = m.pos.clone(), m.token.clone()
    nll_rows, jsd_rows, dense_list, nll_bar, jsd_bar = [], [], [], ref.NLL_FLOOR, ref.JSD_FLOOR
    for w, ids in enumerate(windows):
        B = ids.shape[0]
        ours = _pass_logits(m, ids)                            # [B, S, vocab] fp16
        dense = _pass_logits(d, ids)
        dense = dense.float() if w == 1 else dense             # fp32 dense logits (the reference's FT forward), fp16 (HF's)
        dense = dense.cpu() if w == 2 else dense               # ... on the host: moved a piece at a time
        dense_list.append(dense if B > 1 else dense[0])        # [S, vocab] per window, as the reference's get_logits stacks them
        nll, jsd = m.score_rows(ids if B > 1 else ids[0], dense_logits=dense_list[-1])
        assert nll.shape == jsd.shape == (B, S - 1) and nll.dtype == jsd.dtype == torch.float32 and nll.is_cuda
        assert torch.equal(m.score_rows(ids), nll)             # (without dense logits: the same NLL)
        # the same rows through the kernels in ONE launch over the materialised logits: the same bits
        flat, dflat = ours[:, :-1].reshape(B * (S - 1), vocab), dense.to(DEV)[:, :-1].reshape(B * (S - 1), vocab)
        lab = ids[:, 1:].reshape(-1)
        assert torch.equal(ops.logit_nll(flat, lab.to(DEV))[0].view(B, S - 1), nll)
        assert torch.equal(ops.logit_jsd(flat, dflat).view(B, S - 1), jsd)
        # ... and within the bar of the fp64 restatement on those logits
        en, ej = ref.nll_expected(flat.cpu(), lab), ref.jsd_expected(flat.cpu(), dflat.cpu())
        assert _note(f"score_rows nll[vocab={vocab}]", ref.worst_ratio(nll.reshape(-1), en["nll"], en["nll_bar"])) <= 1.0
        assert _note(f"score_rows jsd[vocab={vocab}]", ref.worst_ratio(jsd.reshape(-1), ej["jsd"], ej["jsd_bar"])) <= 1.0
        nll_bar, jsd_bar = max(nll_bar, en["nll_bar"]), max(jsd_bar, ej["jsd_bar"])
        nll_rows.append(en["nll"].view(B, S - 1))
        jsd_rows.append(ej["jsd"].view(B, S - 1))
    assert torch.equal(m.pos, pos_before) and torch.equal(m.token, tok_before)      # decode state untouched
    # the two window reductions, with the reference's scaling (seqlen, not S - 1; times B)
    for seqlen in (S, 2048):
        ppl = evaluate.eval_ppl(m, None, windows, seqlen=seqlen)
        loss = evaluate.eval_loss(m, object(), windows, dense_list, seqlen=seqlen)
        want_ppl, want_loss = ref.ppl_of(nll_rows, seqlen), ref.loss_of(jsd_rows, seqlen)
        print("eval_ppl", ppl, want_ppl, "eval_loss", loss, want_loss)
        # sum / (n * seqlen) of per-window values that are (mean over rows) * seqlen * B: a mean of rows within the row bar is within it, and the
        # factor B (at most 3 here) scales it
        assert abs(np.log(ppl) - np.log(want_ppl)) <= 3 * nll_bar
        assert abs(loss - want_loss) <= 3 * jsd_bar
    with pytest.raises(ValueError):
        m.score_rows(torch.zeros(1, 65, dtype=torch.int64))    # longer than the RoPE table
    with pytest.raises(ValueError):
        m.score_rows(windows[0], dense_logits=torch.zeros(1, S, vocab + 1))


def test_score_rows_never_holds_a_window_of_logits():
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    V, S = 16384, 64
    m = QuantLlama(dict(arch._cfg(2, 256, 512, 2, 1, 1, vocab=V)), None, device=DEV, max_seq=S, seed=1)
    m.SCORE_ROWS = 16
    ids = torch.randint(0, V, (1, S), generator=torch.Generator().manual_seed(3)).to(DEV)
    dense = torch.randn(1, S, V, generator=torch.Generator().manual_seed(4)).to(torch.float16).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    nll, jsd = m.score_rows(ids, dense_logits=dense)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    window = 1 * S * V * 2                                     # the window's logits in fp16 alone
    print("peak bytes above the start", used, "of", window)
    assert used < window // 2
    assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(jsd).all())


# ---------------------------------------------------------------- the HF surface
def test_hf_forward_with_labels_needs_the_scoring_flag():
    pytest.importorskip("transformers")
    from amq_amd import hf_fast
    from test_gpu_hf_fast import _prepared
    model, _ = _prepared("llama")
    ids = torch.randint(0, 1000, (2, 24), generator=torch.Generator().manual_seed(5)).to(DEV)
    lab = ids.clone()
    lab[0, :5] = -100
    lab[1, 20] = -100
    try:
        hf_fast.convert_model_to_hip(model)
        with torch.inference_mode():
            with pytest.raises(ValueError, match="start_pos"):
                model(ids, start_pos=0, labels=lab)            # without the flag nothing changes
            plain = model(ids, start_pos=0, use_cache=False)
            hf_fast.convert_model_to_hip(model, scoring=True)
            out = model(ids, start_pos=0, labels=lab, use_cache=False)
        assert plain.loss is None and torch.equal(out.logits, plain.logits) and out.logits.dtype == torch.float32
        shifted, target = out.logits[:, :-1].reshape(-1, out.logits.shape[-1]), lab[:, 1:].reshape(-1)
        want = torch.nn.functional.cross_entropy(shifted.double(), target)
        # the mean of per-row values each within the NLL bar of fp64 (the returned fp32 logits hold the fp16 rows exactly)
        e = ref.nll_expected(shifted.cpu().to(torch.float16), target.cpu())
        assert out.loss.dim() == 0 and out.loss.dtype == torch.float32
        assert _note("hf loss", abs(float(out.loss) - float(want)) / e["nll_bar"]) <= 1.0
        assert abs(float(out.loss) - float(torch.nn.functional.cross_entropy(shifted, target))) <= 2 * e["nll_bar"]
        with torch.inference_mode(), pytest.raises(ValueError, match="start_pos"):
            model(ids, start_pos=3, labels=lab, use_cache=False)      # labels are served on a pass from position 0 only
    finally:
        hf_fast.revert_model_to_hf(model)
