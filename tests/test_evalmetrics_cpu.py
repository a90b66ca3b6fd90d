"""CPU-only: the fp64 restatement of the evaluation metrics (tests/evalmetrics_ref.py, what the GPU tests hold the kernels to) against values the
REFERENCE computed (tests/golden/evalmetrics.npz, written by tests/golden/gen_golden_evalmetrics.py); the new entry points' bindings and host-side
validation; the chunk arithmetic of QuantLlama.score_rows."""
import ctypes
import os

import numpy as np
import pytest
import torch

import evalmetrics_ref as ref
from amq_amd import _lib

# the reference evaluates in fp32: its own distance from fp64 was 4e-8 .. 4.4e-7 over V = 100 .. 152064 on the CPU; the golden shapes are small
JSD_TOL = 2e-6
PPL_RTOL = 1e-6


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "evalmetrics.npz"))


def test_restatement_reproduces_the_reference_windows(golden):
    ids = torch.from_numpy(golden["ids"])
    logits, dense = ref.f16(golden["logits"]), ref.f16(golden["dense"])
    seqlen = int(golden["seqlen"])
    assert logits.shape == (3, 1, 12, 500) and ids.shape == (3, 1, 12) and seqlen == 12
    nll = [ref.window_nll(logits[w], ids[w]) for w in range(3)]
    jsd = [ref.window_jsd(logits[w], dense[w]) for w in range(3)]
    ppl, loss = ref.ppl_of(nll, seqlen), ref.loss_of(jsd, seqlen)
    print("eval_ppl", ppl, float(golden["eval_ppl"]), "eval_loss", loss, float(golden["eval_loss"]))
    assert abs(ppl - float(golden["eval_ppl"])) <= PPL_RTOL * float(golden["eval_ppl"])
    assert abs(loss - float(golden["eval_loss"])) <= JSD_TOL
    # the scaling is the reference's: a window's MEAN over its B * (S - 1) rows times seqlen * B, whatever S is
    two = torch.stack([nll[0][0], nll[1][0]])                  # a window of B = 2
    assert abs(float(ref.window_value(two, 2048)) - float(two.mean()) * 2048 * 2) < 1e-9 * 2048
    assert abs(ref.ppl_of([two], 2048) - float(torch.exp(two.mean() * 2))) <= 1e-9 * ref.ppl_of([two], 2048)


@pytest.mark.parametrize("case", ["same", "wide", "near"])
def test_restatement_reproduces_the_reference_jsd(golden, case):
    p = ref.f16(golden[f"jsd_{case}_p"])
    q = p if case == "same" else ref.f16(golden[f"jsd_{case}_q"])
    got = float(ref.row_jsd(p, q).mean())                      # 'batchmean' over the rows
    want = float(golden[f"jsd_{case}"])
    print(case, got, want)
    assert abs(got - want) <= JSD_TOL
    if case == "same":
        assert want < 0.0 and got < 0.0                        # the clamp at eps is part of the definition
    if case == "wide":                                         # about two thirds of the mixture's entries sit under eps
        lp = p.double().log_softmax(-1).exp()
        lq = q.double().log_softmax(-1).exp()
        assert 0.5 < float((0.5 * (lp + lq) < 1e-7).double().mean()) < 0.8


def test_row_rules_of_the_restatement():
    x = torch.tensor([[1.0, 3.0, 3.0, -2.0], [0.5, 0.5, 0.5, 0.5]], dtype=torch.float16)
    assert ref.row_argmax(x).tolist() == [1, 0]                # the first maximum
    nll = ref.row_nll(x, torch.tensor([ref.IGNORE, 4]))
    assert float(nll[0]) == 0.0 and torch.isnan(nll[1])
    nll = ref.row_nll(x, torch.tensor([3, 0]))
    want = torch.nn.functional.cross_entropy(x.double(), torch.tensor([3, 0]), reduction="none")
    assert torch.allclose(nll, want, rtol=0, atol=1e-12)
    assert abs(float(ref.row_lse(x)[1]) - (0.5 + np.log(4.0))) < 1e-12


def test_new_symbols_are_bound():
    lib = _lib.load()
    for name in ("amq_logit_nll_f16", "amq_logit_jsd_f16"):
        assert name in _lib.SIGNATURES and getattr(lib, name).restype is ctypes.c_int
    assert lib.amq_version() == _lib.ABI_VERSION
    from amq_amd import ops
    assert callable(ops.logit_nll) and callable(ops.logit_jsd)


def test_host_side_validation_without_a_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    nll, jsd = lib.amq_logit_nll_f16, lib.amq_logit_jsd_f16
    assert nll(None, 100, one, 4, 100, one, None, None, None) == -1 and b"null" in lib.amq_last_error()
    assert nll(one, 100, one, 4, 100, None, one, one, None) == -1
    assert nll(one, 100, one, 0, 100, one, None, None, None) == -1 and b"M" in lib.amq_last_error()
    assert nll(one, 100, one, 4, 0, one, None, None, None) == -1 and b"V" in lib.amq_last_error()
    assert nll(one, 99, one, 4, 100, one, None, None, None) == -2 and b"stride" in lib.amq_last_error()
    assert jsd(None, 100, one, 100, 0, 4, 100, 1e-7, one, None) == -1
    assert jsd(one, 100, None, 100, 0, 4, 100, 1e-7, one, None) == -1
    assert jsd(one, 100, one, 100, 0, 4, 100, 1e-7, None, None) == -1
    assert jsd(one, 100, one, 100, 2, 4, 100, 1e-7, one, None) == -1 and b"q_is_f32" in lib.amq_last_error()
    assert jsd(one, 100, one, 100, 1, 0, 100, 1e-7, one, None) == -1
    assert jsd(one, 100, one, 100, 1, 4, 0, 1e-7, one, None) == -1
    assert jsd(one, 99, one, 100, 0, 4, 100, 1e-7, one, None) == -2 and b"p_stride" in lib.amq_last_error()
    assert jsd(one, 100, one, 50, 1, 4, 100, 1e-7, one, None) == -2 and b"q_stride" in lib.amq_last_error()
    from amq_amd import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.logit_nll(torch.zeros(2, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="GPU"):
        ops.logit_jsd(torch.zeros(2, 8, dtype=torch.float16), torch.zeros(2, 8))


def test_score_rows_chunk_arithmetic():
    from amq_amd.llama import QuantLlama, DenseLlama
    assert QuantLlama.SCORE_ROWS == 512 and DenseLlama.score_rows is QuantLlama.score_rows
    chunks = QuantLlama.score_chunks
    assert chunks(2048, 512) == [(0, 512), (512, 1024), (1024, 1536), (1536, 2047)]         # the last row of a window has no label
    assert chunks(50, 16) == [(0, 16), (16, 32), (32, 48), (48, 49)]
    assert chunks(17, 16) == [(0, 16)] and chunks(18, 16) == [(0, 16), (16, 17)] and chunks(2, 512) == [(0, 1)]
    for S, rows in ((2, 1), (5, 1), (33, 7), (2048, 512), (513, 512), (514, 512)):
        c = chunks(S, rows)
        assert c[0][0] == 0 and c[-1][1] == S - 1 and all(a[1] == b[0] for a, b in zip(c, c[1:]))
        assert all(0 < t1 - t0 <= rows for t0, t1 in c) and len(c) == -(-(S - 1) // rows)
    with pytest.raises(ValueError):
        chunks(1, 16)
    with pytest.raises(ValueError):
        chunks(8, 0)


def test_window_reductions_of_the_package_match_the_restatement():
    """evaluate.window_value and the two final reductions on CPU tensors: the package's plumbing, no GPU"""
    from amq_amd import evaluate
    rows = [torch.rand(2, 11, dtype=torch.float32) for _ in range(3)]
    vals = evaluate._gathered(None, [evaluate.window_value(r, 12) for r in rows])
    assert abs(float(torch.exp(vals.sum() / (3 * 12))) - ref.ppl_of(rows, 12)) <= 1e-12 * ref.ppl_of(rows, 12)
    assert abs(float(vals.sum() / (3 * 12)) - ref.loss_of(rows, 12)) <= 1e-12

    class Acc:
        def gather_for_metrics(self, x):
            return list(x) + list(x)                            # two processes' worth
    assert evaluate._gathered(Acc(), [evaluate.window_value(r, 12) for r in rows]).numel() == 6
    assert evaluate._gathered(object(), [evaluate.window_value(r, 12) for r in rows]).numel() == 3      # no gather_for_metrics: ignored
