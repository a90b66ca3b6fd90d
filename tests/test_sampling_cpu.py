"""CPU-only: the rules of sampled decoding (tests/sampling_ref.py, the fp64 restatement the GPU tests hold the kernel to) against transformers'
own logits warpers, the generator against Philox4x32-10's known answers, and the two new C-ABI entry points' argument validation."""
import ctypes

import numpy as np
import pytest

import sampling_ref as ref


def test_restatement_matches_hf_warpers():
    """temperature -> top-k -> top-p as HF applies them: the kept sets are equal, or HF's is a subset and every token it drops beyond ours has
    exactly the smallest kept logit (HF cuts inside the boundary tie class in sort order; here the class is kept whole)"""
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    differ = 0
    for vi, vocab in enumerate(ref.VOCABS):
        for si, scale in enumerate(ref.SCALES):
            logits = ref.logits_row(vocab, scale, seed=1000 + 10 * vi + si)
            for temperature, top_k, top_p in ref.GRID:
                kept, _, _ = ref.kept_set(logits, temperature, top_k, top_p)
                scores = torch.from_numpy(logits.astype(np.float64))[None]
                ids = torch.zeros(1, 1, dtype=torch.int64)
                if temperature != 1.0:
                    scores = lp.TemperatureLogitsWarper(temperature)(ids, scores)
                if top_k > 0:
                    scores = lp.TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=1)(ids, scores)
                if top_p < 1.0:
                    scores = lp.TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=1)(ids, scores)
                hf = torch.isfinite(scores[0]).numpy()
                if np.array_equal(hf, kept):
                    continue
                differ += 1
                assert not (hf & ~kept).any(), (vocab, scale, temperature, top_k, top_p, "HF keeps a token the rule drops")
                extra = kept & ~hf
                smallest = logits[kept].astype(np.float64).min()
                assert np.all(logits[extra].astype(np.float64) == smallest), (vocab, scale, temperature, top_k, top_p)
    assert differ <= 30          # (measured: 8 of 120; a rule that differed everywhere would not be HF's)


def test_kept_set_rules():
    logits = np.array([1.0, 3.0, 3.0, -np.inf, 2.0, np.nan, 0.0, 2.0], dtype=np.float16)
    kept, kept_k, d = ref.kept_set(logits, 1.0, 1, 1.0)
    assert kept.tolist() == [False, True, True, False, False, False, False, False]       # the tie with the maximum is kept whole
    kept, _, _ = ref.kept_set(logits, 1.0, 3, 1.0)
    assert kept.tolist() == [False, True, True, False, True, False, False, True]         # k-th value = 2.0: both 2.0s stay
    kept, _, _ = ref.kept_set(logits, 1.0, 0, 1.0, suppress=(1, 2, -1))
    assert kept.tolist() == [True, False, False, False, True, False, True, True]
    kept, _, d = ref.kept_set(logits, 1.0, 0, 0.5)
    assert d[1] == d[2] == 0.0 and kept.tolist() == [False, True, True, False, False, False, False, False]
    assert ref.draw(logits, 1.0, kept, 0.0) == 1 and ref.draw(logits, 1.0, kept, 0.49) == 1 and ref.draw(logits, 1.0, kept, 0.51) == 2
    assert ref.draw(logits, 1.0, kept, 1.0 - 2.0 ** -24) == 2


def test_philox_known_answers():
    assert ref.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    assert ref.philox4x32_10([ones] * 4, [ones] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert ref.uniform(0, 0, 0) == (0x6627E8D5 >> 8) * 2.0 ** -24
    us = [ref.uniform(7, d, s) for d in range(4) for s in range(3)]
    assert len(set(us)) == len(us) and all(0.0 <= u < 1.0 for u in us)


def test_abi_validation_without_gpu():
    from amq_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    rc = lib.amq_sample_f16(one, 1, 1000, None, None, None, one, None, 0, 0, None)
    assert rc == -1 and b"state" in lib.amq_last_error()
    assert lib.amq_sample_f16(one, 1, 0, one, None, None, one, None, 0, 0, None) == -1 and b"vocab" in lib.amq_last_error()
    assert lib.amq_sample_f16(one, 0, 1000, one, None, None, one, None, 0, 0, None) == -1 and b"rows" in lib.amq_last_error()
    assert lib.amq_sample_f16(one, 9, 1000, one, None, None, one, None, 0, 2, None) == -2          # EOS bookkeeping: 8 flags
    rc = lib.amq_decode_tail_sample_f16(one, 1000, one, 256, one, one, one, None, None, 0, 1, None, None, None)
    assert rc == -1 and b"state" in lib.amq_last_error()
    assert lib.amq_decode_tail_sample_f16(one, 0, one, 256, one, one, one, None, None, 0, 1, None, one, None) == -1
    assert lib.amq_decode_tail_sample_f16(one, 1000, one, 256, one, one, one, None, None, 0, 0, None, one, None) == -1
    assert lib.amq_decode_tail_sample_f16(one, 1000, one, 256, one, one, one, None, None, 0, 9, None, one, None) == -2
    assert lib.amq_version() == 521


def test_ops_range_checks():
    torch = pytest.importorskip("torch")
    from amq_amd import ops
    state = torch.zeros(32, dtype=torch.int32)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(eos_ids=list(range(9)))):
        with pytest.raises(ValueError, match="temperature|top_k|top_p|EOS"):
            ops.set_sampling_state(state, **bad)
