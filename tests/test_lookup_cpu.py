"""CPU-only: the prompt-lookup rules (tests/lookup_ref.py), the HF routing predicate, and the library's new entry points -- bindings and argument
validation before any GPU call."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_ref  # noqa: E402

from amq_amd import _lib, hf_fast  # noqa: E402


def test_propose_hand_worked():
    P = lookup_ref.propose
    assert P([1, 2, 3, 4], 3, 2) == [-1, -1, -1]                          # no match
    assert P([5, 1, 7, 9, 2, 1], 2, 2) == [7, 9]                          # only at g = 1 (the 2-gram (2, 1) occurs nowhere else)
    assert P([1, 2, 8, 8, 1, 2, 9, 9, 1, 2], 2, 2) == [9, 9]              # two matches: the most recent wins (HF would give 8, 8)
    assert P([3, 4, 6, 3, 4], 4, 2) == [6, 3, 4, -1]                      # the continuation is shorter than D
    assert P([1, 2, 3, 7, 7], 2, 3) == [7, -1]                            # g = 1 match directly in front of the suffix: one token follows
    assert P([4, 5, 6], 2, 3) == [-1, -1]                                 # the suffix matches only itself
    assert P([9], 3, 2) == [-1, -1, -1] and P([], 3, 2) == [-1, -1, -1]
    assert P([1, 2, 3, 1, 2, 4, 2], 2, 2) == [4, 2]                       # g = 2 has no earlier occurrence; g = 1: the latest 2 followed by a token
    assert P([7, 1, 2, 3, 9, 2, 3, 5, 1, 2, 3], 3, 3) == [9, 2, 3]        # the longer match beats the more recent shorter one


def test_accept_hand_worked():
    A = lookup_ref.accept
    assert A([5, 6, 7], [5, 6, 7, 8]) == (3, [5, 6, 7, 8])
    assert A([5, 6, 7], [4, 6, 7, 8]) == (0, [4])
    assert A([5, -1, 7], [5, 6, 7, 8]) == (1, [5, 6])                     # -1 never matches, and nothing behind it is looked at
    assert A([5, 6, 7], [5, 6, 0, 8]) == (2, [5, 6, 0])
    assert A([-1, -1], [3, 3, 3]) == (0, [3])


def test_propose_against_brute_force():
    rng = random.Random(1234)
    hits = 0
    for _ in range(400):
        L = rng.randint(0, 40)
        h = [rng.randrange(4) for _ in range(L)]
        D, g = rng.randint(1, 7), rng.randint(1, 4)
        got = lookup_ref.propose(h, D, g)
        assert got == lookup_ref.propose_brute(h, D, g), (h, D, g)
        assert len(got) == D
        hits += got[0] >= 0
    assert hits > 300                                                      # a 4-symbol alphabet: matches are the rule


def test_routing_predicate():
    R = hf_fast.lookup_request
    base = dict(max_new_tokens=16, min_new_tokens=16, do_sample=False, num_beams=1)
    assert R(dict(base, prompt_lookup_num_tokens=3), 1) == (3, 2)
    assert R(dict(base, prompt_lookup_num_tokens=7, max_matching_ngram_size=4), 1) == (7, 4)
    assert R(dict(base, prompt_lookup_num_tokens=1, max_matching_ngram_size=None), 1) == (1, 2)
    assert R(dict(prompt_lookup_num_tokens=3, max_new_tokens=4), 1) == (3, 2)
    assert R(dict(base, prompt_lookup_num_tokens=3), 1, enabled=False) is None
    assert R(dict(base, prompt_lookup_num_tokens=3), 2) is None            # batches
    assert R(dict(base, prompt_lookup_num_tokens=8), 1) is None
    assert R(dict(base, prompt_lookup_num_tokens=0), 1) is None
    assert R(dict(base, prompt_lookup_num_tokens=3, max_matching_ngram_size=5), 1) is None
    assert R(dict(base, prompt_lookup_num_tokens=3, max_matching_ngram_size=0), 1) is None
    assert R(dict(base, prompt_lookup_num_tokens=3.0), 1) is None
    assert R(dict(base, prompt_lookup_num_tokens=True), 1) is None
    assert R(dict(base, prompt_lookup_num_tokens=3, do_sample=True), 1) is None
    assert R(dict(base, prompt_lookup_num_tokens=3, num_beams=4), 1) is None
    assert R(dict(base, prompt_lookup_num_tokens=3, repetition_penalty=1.1), 1) is None
    assert R(dict(base), 1) is None


def test_new_symbols_bound():
    for name in ("amq_attn_decode_rows_f16", "amq_decode_tail_lookup_f16"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert _lib.load().amq_version() == 521


def test_entry_points_validate_before_any_gpu_call():
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    A = lib.amq_attn_decode_rows_f16
    ok = dict(rows=4, nh=32, nkv=32, hd=128, max_seq=256)
    call = lambda q=one, st=one, rows=4, nh=32, nkv=32, hd=128, max_seq=256, splits=0, ws=None, wsb=0, tk=None: \
        A(q, one, one, one, one, one, st, rows, nh, nkv, hd, max_seq, splits, ws, wsb, tk, None)
    assert call(q=None) == -1 and call(st=None) == -1
    for rows in (0, 1, 9, -3):
        assert call(rows=rows) == -2 and b"rows" in lib.amq_last_error()
    assert call(hd=64) == -2 and call(nkv=5) == -2 and call(max_seq=0) == -2
    assert call(splits=-1) == -1 and call(splits=2) == -1                   # split: workspace / tickets required
    assert call(splits=2, ws=one, wsb=16, tk=one) == -1 and b"workspace" in lib.amq_last_error()
    assert call(max_seq=1 << 20) == -2                                      # the single-workgroup form's score array
    T = lib.amq_decode_tail_lookup_f16
    tail = lambda logits=one, state=one, hist=one, rows=4, vocab=32000, hidden=4096, rope_rows=256, cap=256: \
        T(logits, vocab, one, hidden, one, one, one, one, rope_rows, rows, None, state, hist, cap, None)
    assert tail(logits=None) == -1 and tail(state=None) == -1 and tail(hist=None) == -1
    for rows in (0, 1, 9):
        assert tail(rows=rows) == -2 and b"rows" in lib.amq_last_error()
    assert tail(cap=255) == -2 and b"history_cap" in lib.amq_last_error()   # history_cap < max_seq
    assert tail(vocab=32001) == -2 and tail(hidden=4100) == -2 and tail(rope_rows=0) == -1
