"""CPU-only: the sampled prompt-lookup tail's entry point (binding, export, one refused call per rule -- the style of tests/test_decode_entry_cpu.py),
the HF routing predicate with ``sampling=True``, and tests/lookup_sample_ref.py against its brute-force restatement."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_sample_ref  # noqa: E402

from amq_amd import _lib, hf_fast  # noqa: E402

EINVAL, ESHAPE = -1, -2
NAME = "amq_decode_tail_lookup_sample_f16"


def test_symbol_bound_and_exported():
    assert NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME][1]) == 18
    assert hasattr(_lib.load(), NAME)
    assert _lib.load().amq_version() == 521
    assert hasattr(_lib.open_twin(), NAME)          # the conservative-waits twin: the same sources


_ORDER = ("logits vocab embed hidden token step_states x rope_table rope_rows rows suppress_ids lookup_state history history_cap sample_state u_in "
          "kept_out stream").split()
_ONE = ctypes.c_void_p(256)         # a made-up pointer: every call below is refused before anything is launched
_OK = dict(logits=_ONE, vocab=32000, embed=_ONE, hidden=4096, token=_ONE, step_states=_ONE, x=_ONE, rope_table=_ONE, rope_rows=256, rows=4,
           suppress_ids=None, lookup_state=_ONE, history=_ONE, history_cap=256, sample_state=_ONE, u_in=None, kept_out=None, stream=None)
REFUSED = [
    ("sample_state null", dict(sample_state=None), EINVAL, b"sample_state"),
    ("sample_state null is answered before a shape error", dict(sample_state=None, rows=9, vocab=32001), EINVAL, b"sample_state"),
    ("lookup_state null", dict(lookup_state=None), EINVAL, b"lookup_state"),
    ("history null", dict(history=None), EINVAL, b"history"),
    ("logits null", dict(logits=None), EINVAL, b"null"),
    ("embed null", dict(embed=None), EINVAL, b"null"),
    ("token null", dict(token=None), EINVAL, b"null"),
    ("step_states null", dict(step_states=None), EINVAL, b"null"),
    ("x null", dict(x=None), EINVAL, b"null"),
    ("rope_table null (required)", dict(rope_table=None), EINVAL, b"null"),
    ("rope_rows 0", dict(rope_rows=0), EINVAL, b"rope_rows"),
    ("vocab 0", dict(vocab=0), ESHAPE, b"vocab"),
    ("vocab % 8", dict(vocab=32001), ESHAPE, b"vocab"),
    ("hidden 0", dict(hidden=0), ESHAPE, b"hidden"),
    ("hidden % 8", dict(hidden=4100), ESHAPE, b"hidden"),
    ("rows 0", dict(rows=0), ESHAPE, b"rows"),
    ("rows 1", dict(rows=1), ESHAPE, b"rows"),
    ("rows 9", dict(rows=9), ESHAPE, b"rows"),
    ("history_cap below rope_rows", dict(history_cap=255), ESHAPE, b"history_cap"),
    ("history_cap above 2^24", dict(rope_rows=256, history_cap=(1 << 24) + 1), ESHAPE, b"history_cap"),
]


@pytest.mark.parametrize("what,change,code,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_calls(what, change, code, word):
    lib = _lib.load()
    args = dict(_OK, **change)
    assert getattr(lib, NAME)(*[args[k] for k in _ORDER]) == code, what
    assert word in lib.amq_last_error(), (what, lib.amq_last_error())


def test_routing_predicate_with_sampling():
    R = hf_fast.lookup_request
    base = dict(max_new_tokens=16, min_new_tokens=16, num_beams=1, prompt_lookup_num_tokens=3)
    warped = dict(base, do_sample=True, temperature=0.8, top_k=20, top_p=0.9)
    assert R(warped, 1, sampling=True) == (3, 2)
    assert R(dict(base, do_sample=True), 1, sampling=True) == (3, 2)
    assert R(dict(warped, max_matching_ngram_size=4, prompt_lookup_num_tokens=7), 1, sampling=True) == (7, 4)
    assert R(dict(base, do_sample=False), 1, sampling=True) == (3, 2)          # greedy calls are served as before
    assert R(warped, 1, sampling=False) is None and R(warped, 1) is None
    assert R(dict(base, do_sample=True), 1, sampling=False) is None
    assert R(dict(base, do_sample=False, temperature=0.8), 1, sampling=False) is None      # (an unknown key without the flag)
    assert R(warped, 1, enabled=False, sampling=True) is None
    assert R(dict(warped, num_beams=4), 1, sampling=True) is None
    assert R(warped, 2, sampling=True) is None and R(warped, 0, sampling=True) is None
    assert R(dict(warped, repetition_penalty=1.1), 1, sampling=True) is None
    assert R(dict(warped, min_p=0.1), 1, sampling=True) is None
    assert R(dict(warped, prompt_lookup_num_tokens=8), 1, sampling=True) is None


def test_helper_against_brute_force():
    rng = random.Random(99)
    seen = set()
    for _ in range(400):
        D, g = rng.randint(1, 7), rng.randint(1, 4)
        hist = [rng.randrange(4) for _ in range(rng.randint(1, 30))]
        drawn = [rng.randrange(4) for _ in range(D + 1)]
        drafts = [rng.choice([drawn[i], drawn[i], rng.randrange(4), -1]) for i in range(D)]
        c = rng.choice([0, 5, (1 << 32) - 2, (1 << 64) - 3, rng.randrange(1 << 40)])
        ext = rng.random() < 0.2
        got = lookup_sample_ref.step(hist, drafts, drawn, D, g, ext, counter=c)
        assert got == lookup_sample_ref.step_brute(hist, drafts, drawn, D, g, ext, counter=c), (hist, drafts, drawn, D, g, ext, c)
        n, new, nxt, c2 = got
        assert new == hist + drawn[:n + 1] and len(nxt) == D and c2 == (c + n + 1) % (1 << 64)
        seen.add(n)
    assert {0, 1, 2, 3} <= seen
    # hand-worked: a -1 draft stops the acceptance; the counter crosses the 32-bit carry inside one step
    assert lookup_sample_ref.step([1, 2, 3], [10, -1, 12, 13], [10, 11, 12, 13, 14], 4, 2, counter=7)[::3] == (1, 9)
    assert lookup_sample_ref.step([1], [4, 5, 6], [4, 5, 6, 7], 3, 2, counter=(1 << 32) - 2)[3] == (1 << 32) + 2
