"""What a runner refuses, without building one (amq_amd/llama.py: runner_options, route_reasons -- host logic only).

(a) runner_options answers every combination of GRID as the constructor of the commit recorded in tests/golden/runner_options.json did: the same
message where it refused, acceptance where it went on to the device (tests/golden/gen_runner_options.py wrote the file from the constructor
itself).  (b) route_reasons gives, for model facts that break exactly one requirement of an A/B route, the message that constructor raised -- the
literals below are copied from its source --, in its order of precedence."""
import itertools
import json
import os
import string

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runner_options.json")
ACCEPTED = "accepted"
LETTERS = string.ascii_letters          # one per distinct outcome
GRID = dict(fuse=(False, True), config=("tiny-qwen3-test", "Llama-2-7b-hf"), batch=(0, 1, 2, 8, 9), ragged=(False, True), lookup=(0, 1, 7, 8),
            ngram_max=(0, 2, 4, 5), lookup_sampling=(False, True), kv_bits=(16, 8, 4), lm_head_bits=(16, 8, 4, 2), engine=(None, False, True))


def combinations():
    """(FUSE_QKV_ATTN, config name, the constructor's option keywords) over GRID, the last key fastest"""
    for values in itertools.product(*GRID.values()):
        kw = dict(zip(GRID, values))
        yield kw.pop("fuse"), kw.pop("config"), kw


def test_every_combination_as_recorded():
    from amq_amd.arch import MODEL_CONFIGS
    from amq_amd.llama import runner_options
    doc = json.load(open(GOLDEN))
    outcomes, grid = doc["outcomes"], doc["grid"]
    assert outcomes[0] == ACCEPTED and len(outcomes) == 23 and len(grid) == 46080
    seen, wrong = set(), []
    for (fuse, config, kw), letter in zip(combinations(), grid):
        want = outcomes[LETTERS.index(letter)]
        try:
            opts = runner_options(**kw, fuse_qkv_attn=fuse, qk_norm=MODEL_CONFIGS[config].get("qk_norm"))
            got = ACCEPTED
            assert (opts.B, opts.R, opts.engine) == (kw["batch"], kw["lookup"] + 1 if kw["lookup"] else kw["batch"], kw["engine"])
        except ValueError as e:
            got = str(e)
        seen.add(got)
        if got != want and len(wrong) < 5:
            wrong.append((fuse, config, kw, got, want))
    assert not wrong, f"not what commit {doc['commit'][:7]} answered (first few): {wrong}"
    assert seen == set(outcomes), "every recorded message is raised by some combination"
    assert grid.count(LETTERS[0]) == 552


# ---------------------------------------------------------------- (b) the two A/B routes
ENGINE, FUSE = "the decode engine", "the fused q/k/v + attention launch"
OWQ = (" does not serve a model with OWQ layers: their gather and outlier columns run as a stage launch in front of each packed GEMV "
       "(the five-launch step's staged plan)")
FINE = "the decode engine serves groups of 128"
NO_HEAD_NORM = " does not serve this model: it has no per-head q / k norm"
WIDTHS = " does not serve this model: q / o widths of heads * 128 = 512 != hidden_size 256"
ENGINE_GENERIC = "the decode engine needs batch 1 and max_seq <= 512"
SERVED = dict(R=1, ragged=False, kv_bits=16, fine=False, owq=False, has_bias=False, qk_norm=False, qd=4096, H=4096, max_seq=512)
QWEN3_WIDTHS = dict(qd=512, H=256)


def _reasons(route, **broken):
    from amq_amd.llama import route_reasons
    return route_reasons(route, **dict(SERVED, **broken))


@pytest.mark.parametrize("route", ["engine", "fuse_qkv_attn"])
def test_a_model_the_route_serves(route):
    assert _reasons(route) == []


@pytest.mark.parametrize("broken, first", [
    (dict(fine=True), FINE),
    (dict(owq=True), ENGINE + OWQ),
    (dict(qk_norm=True), ENGINE + NO_HEAD_NORM),
    (QWEN3_WIDTHS, ENGINE + WIDTHS),
    (dict(R=2), ENGINE_GENERIC),
    (dict(max_seq=513), ENGINE_GENERIC),
    (dict(has_bias=True), ENGINE_GENERIC),
    (dict(ragged=True), ENGINE_GENERIC),
    (dict(kv_bits=8), ENGINE_GENERIC),
], ids=lambda v: "-".join(v) if isinstance(v, dict) else None)
def test_engine_reason(broken, first):
    assert _reasons("engine", **broken)[0] == first


@pytest.mark.parametrize("broken, first", [
    (dict(owq=True), FUSE + OWQ),
    (dict(qk_norm=True), FUSE + NO_HEAD_NORM),
    (QWEN3_WIDTHS, FUSE + WIDTHS),
], ids=lambda v: "-".join(v) if isinstance(v, dict) else None)
def test_fused_launch_reason(broken, first):
    assert _reasons("fuse_qkv_attn", **broken) == [first]


@pytest.mark.parametrize("broken", [dict(R=2), dict(max_seq=513), dict(H=8320, qd=8320), dict(fine=True), dict(has_bias=True), dict(ragged=True),
                                    dict(kv_bits=8)], ids=lambda v: "-".join(v))
def test_fused_launch_where_it_merely_does_not_fit(broken):
    """FUSE_QKV_ATTN on such a runner raised nothing and left can_fuse_qkv_attn False: the one reason is the line _take_routes never raises"""
    from amq_amd.llama import FUSE_UNFIT
    assert _reasons("fuse_qkv_attn", **broken) == [FUSE_UNFIT]


@pytest.mark.parametrize("route, what", [("engine", ENGINE), ("fuse_qkv_attn", FUSE)])
def test_owq_wins_over_the_qwen3_shape(route, what):
    assert _reasons(route, owq=True, qk_norm=True, **QWEN3_WIDTHS) == [what + OWQ, what + NO_HEAD_NORM]


def test_engine_generic_message_alone_and_last():
    assert _reasons("engine", has_bias=True, R=2) == [ENGINE_GENERIC]
    assert _reasons("engine", fine=True, owq=True, R=8) == [FINE, ENGINE + OWQ, ENGINE_GENERIC]
