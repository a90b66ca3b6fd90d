"""QuantLlama._rows_route: which kernels the walk of a prompt pass takes, as a table.  It reads FRAG_ROWS, fine, owq and ragged of the
runner and nothing else, so a stand-in object serves; the bytes of every route are tests/test_gpu_prompt_digests.py's."""
from types import SimpleNamespace

import pytest

from amq_amd.llama import DenseLlama, QuantLlama


def route(B, S, cache=True, **kw):
    r = SimpleNamespace(**{**dict(FRAG_ROWS=QuantLlama.FRAG_ROWS, fine=False, owq=False, ragged=False), **kw})
    return QuantLlama._rows_route(r, B, S, cache)


@pytest.mark.parametrize("S,want", [(1, "few"), (8, "few"), (9, "tiled"), (16, "tiled"), (17, "frag"), (384, "frag"), (385, "tiled")])
def test_one_prompt_into_the_cache_by_rows(S, want):
    assert route(1, S) == want


def test_everything_else_is_tiled():
    for S in (3, 40):
        assert route(2, S) == "tiled"                       # a batch, B * S <= 8 included
        assert route(1, S, ragged=True) == "tiled"
        assert route(1, S, cache=False) == "tiled"          # score_rows, prefill_batch
        assert DenseLlama._rows_route(None, 1, S, True) == "tiled"


def test_fine_groups_and_owq_layers_never_take_the_fragment_kernels():
    assert route(1, 40, fine=True) == route(1, 40, owq=True) == "tiled"
    assert route(1, 5, fine=True) == route(1, 5, owq=True) == "few"


def test_the_bounds_are_the_class_attribute_tools_set():
    assert route(1, 12, FRAG_ROWS=(8, 384)) == "frag" and route(1, 5, FRAG_ROWS=(0, 384)) == "frag" and route(1, 40, FRAG_ROWS=(0, 0)) == "tiled"
