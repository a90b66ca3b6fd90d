"""CPU-only: which kernel a grouped GEMV launch takes (amq_gemv_route, include/amq_hip.h) and the order its segments run in
(amq_gemv_segment_order).  Host logic of launch_gemv, exported so that it can be asserted without a device: the keyed kernels (bit-widths
fixed at compile time) serve the one-row launches of a 7B-class decode step and nothing else."""
import itertools

import pytest

from amq_amd import _lib, ops

KEYED, GENERIC = _lib.GEMV_ROUTE_KEYED, _lib.GEMV_ROUTE_GENERIC
H, I = 4096, 11008

# the five one-row launch forms of the headline step: (prologue, K, segments)
FORMS = [("qkv", ops.PRO_RMSNORM, H, 3), ("o_proj", ops.PRO_NONE, H, 1), ("gate_up", ops.PRO_RMSNORM, H, 2), ("down_mul", _lib.PRO_MUL, I, 1),
         ("down_silu_mul", ops.PRO_SILU_MUL, I, 1)]


@pytest.mark.parametrize("name,pro,k,nseg", FORMS, ids=[f[0] for f in FORMS])
def test_headline_launch_forms_are_keyed_in_every_order(name, pro, k, nseg):
    for bits in itertools.product((2, 3, 4), repeat=nseg):
        assert ops.gemv_route(pro, 1, k, list(bits)) == KEYED, (name, bits)
        # the A/B switch sends the same launch to the generic kernel
        assert ops.gemv_route(pro, 1, k, list(bits), opts=ops.GemvOpts(depth=_lib.GEMV_DEPTH_GENERIC)) == GENERIC, (name, bits)


def test_waves_decide_with_the_geometry():
    # what the launch picks itself: 4 waves below K = 2048 (generic), 8 up to 4096, 16 beyond
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, 1024, [3, 3, 3]) == GENERIC
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, 2048, [3, 3, 3]) == KEYED
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, 1024, [3, 3, 3], opts=ops.GemvOpts(waves=8)) == KEYED
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, 256, [2, 4], opts=ops.GemvOpts(waves=8)) == KEYED
    assert ops.gemv_route(ops.PRO_NONE, 1, 256, [4], opts=ops.GemvOpts(waves=8)) == KEYED
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [3, 3, 3], opts=ops.GemvOpts(waves=16)) == GENERIC
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [3, 3, 3], opts=ops.GemvOpts(waves=4)) == GENERIC
    assert ops.gemv_route(_lib.PRO_MUL, 1, 1408, [3]) == GENERIC
    assert ops.gemv_route(_lib.PRO_MUL, 1, 1408, [3], opts=ops.GemvOpts(waves=16)) == KEYED
    assert ops.gemv_route(ops.PRO_SILU_MUL, 1, 1408, [3], opts=ops.GemvOpts(waves=16)) == KEYED
    assert ops.gemv_route(_lib.PRO_MUL, 1, I, [3], opts=ops.GemvOpts(waves=8)) == GENERIC
    assert ops.gemv_route(_lib.PRO_MUL, 1, 16384, [3]) == KEYED


# every excluded case: one assertion each
def test_rows_beyond_one_are_generic():
    for m in (2, 4, 5, 8, 9, 16):
        assert ops.gemv_route(ops.PRO_RMSNORM, m, H, [2, 3, 4]) == GENERIC, m


def test_fma_segments_are_generic():
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [2, 3, 4], modes=[ops.MODE_FMA] * 3) == GENERIC


def test_fma1_segments_are_generic():
    assert ops.gemv_route(ops.PRO_NONE, 1, H, [4], modes=[ops.MODE_FMA1]) == GENERIC


def test_mixed_modes_are_generic():
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [2, 3, 4], modes=[ops.MODE_HQQ, ops.MODE_FMA, ops.MODE_HQQ]) == GENERIC
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [3, 3], modes=[ops.MODE_HQQ, ops.MODE_FMA1]) == GENERIC


def test_groups_of_64_are_generic():
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [2, 3, 4], group=64) == GENERIC


def test_groups_of_32_are_generic():
    assert ops.gemv_route(ops.PRO_NONE, 1, H, [4], group=32) == GENERIC


def test_group_scale_math_is_generic():
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [2, 3, 4], opts=ops.GemvOpts(math=ops.MATH_GROUPSCALE)) == GENERIC


def test_linear_math_is_generic():
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [2, 3, 4], opts=ops.GemvOpts(math=ops.MATH_LINEAR)) == GENERIC


def test_dot_math_is_generic():
    assert ops.gemv_route(ops.PRO_NONE, 1, H, [4], opts=ops.GemvOpts(dot=1)) == GENERIC


def test_two_chunk_kernels_are_generic():
    for k in (4224, 5120, 8192):                    # 4096 < K <= 8192: 8 waves, two x chunks per thread
        assert ops.gemv_route(ops.PRO_RMSNORM, 1, k, [2, 3, 4]) == GENERIC, k
        assert ops.gemv_route(ops.PRO_NONE, 1, k, [4]) == GENERIC, k
        assert ops.gemv_route(ops.PRO_RMSNORM, 1, k, [2, 3, 4], opts=ops.GemvOpts(waves=8)) == GENERIC, k
        assert ops.gemv_route(_lib.PRO_MUL, 1, k, [3]) == GENERIC, k
        assert ops.gemv_route(ops.PRO_SILU_MUL, 1, k, [3]) == GENERIC, k
        assert ops.gemv_route(_lib.PRO_MUL, 1, k, [3], opts=ops.GemvOpts(waves=16)) == KEYED, k     # (16 waves asked for: the two-chunk 16-wave geometry)


def test_k_beyond_16384_is_generic():
    assert ops.gemv_route(_lib.PRO_MUL, 1, 28672, [3]) == GENERIC
    assert ops.gemv_route(ops.PRO_SILU_MUL, 1, 16512, [3]) == GENERIC


def test_other_ab_options_are_generic():
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [2, 3, 4], opts=ops.GemvOpts(depth=2)) == GENERIC
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [2, 3, 4], opts=ops.GemvOpts(depth=4)) == GENERIC
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [2, 3, 4], opts=ops.GemvOpts(rpt=2)) == GENERIC


def test_segment_counts_outside_the_step_are_generic():
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [2, 3, 4, 4]) == GENERIC
    assert ops.gemv_route(ops.PRO_NONE, 1, H, [3, 3]) == GENERIC
    assert ops.gemv_route(_lib.PRO_MUL, 1, I, [3, 3]) == GENERIC


def test_act_mask_does_not_change_the_route():
    assert ops.gemv_route(ops.PRO_RMSNORM, 1, H, [4, 2], opts=ops.GemvOpts(act_mask=1)) == KEYED


def test_opts_keep_their_size():
    import ctypes
    assert ctypes.sizeof(ops.GemvOpts) == 6 * 4


def test_sort_is_stable_and_carries_act_mask():
    for n in (1, 2, 3, 4):
        for bits in itertools.product((2, 3, 4), repeat=n):
            for act_mask in range(1 << n):
                order, mask = ops.gemv_segment_order(list(bits), act_mask)
                assert sorted(order) == list(range(n))
                keys = [(bits[i], i) for i in order]
                assert keys == sorted(keys), (bits, order)             # ascending width; equal widths in the caller's order
                assert [(mask >> p) & 1 for p in range(n)] == [(act_mask >> i) & 1 for i in order], (bits, act_mask)
    assert ops.gemv_segment_order([4, 2, 3], 0b001) == ([1, 2, 0], 0b100)
    assert ops.gemv_segment_order([3, 3, 2], 0b010) == ([2, 0, 1], 0b100)
    assert ops.gemv_segment_order([4, 2], 0b01) == ([1, 0], 0b10)


def test_bad_arguments_are_refused():
    with pytest.raises(_lib.AmqError):
        ops.gemv_route(ops.PRO_RMSNORM, 1, H, [3] * 5)
    with pytest.raises(_lib.AmqError):
        ops.gemv_route(ops.PRO_RMSNORM, 1, H, [3], group=96)
