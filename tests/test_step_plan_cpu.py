"""CPU-only: ``llama.step_plan`` -- which launches a token step of R rows is made of -- against the table of DESIGN.md section 4, at 7B widths with
the row limits the library itself reports (amq_query: no GPU needed)."""
import pytest

from amq_amd.llama import (DOWN_FUSED, DOWN_GEMM, DOWN_GEMV, DOWN_GEMV_SUMS, NORM_FROM_SUMS, NORM_FUSED, NORM_LAUNCH, QuantLlama, StepPlan,
                           step_plan)

H, I = 4096, 11008


def _limits(inter=I, fine=False):
    """(rows_h, rows_i, rows_i_phased) as QuantLlama.__init__ reads them"""
    try:
        from amq_amd import ops
        return (ops.gemv_max_rows(H, plain=True), ops.gemv_max_rows(inter, plain=not fine), ops.gemv_max_rows(inter, plain=not fine, norm=False))
    except (OSError, AttributeError) as e:
        pytest.skip(f"libamq_hip.so does not load here: {e}")


def _plan(R, inter=I, fine=False, **switches):
    return step_plan(R, H, inter, fine, *_limits(inter, fine), **switches)


@pytest.mark.parametrize("R", range(1, 9))
def test_table_at_7b_widths(R):
    first = NORM_FUSED if R <= 4 else NORM_LAUNCH
    expect = StepPlan(NORM_FUSED, NORM_FUSED, DOWN_FUSED) if R == 1 else StepPlan(first, NORM_FROM_SUMS, DOWN_GEMV_SUMS)
    assert _plan(R) == expect
    assert _plan(R).block_norm == expect.norm                   # block 1 .. ride on down_proj's sums
    # the defaults are the class switches
    assert _plan(R, norm_sums=QuantLlama.NORM_SUMS, norm_fused_rows=QuantLlama.NORM_FUSED_ROWS, down_fused_rows=QuantLlama.DOWN_FUSED_ROWS) == expect


@pytest.mark.parametrize("R", range(2, 9))
def test_without_sums(R):
    own = NORM_FUSED if R <= 4 else NORM_LAUNCH
    assert _plan(R, norm_sums=False) == StepPlan(own, own, DOWN_GEMV)


@pytest.mark.parametrize("R", range(1, 9))
def test_fine_groups_never_ride_on_sums(R):
    p = _plan(R, fine=True)
    assert NORM_FROM_SUMS not in (p.first_norm, p.norm, p.block_norm) and p.down != DOWN_GEMV_SUMS
    assert p.first_norm == p.norm == (NORM_FUSED if R <= 4 else NORM_LAUNCH)


def test_rows_past_the_phased_stage_take_the_gemm():
    """an intermediate size whose rows do not fit the GEMV's LDS stage even in two K phases, found from the library's own limits: down_proj is the
    few-row GEMM, which leaves no sums -- o_proj still does, so the second norm rides on them and the next block's first norm falls back"""
    inter, phased = next((i, _limits(i)[2]) for i in range(I, 1 << 17, 1024) if 1 <= _limits(i)[2] < 8)
    R = phased + 1
    p = _plan(R, inter)
    own = NORM_FUSED if R <= 4 else NORM_LAUNCH
    assert p == StepPlan(own, NORM_FROM_SUMS, DOWN_GEMM) and p.block_norm == own
    assert _plan(phased, inter).down == DOWN_GEMV_SUMS
    assert _plan(R, inter, norm_sums=False) == StepPlan(own, own, DOWN_GEMM)


def test_fused_down_proj_leaves_no_sums():
    """DOWN_FUSED_ROWS raised (an A/B setting): the prologue GEMV leaves no sums, the next block's first norm falls back"""
    p = _plan(2, down_fused_rows=4)
    assert p == StepPlan(NORM_FUSED, NORM_FROM_SUMS, DOWN_FUSED) and p.block_norm == NORM_FUSED
