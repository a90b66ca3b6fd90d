"""What the three device quantizers share (csrc/amq_quant.cuh, amq_quant_pack.hip): the Format A word, written by the HQQ emit kernel
and by the pack kernel of the GPTQ solve and AWQ's quantize, compared over the WHOLE packed tensor -- the padding of the last 3-bit words included --
and the pass that ORs the waves' nonfinite flags into the info block, with more flags than one stride of its 256 threads."""
import pytest
import torch

import awq_search_ref
import gptq_solver_ref
from quantize_common import assert_codes, assert_format_a, unpack_rows
from test_gpu_hqq_quantize import multi_w

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# R = 16: 3-bit chunk 9 missing, chunk 8 partly; R = 64: R % 10 != 0, several word rows per chunk; R = 80: R % 10 == 0
PACK_SHAPES = [(16, 128, 128), (16, 128, 32), (80, 128, 128)]


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("N,K,group", PACK_SHAPES + [(16, 256, 256)])       # groups of 256: HQQ alone has them
def test_hqq_emit_packs_its_own_codes_over_the_whole_tensor(N, K, group, bits):
    from amq_amd import ops
    h, info = ops.hqq_quantize(multi_w(N, K).to(DEV), bits, group, return_info=True)
    assert info.nonfinite == 0
    assert_format_a(h, bits, group, (N, K))
    assert_codes(h, unpack_rows(h.W_q.cpu(), bits, N * K // group))


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("N,K,group", PACK_SHAPES)
def test_gptq_pack_over_the_whole_tensor(N, K, group, bits):
    from amq_amd import ops
    W = multi_w(N, K)
    g = torch.Generator().manual_seed(K + group)
    U = torch.triu(0.05 * torch.randn(K, K, generator=g)) + torch.diag(0.5 + torch.rand(K, generator=g))       # upper, positive diagonal
    want = gptq_solver_ref.solve(W, U, bits, group, deploy=True)
    h = ops.gptq_quantize(W.to(DEV), U.to(DEV), bits, group)
    assert_format_a(h, bits, group, (N, K))
    assert_codes(h, want["q"])


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("N,K,group", PACK_SHAPES)
def test_awq_pack_over_the_whole_tensor(N, K, group, bits):
    from amq_amd import ops
    W = multi_w(N, K)
    want = awq_search_ref.quantize(W, bits, group, deploy=True)
    h = ops.awq_quantize(W.to(DEV), bits, group)
    assert_format_a(h, bits, group, (N, K))
    assert_codes(h, want["q"])


# ---------------------------------------------------------------------------------------------------------------- the flag pass
# N = 1040, K = 128: 260 wave flags of the GPTQ solve, 260 of AWQ's quantize, 520 of AWQ's clip at groups of 32 -- more than one stride of the 256
# threads that OR them -- and 325 passes = two workgroups' flags for HQQ's stop kernel at groups of 128
FLAG_N, FLAG_K, FLAG_T = 1040, 128, 16
STALE = 0x5a5a5a5a


def _flag_inputs():
    W = multi_w(FLAG_N, FLAG_K).to(DEV)
    X = torch.randn(FLAG_T, FLAG_K, generator=torch.Generator().manual_seed(3)).half().to(DEV)
    return W, X, torch.eye(FLAG_K, dtype=torch.float32, device=DEV)


def test_flag_pass_leaves_zero_over_a_stale_info_block():
    from amq_amd import ops
    W, X, U = _flag_inputs()
    N, K = W.shape
    W_q, scale, zero, info, work = ops.hqq_quantize_buffers(N, K, 3, 128, W.device)
    info.fill_(STALE)
    ops.hqq_quantize_launch(W, 3, 128, False, W_q, scale, zero, info, work)
    assert ops.HQQQuantizeInfo(info.cpu()).nonfinite == 0
    W_q, scale, zero, row_loss, info, work = ops.gptq_quantize_buffers(N, K, 3, 128, W.device)
    info.fill_(STALE)
    ops.gptq_quantize_launch(W, U, 3, 128, W_q, scale, zero, row_loss, info, work)
    assert int(info.cpu()[0]) == 0
    W_q, scale, zero, _, info, work = ops.awq_quantize_buffers(N, K, 3, 128, W.device)
    info.fill_(STALE)
    ops.awq_quantize_launch(W, 3, 128, None, None, None, W_q, scale, zero, None, info, work)
    assert int(info.cpu()[0]) == 0
    hi, lo, best, err, info, work = ops.awq_clip_buffers(N, K, FLAG_T, 3, 32, W.device)
    info.fill_(STALE)
    ops.awq_clip_launch(W, X, 3, 32, hi, lo, best, err, info, work)
    assert int(info.cpu()[0]) == 0


def test_flag_pass_sees_the_last_flag():
    from amq_amd import ops
    W, X, U = _flag_inputs()
    W[FLAG_N - 1, FLAG_K - 1] = float("nan")             # the last element: the last wave's flag, the last slot of every flag array
    with pytest.raises(ValueError, match="inf or NaN"):
        ops.hqq_quantize(W, 3, 128)
    with pytest.raises(ValueError, match="not finite"):
        ops.gptq_quantize(W, U, 3, 128)
    with pytest.raises(ValueError, match="not finite"):
        ops.awq_quantize(W, 3, 128)
    with pytest.raises(ValueError, match="not finite"):
        ops.awq_clip(W, X, 3, 32)
