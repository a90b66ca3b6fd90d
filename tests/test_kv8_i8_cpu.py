"""kv8_kernel="i8" without a GPU: what the runner's option check accepts and refuses, and the auto policy's chunks (whole 128-key stages)."""
import pytest

from amq_amd import llama, ops


def test_check_kv8_kernel_serves_multi_head_and_grouped_models():
    assert llama.check_kv8_kernel("i8", 8, 32, 32) == "i8" and llama.check_kv8_kernel("i8", 8, 32, 8) == "i8"
    assert "i8" in ops.KV8_KERNELS
    with pytest.raises(ValueError, match="needs kv_bits=8"):
        llama.check_kv8_kernel("i8", 16, 32, 32)
    with pytest.raises(ValueError, match="1 .. 16 query heads"):
        llama.check_kv8_kernel("i8", 8, 32, 1)
    with pytest.raises(ValueError, match="grouped-query"):          # what "mfma" is refused for stays refused for it
        llama.check_kv8_kernel("mfma", 8, 32, 32)


@pytest.mark.parametrize("nh,nkv", [(32, 32), (32, 8), (16, 1)])
@pytest.mark.parametrize("batch", [1, 8])
def test_splits_policy_gives_whole_stages(nh, nkv, batch):
    assert all(ops.attn_decode_kv8_i8_splits(ms, nh, batch, nkv) == 1 for ms in (1, 64, 128))         # a cache of one stage
    for max_seq in (129, 256, 1000, 1024, 4160, 32832, 100000):
        ns = ops.attn_decode_kv8_i8_splits(max_seq, nh, batch, nkv)
        chunk = ops.attn_decode_kv8_i8_chunk(max_seq, ns)
        assert 1 <= ns <= 1024 and chunk % ops.KV8_GQA_STAGE == 0
        assert ns * chunk >= max_seq > (ns - 1) * chunk, (max_seq, ns, chunk)       # the chunks cover the cache, none is empty
