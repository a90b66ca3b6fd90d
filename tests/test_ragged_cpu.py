"""CPU-only: the host side of batched decode over prompts of unequal length -- the mask helper of the HF surface (left padding -> right-padded ids +
lengths), the ``padded`` flag of convert_model_to_hip, and the per-sequence step-state entry points in the header, the library and the bindings."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ_SYMBOLS = ("amq_attn_decode_seq_f16", "amq_decode_tail_seq_f16", "amq_decode_tail_sample_seq_f16", "amq_set_token_seq_f16")


def _left_pad(rows, S, pad):
    ids = torch.full((len(rows), S), pad, dtype=torch.int64)
    mask = torch.zeros(len(rows), S, dtype=torch.int64)
    for b, r in enumerate(rows):
        ids[b, S - len(r):] = torch.tensor(r)
        mask[b, S - len(r):] = 1
    return ids, mask


def test_left_padded_masks_give_right_padded_ids_and_lengths():
    from amq_amd.hf_fast import left_padded_to_right
    rows = [[11, 12, 13, 14, 15, 16, 17, 18, 19], [21, 22, 23, 24], [31, 32, 33, 34, 35, 36, 37], [41]]
    ids, mask = _left_pad(rows, 9, pad=999)
    right, lengths = left_padded_to_right(mask, ids)
    assert lengths.tolist() == [9, 4, 7, 1] and lengths.dtype is torch.int64
    assert right.shape == ids.shape and right.dtype is ids.dtype
    for b, r in enumerate(rows):
        assert right[b, :len(r)].tolist() == r
        assert right[b, len(r):].tolist() == [0] * (9 - len(r))            # the fill id: a valid token, never the caller's pad id
    assert left_padded_to_right(mask, ids, fill=7)[0][1, 4:].tolist() == [7] * 5
    # the caller's tensors are not touched
    ids2, mask2 = _left_pad(rows, 9, pad=999)
    assert torch.equal(ids, ids2) and torch.equal(mask, mask2)
    # other integer dtypes and bool carry the same 0 / 1 values
    for dt in (torch.int32, torch.uint8, torch.bool):
        r2, l2 = left_padded_to_right(mask.to(dt), ids.to(torch.int32))
        assert l2.tolist() == [9, 4, 7, 1] and torch.equal(r2.to(torch.int64), right)


def test_full_mask_gives_every_length_s():
    from amq_amd.hf_fast import left_padded_to_right
    ids = torch.arange(1, 13).view(2, 6)
    right, lengths = left_padded_to_right(torch.ones_like(ids), ids)
    assert torch.equal(right, ids) and lengths.tolist() == [6, 6]


def test_everything_else_is_refused():
    from amq_amd.hf_fast import left_padded_to_right
    ids = torch.arange(1, 13).view(2, 6)
    ok = torch.tensor([[0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]])
    assert left_padded_to_right(ok, ids) is not None
    hole = torch.tensor([[0, 1, 0, 1, 1, 1], [1, 1, 1, 1, 1, 1]])
    right_pad = torch.tensor([[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]])
    both = torch.tensor([[0, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1]])
    empty_row = torch.tensor([[0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1]])
    twos = torch.tensor([[0, 0, 2, 2, 2, 2], [1, 1, 1, 1, 1, 1]])
    negative = torch.tensor([[0, 0, -1, 1, 1, 1], [1, 1, 1, 1, 1, 1]])
    for bad in (hole, right_pad, both, empty_row, twos, negative):
        assert left_padded_to_right(bad, ids) is None, bad.tolist()
    assert left_padded_to_right(ok.to(torch.float32), ids) is None         # a floating mask (HF's additive form is one) is not this helper's
    assert left_padded_to_right(ok.to(torch.float16), ids) is None
    assert left_padded_to_right(ok[:, :5], ids) is None                    # shapes differ
    assert left_padded_to_right(ok[0], ids[0]) is None                     # not [B, S]
    assert left_padded_to_right(None, ids) is None
    assert left_padded_to_right(ok.tolist(), ids) is None


def test_compacting_then_expanding_reproduces_the_ids():
    from amq_amd.hf_fast import left_padded_to_right
    g = torch.Generator().manual_seed(3)
    for B, S in ((1, 1), (3, 9), (8, 33)):
        lens = torch.randint(1, S + 1, (B,), generator=g).tolist()
        rows = [torch.randint(1, 1000, (n,), generator=g).tolist() for n in lens]
        ids, mask = _left_pad(rows, S, pad=0)
        right, lengths = left_padded_to_right(mask, ids)
        assert lengths.tolist() == lens
        back = torch.zeros_like(ids)
        for b, n in enumerate(lens):
            back[b, S - n:] = right[b, :n]
        assert torch.equal(back, ids)


def test_padded_is_an_opt_in_flag_beside_sampling():
    import inspect
    from amq_amd import hf_fast
    from amq_amd.llama import DenseLlama, QuantLlama
    sig = inspect.signature(hf_fast.convert_model_to_hip)
    assert sig.parameters["padded"].default is False and sig.parameters["sampling"].default is False
    assert inspect.signature(QuantLlama.__init__).parameters["ragged"].default is False
    assert inspect.signature(QuantLlama.from_hf).parameters["ragged"].default is False
    for fn in (QuantLlama.prefill, QuantLlama.generate):
        assert inspect.signature(fn).parameters["lengths"].default is None
    with pytest.raises(ValueError, match="one position"):
        DenseLlama("7B", ragged=True)                                       # refused before anything is built


def test_per_sequence_entry_points_declared_exported_and_bound():
    from amq_amd import _lib
    src = open(os.path.join(ROOT, "include", "amq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    stride = int(re.search(r"#define\s+AMQ_STEP_STATE_STRIDE\s+(\d+)", code).group(1))
    assert stride % 16 == 0 and stride >= 264 and stride == _lib.STEP_STATE_STRIDE
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SEQ_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), f"{s} not declared in amq_hip.h"
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound"
    # the argument counts of the bindings are the header's
    for s in SEQ_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % s, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[s][1]), s


def test_per_sequence_entry_points_validate_before_any_launch():
    from amq_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(4096)
    f = lib.amq_attn_decode_seq_f16
    assert f(one, one, one, one, one, one, None, 3, 8, 2, 128, 2048, 0, None, 0, None, None) == -1           # no step states
    assert f(one, one, one, one, one, one, one, 3, 8, 2, 64, 2048, 0, None, 0, None, None) == -2             # head_dim
    assert f(one, one, one, one, one, one, one, 3, 8, 3, 128, 2048, 0, None, 0, None, None) == -2            # heads
    assert f(one, one, one, one, one, one, one, 3, 8, 2, 128, 2048, 4, None, 0, None, None) == -1            # split without workspace / tickets
    assert f(one, one, one, one, one, one, one, 3, 8, 2, 128, 2048, 4, one, 16, one, None) == -1 and b"workspace" in lib.amq_last_error()
    assert f(one, one, one, one, one, one, one, 3, 8, 2, 128, 1 << 20, 0, None, 0, None, None) == -2         # single workgroup: cache too long
    t = lib.amq_decode_tail_seq_f16
    assert t(one, 1024, one, 256, one, None, one, one, 64, 3, None, None) == -1
    assert t(one, 1024, one, 256, one, one, one, None, 64, 3, None, None) == -1                               # the table is not optional here
    assert t(one, 1001, one, 256, one, one, one, one, 64, 3, None, None) == -2                                # batched rows: vocab % 8
    s = lib.amq_decode_tail_sample_seq_f16
    assert s(one, 1024, one, 256, one, one, one, one, 64, 3, None, None, None) == -1 and b"state" in lib.amq_last_error()
    assert s(one, 1024, one, 256, one, one, one, one, 64, 9, None, one, None) == -2
    k = lib.amq_set_token_seq_f16
    assert k(one, 2, one, 1024, 256, one, one, one, one, 64, 3, None) == -2                                   # 2 ids for 3 sequences
    assert k(None, 1, one, 1024, 256, one, one, one, one, 64, 3, None) == -1
