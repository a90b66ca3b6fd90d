"""Every prompt pass of the runners (amq_amd/llama.py: prefill, prefill_batch, score_rows) gives, byte for byte, what the commit recorded in
tests/golden/prompt_digests.json gave: the walk over the blocks is host-side code that only chooses launches, so a digest that moves is a launch
that changed.  The cases are the smallest that take every route of the walk (few / tiled / frag, both edges of each), every form of the rotation
and cache write (no cache, fp16 cache at position 0 and behind cached rows, 8-bit cache) and every end of a pass (last row, all rows, ragged
lengths, lookup history, packed lm_head) on a two-block grouped-query model: the fused down_proj + norm of block 0 and the plain down_proj of the
last block both run.  Every case also digests its ``inputs`` (the embedding and one linear's weights: the synthetic weights come from a device
generator), so that other weights do not read as another walk.  tests/golden/gen_prompt_digests.py wrote the file; all passes run eager (that a
replay equals the eager pass is asserted elsewhere)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prompt_digests.json")
MAX_SEQ = 576           # the chunked case ends at row 464; everything else fits 512
_IDS = []
CASES = {}


def ids_pool():
    """int64 [9, 576] below 1000 (a valid id in every model here), the same on any CPU; drawn once, never written"""
    if not _IDS:
        _IDS.append(torch.randint(0, 1000, (9, MAX_SEQ), generator=torch.Generator().manual_seed(20261021)))
    return _IDS[0]


def _prefill(key, model, chunks, lengths=None, all_logits=False, **kw):
    """a case of prefill(): ``chunks`` an int S (one pass at position 0) or [(start_pos, S), ...] run in turn"""
    CASES[key] = dict(op="prefill", model=model, chunks=[(0, chunks)] if isinstance(chunks, int) else chunks, lengths=lengths,
                      all_logits=all_logits, kw=kw)


for _S in (5, 8, 9, 16, 17, 40, 384, 385):                                 # few | tiled | frag | tiled, both edges of each
    _prefill(f"b1_S{_S}", "base", _S)
_prefill("nofuse_S40", "nofuse", 40)
_prefill("chunk_frag", "base", [(0, 40), (40, 24)])
_prefill("chunk_few", "base", [(0, 40), (40, 24), (64, 3)])
_prefill("chunk_tiled", "base", [(0, 40), (40, 24), (64, 400)])
_prefill("g64_S40", "base", 40, group=64)
_prefill("g64_S5", "base", 5, group=64)
_prefill("mixed_S40", "mixed", 40)
for _S in (5, 40, 400):
    _prefill(f"kv8_S{_S}", "base", _S, kv_bits=8)
_prefill("kv8_B2_S40", "base", 40, kv_bits=8, batch=2)
_prefill("qwen3_S5", "qwen3", 5)
_prefill("qwen3_S40", "qwen3", 40)
_prefill("qwen3_B2_S24", "qwen3", 24, batch=2)
_prefill("qwen3_ragged_B2_S24", "qwen3", 24, lengths=(24, 7), batch=2, ragged=True)
_prefill("B3_S40", "base", 40, batch=3)
_prefill("ragged_B3_S40", "base", 40, lengths=(40, 1, 17), batch=3, ragged=True)
_prefill("ragged_B1_S40", "base", 40, batch=1, ragged=True)               # the tiled walk, not frag
_prefill("B2_S3", "base", 3, batch=2)                                       # B * S <= 8 stays on the tiled kernels
_prefill("lookup3_S40", "base", 40, lookup=3)
_prefill("all_S40", "base", 40, all_logits=True)
_prefill("all_B2_S40", "base", 40, all_logits=True, batch=2)
_prefill("all_lm8_S64", "base", 64, all_logits=True, lm_head_bits=8)      # the sliced route
_prefill("all_lm8_S40", "base", 40, all_logits=True, lm_head_bits=8)      # streamed
_prefill("all_lm4_S40", "base", 40, all_logits=True, lm_head_bits=4)
for _b in (8, 4):
    _prefill(f"lm{_b}_S40", "base", 40, lm_head_bits=_b)
    _prefill(f"lm{_b}_B3_S12", "base", 12, lm_head_bits=_b, batch=3)
_prefill("owq_S5", "owq", 5)
_prefill("owq_S40", "owq", 40)
_prefill("owq_B2_S12", "owq", 12, batch=2)
_prefill("dense_S5", "dense", 5)
_prefill("dense_S40", "dense", 40)
_prefill("dense_chunk", "dense", [(0, 40), (40, 24)])
_prefill("dense_B2_S12", "dense", 12, batch=2)
_prefill("dense_qkn_S12", "dense_qkn", 12)
CASES["batch_3x40"] = dict(op="prefill_batch", model="base", shape=(3, 40), kw={})
CASES["batch_dense_3x40"] = dict(op="prefill_batch", model="dense", shape=(3, 40), kw={})
CASES["batch_9x12"] = dict(op="prefill_batch", model="base", shape=(9, 12), kw={})      # one 8-row lm_head launch + the one-row vector form
CASES["score_2x40"] = dict(op="score_rows", model="base", shape=(2, 40), kw={})


def _base_cfg(**extra):
    from amq_amd import arch
    return dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=1024, **extra))


def build(model, kw):
    from amq_amd.llama import DenseLlama, QuantLlama
    if model == "owq":
        from test_gpu_owq_runner import owq_model       # (skips without transformers, as that module does)
        return QuantLlama.from_hf(owq_model(2)[1], max_seq=64, **kw)
    if model in ("dense", "dense_qkn"):
        return DenseLlama(_base_cfg(qk_norm=True) if model == "dense_qkn" else _base_cfg(), device=DEV, max_seq=MAX_SEQ, seed=4, **kw)
    if model == "qwen3":
        return QuantLlama("tiny-qwen3-test", None, device=DEV, max_seq=MAX_SEQ, seed=3, **kw)
    cls, al = QuantLlama, None
    if model == "nofuse":
        cls = type("NoFuse", (QuantLlama,), {"FUSE_DOWN_NORM": False})
    if model == "mixed":
        rng = np.random.default_rng(0)
        al = {name: [int(b) for b in rng.choice([2, 3, 4], size=2)] for name in _base_cfg()["linear"]}
    return cls(_base_cfg(), al, device=DEV, max_seq=MAX_SEQ, seed=3, **kw)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def digest(key):
    """{name: sha256} of everything the case's pass leaves behind"""
    c = CASES[key]
    r = build(c["model"], dict(c["kw"]))
    lin = r.blocks[0]["self_attn.q_proj"]
    out = {"inputs": _sha(r.embed, *((lin,) if isinstance(lin, torch.Tensor) else (lin.qn, lin.mn)))}
    if c["op"] != "prefill":
        B, S = c["shape"]
        ids = ids_pool()[:B, :S].to(DEV)
        out["result"] = _sha(r.prefill_batch(ids) if c["op"] == "prefill_batch" else r.score_rows(ids))
        return out
    r.all_logits = c["all_logits"]
    for start, S in c["chunks"]:
        r.prefill(ids_pool()[:r.B, start:start + S].to(DEV), use_graph=False, start_pos=start, lengths=c["lengths"])
    out.update(logits=_sha(r.logits), token=_sha(r.token), pos=_sha(r.pos))
    for name in ("kc", "vc", "kc8", "ks", "vc8", "vs"):
        out.update({f"{name}.{i}": _sha(blk[name]) for i, blk in enumerate(r.blocks) if name in blk})
    if c["all_logits"]:
        out["logits_rows"] = _sha(r.logits_rows)
    if r.lookup:
        out.update(history=_sha(r.history[:S]), lookup_state=_sha(r.lookup_state))
    return out


@pytest.mark.parametrize("key", list(CASES))
def test_bytes_of_the_recorded_commit(key):
    doc = json.load(open(GOLDEN))
    got, want = digest(key), doc["cases"][key]
    where = f"commit {doc['commit'][:7]}; recorded under HIP {doc['hip']} on {doc['device']}, this run under HIP {torch.version.hip}"
    assert got["inputs"] == want["inputs"], f"the INPUTS (embedding, block 0's q_proj) are not the recorded ones: nothing is said about the walk; {where}"
    assert got == want, f"{[k for k in want if got.get(k) != want[k]]} differ from {where}"
