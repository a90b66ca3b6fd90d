"""Every token step of the runners (amq_amd/llama.py: decode_step behind a prompt pass) gives, byte for byte, what the commit recorded in
tests/golden/step_digests.json gave.  How a runner is put together -- which options it accepts, in which order its synthetic weights are drawn,
which buffers, caches, plan and routes it ends up with -- is host-side code that only chooses tensors and launches, so a digest that moves is a
weight that was drawn differently or a launch that changed.  Each case builds a runner, runs an eager prompt pass of 12 ids and 6 eager token
steps and digests its ``inputs`` (the embedding, drawn after every block, and block 0's q_proj), the six tokens, the final logits, the position
and every block's cache tensors (a lookup runner: its history and state block too).  The models are the smallest with two blocks: block 1's first
norm rides on the sums block 0's down_proj left.  tests/golden/gen_step_digests.py wrote the file; that a replay equals the eager step is
asserted elsewhere."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_digests.json")
MAX_SEQ, PROMPT, STEPS = 64, 12, 6
_IDS = []
CASES = {}


def ids_pool():
    """int64 [8, 12] below 1000 (a valid id in every model here), the same on any CPU; drawn once, never written"""
    if not _IDS:
        _IDS.append(torch.randint(0, 1000, (8, PROMPT), generator=torch.Generator().manual_seed(20261022)))
    return _IDS[0]


def _case(key, model="base", lengths=None, sampling=None, **kw):
    CASES[key] = dict(model=model, lengths=lengths, sampling=sampling, kw=kw)


for _b in (1, 2, 5, 8):
    _case(f"B{_b}", batch=_b)
_case("ragged_B3", lengths=(12, 1, 7), batch=3, ragged=True)
_case("lookup3", lookup=3)
_case("lookup3_sampled", sampling=dict(seed=1, top_k=8), lookup=3, lookup_sampling=True)
_case("B2_sampled", sampling=dict(seed=1, top_k=8), batch=2)
_case("kv8_B1", kv_bits=8)
_case("kv8_B2", kv_bits=8, batch=2)
_case("lm8", lm_head_bits=8)
_case("lm4", lm_head_bits=4)
_case("g64", group=64)
_case("mixed", "mixed")
_case("qwen3_B1", "qwen3")
_case("qwen3_B2", "qwen3", batch=2)
_case("owq", "owq")
_case("dense_B1", "dense")
_case("dense_B2", "dense", batch=2)


def _base_cfg():
    from amq_amd import arch
    return dict(arch._cfg(2, 512, 1024, 4, 2, 1, vocab=1024))


def build(model, kw):
    from amq_amd.llama import DenseLlama, QuantLlama
    if model == "owq":
        from test_gpu_owq_runner import owq_model       # (skips without transformers, as that module does)
        return QuantLlama.from_hf(owq_model(2)[1], max_seq=MAX_SEQ, **kw)
    if model == "dense":
        return DenseLlama(_base_cfg(), device=DEV, max_seq=MAX_SEQ, seed=4, **kw)
    if model == "qwen3":
        return QuantLlama("tiny-qwen3-test", None, device=DEV, max_seq=MAX_SEQ, seed=3, **kw)
    al = None
    if model == "mixed":
        rng = np.random.default_rng(0)
        al = {name: [int(b) for b in rng.choice([2, 3, 4], size=2)] for name in _base_cfg()["linear"]}
    return QuantLlama(_base_cfg(), al, device=DEV, max_seq=MAX_SEQ, seed=3, **kw)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def digest(key):
    """{name: sha256} of everything the case's prompt pass and token steps leave behind"""
    c = CASES[key]
    r = build(c["model"], dict(c["kw"]))
    lin = r.blocks[0]["self_attn.q_proj"]
    out = {"inputs": _sha(r.embed, *((lin,) if isinstance(lin, torch.Tensor) else (lin.qn, lin.mn)))}
    if c["sampling"]:
        r.set_sampling(**c["sampling"])
    r.prefill(ids_pool()[:r.B].to(DEV), use_graph=False, lengths=c["lengths"])
    tokens = [r.token.clone()]
    for _ in range(STEPS):
        r.decode_step(use_graph=False)
        tokens.append(r.token.clone())
    r.check()
    out.update(first_token=_sha(tokens[0]), tokens=_sha(*tokens[1:]), logits=_sha(r.logits), pos=_sha(r.pos))
    for name in ("kc", "vc", "kc8", "ks", "vc8", "vs"):
        out.update({f"{name}.{i}": _sha(blk[name]) for i, blk in enumerate(r.blocks) if name in blk})
    if r.lookup:
        out.update(history=_sha(r.history), lookup_state=_sha(r.lookup_state))
    return out


@pytest.mark.parametrize("key", list(CASES))
def test_bytes_of_the_recorded_commit(key):
    doc = json.load(open(GOLDEN))
    got, want = digest(key), doc["cases"][key]
    where = f"commit {doc['commit'][:7]}; recorded under HIP {doc['hip']} on {doc['device']}, this run under HIP {torch.version.hip}"
    assert got["inputs"] == want["inputs"], f"the INPUTS (embedding, block 0's q_proj) are not the recorded ones: nothing is said about the steps; {where}"
    assert got == want, f"{[k for k in want if got.get(k) != want[k]]} differ from {where}"
