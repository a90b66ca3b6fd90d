"""Which launches make up one eager token step of R rows (QuantLlama.plan walked by ``_step``): the recorded sequence of ops calls of a two-block
7B-width model, for every row count at which the plan changes and for the ragged, lookup, NORM_SUMS = False and sampled-tail runners.  Two blocks
are the smallest model in which block 1's first norm rides on the sums block 0's down_proj left.  The expected lists were recorded with this
recorder on the commit before ``step_plan`` existed (the flag-driven ``_step``); they are not produced by the code under test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RECORDED = ("gemv_grouped", "gemv_grouped_sums", "rmsnorm", "silu_mul", "attn_decode", "attn_decode_rows", "gemm", "gemv_f16w", "decode_tail",
            "decode_tail_sample", "decode_tail_lookup")
PROLOGUES = {0: "NONE", 1: "RMSNORM", 2: "SILU_MUL"}


def _other(name):
    return (name, None, 0, False, False)


def _grouped(pro, nseg):
    return ("gemv_grouped", pro, nseg, False, False)


def _sums(pro, nseg, sums_in, sums_out):
    return ("gemv_grouped_sums", pro, nseg, sums_in, sums_out)


# (name, prologue, number of segments, sums_in given, sums_out given)
_FUSED_BLOCK = [_grouped("RMSNORM", 3), _other("attn_decode"), _grouped("NONE", 1), _grouped("RMSNORM", 2), _grouped("SILU_MUL", 1)]
_SUMS_REST = [_sums("NONE", 1, False, True), _sums("RMSNORM", 2, True, False), _other("silu_mul"), _sums("NONE", 1, False, True)]


def _sums_step(first, attn="attn_decode", tail="decode_tail"):
    """a step whose norms ride on partial sums: block 0 opens with ``first``, block 1 with the sums block 0's down_proj left"""
    return first + [_other(attn)] + _SUMS_REST + [_sums("RMSNORM", 3, True, False), _other(attn)] + _SUMS_REST + [_other("gemv_f16w"), _other(tail)]


_LAUNCHED_BLOCK = [_other("rmsnorm"), _grouped("NONE", 3), _other("attn_decode"), _grouped("NONE", 1), _other("rmsnorm"), _grouped("NONE", 2),
                   _other("silu_mul"), _grouped("NONE", 1)]

EXPECTED = {
    "batch1": _FUSED_BLOCK * 2 + [_other("gemv_f16w"), _other("decode_tail")],
    "batch2": _sums_step([_grouped("RMSNORM", 3)]),
    "batch4": _sums_step([_grouped("RMSNORM", 3)]),
    "batch5": _sums_step([_other("rmsnorm"), _grouped("NONE", 3)]),
    "batch8": _sums_step([_other("rmsnorm"), _grouped("NONE", 3)]),
    "ragged2": _sums_step([_grouped("RMSNORM", 3)]),
    "lookup3": _sums_step([_grouped("RMSNORM", 3)], attn="attn_decode_rows", tail="decode_tail_lookup"),
    "batch5_no_sums": _LAUNCHED_BLOCK * 2 + [_other("gemv_f16w"), _other("decode_tail")],
    "batch1_sampled": _FUSED_BLOCK * 2 + [_other("gemv_f16w"), _other("decode_tail_sample")],
}

CASES = {       # name -> (constructor arguments, NORM_SUMS, sampled tail)
    "batch1": (dict(batch=1), True, False),
    "batch2": (dict(batch=2), True, False),
    "batch4": (dict(batch=4), True, False),
    "batch5": (dict(batch=5), True, False),
    "batch8": (dict(batch=8), True, False),
    "ragged2": (dict(batch=2, ragged=True), True, False),
    "lookup3": (dict(lookup=3), True, False),
    "batch5_no_sums": (dict(batch=5), False, False),
    "batch1_sampled": (dict(batch=1), True, True),
}


def build_runner(name, setattr_=setattr):
    """the runner of case ``name`` after its 4-token prompt (``setattr_``: how the class switch is set -- monkeypatch.setattr in the test)"""
    from amq_amd import arch
    from amq_amd.llama import QuantLlama
    kwargs, norm_sums, sampled = CASES[name]
    setattr_(QuantLlama, "NORM_SUMS", norm_sums)
    m = QuantLlama(arch._cfg(2, 4096, 11008, 32, 32, 1, vocab=1024), max_seq=32, device=DEV, **kwargs)
    if sampled:
        m.set_sampling(0.8, 20, 0.9, seed=5)
    ids = torch.randint(0, 1023, (m.B, 4) if m.B > 1 else (4,), generator=torch.Generator().manual_seed(1))
    m.prefill(ids, use_graph=False)
    return m, sampled


def record_step(m, sampled, setattr_):
    """one eager ``_step`` of ``m`` with pass-through recorders over the ops functions of RECORDED -> the list of launches"""
    from amq_amd import ops
    calls = []

    def recorder(name, fn):
        def wrapped(*args, **kwargs):
            if name == "gemv_grouped":
                pro = kwargs.get("prologue", args[3] if len(args) > 3 else ops.PRO_NONE)
                calls.append((name, PROLOGUES[pro], len(args[1]), False, False))
            elif name == "gemv_grouped_sums":
                calls.append((name, "RMSNORM" if kwargs.get("gamma") is not None else "NONE", len(args[1]), kwargs.get("sums_in") is not None,
                              kwargs.get("sums_out") is not None))
            else:
                calls.append(_other(name))
            return fn(*args, **kwargs)
        return wrapped

    for name in RECORDED:
        setattr_(ops, name, recorder(name, getattr(ops, name)))
    m._step(True) if sampled else m._step()
    torch.cuda.synchronize()
    m.check()
    return calls


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_of_one_step(name, monkeypatch):
    m, sampled = build_runner(name, monkeypatch.setattr)
    calls = record_step(m, sampled, monkeypatch.setattr)
    print(name, calls)
    assert calls == EXPECTED[name]
    assert bool(torch.isfinite(m.logits.float()).all())
