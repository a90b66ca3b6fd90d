"""One-row decode: SiLU in gate_proj's epilogue (a segment with ``act``), down_proj's prologue only multiplies (``x_activated``: AMQ_PRO_MUL).

Before: down_proj staged fp16(silu_f(float(g))) * u from the stored fp16 gate g in EVERY workgroup.  After: the workgroup that produces g stores
s = fp16(silu_f(float(g))) -- the same device function on the same fp16 value -- and down_proj stages s * u: the same fp16 multiply.  Everything
here is therefore compared with torch.equal, never with a tolerance."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _layer(bits, n, k, seed, bias=False):
    from amq_amd import ops
    from amq_amd.hqq_format import random_hqq
    h = random_hqq(n, k, bits, seed=seed, bias=bias).to(DEV)
    qn, mn = ops.repack_from_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, n, k)
    return qn, mn, h.bias


def _rand(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.float16).to(DEV)


def _seg(layer, bits, n, y, **kw):
    from amq_amd import ops
    return dict(qn=layer[0], mn=layer[1], bits=bits, mode=ops.MODE_HQQ, N=n, y=y, **kw)


# ------------------------------------------------------------------------------------------------------------------ 1. the activated segment
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("gbits,ubits", [(4, 2), (3, 3), (2, 4)])
@pytest.mark.parametrize("k", [256, 4096])          # two tiles (most waves own none) / the hidden size of 7B
@pytest.mark.parametrize("m", [1, 3, 8])            # one row; the 2 .. 4-row and the 5 .. 8-row kernels
def test_activated_segment_is_silu_of_the_plain_one(m, k, gbits, ubits, bias):
    from amq_amd import ops
    n = 48                                          # three row-tiles: a workgroup of a rpt = 2 launch walks two (checked below with opts.rpt)
    gate_l, up_l = _layer(gbits, n, k, 10 + gbits, bias), _layer(ubits, n, k, 20 + ubits)
    x = _rand(m, k, seed=m + k)
    # (gamma around 8: gate values of a few units either side of 0, where SiLU bends)
    gamma = (8.0 + 0.8 * torch.randn(k, generator=torch.Generator().manual_seed(3))).to(torch.float16).to(DEV)
    for opts in (None, ops.GemvOpts(rpt=2)):
        outs = {}
        for act in (False, True):
            g, u = (torch.empty(m, n, dtype=torch.float16, device=DEV) for _ in range(2))
            ops.gemv_grouped(x, [_seg(gate_l, gbits, n, g, bias=gate_l[2] if bias else None, act=act), _seg(up_l, ubits, n, u)], k,
                             prologue=ops.PRO_RMSNORM, gamma=gamma, eps=1e-5, opts=opts)
            outs[act] = (g, u)
        (g_plain, u_plain), (g_act, u_act) = outs[False], outs[True]
        assert bool((g_plain < 0).any()) and bool((g_plain > 0).any()) and bool(torch.isfinite(g_plain.float()).all())
        assert torch.equal(g_act, ops.silu_mul(g_plain, torch.ones_like(g_plain)))
        assert torch.equal(u_act, u_plain)
        if opts is not None:
            assert (opts.rpt, opts.act_mask) == (2, 0)      # the caller's options are not written to


def test_activated_segment_takes_no_residual_and_no_sums():
    from amq_amd import ops
    from amq_amd._lib import AmqError
    k, n, m = 4096, 48, 2
    layer = _layer(3, n, k, 13)
    x, res = _rand(m, k, seed=1), _rand(m, n, seed=2)
    y = torch.empty(m, n, dtype=torch.float16, device=DEV)
    with pytest.raises(AmqError):
        ops.gemv_grouped(x, [_seg(layer, 3, n, y, residual=res, act=True)], k)
    ss = torch.zeros(m, n // 16, dtype=torch.float32, device=DEV)
    with pytest.raises((AmqError, ValueError)):
        ops.gemv_grouped_sums(x, [_seg(layer, 3, n, y, act=True)], k, sums_out=ss)
    with pytest.raises(ValueError):                 # the multiply-only prologue is a form of SiLU*mul
        ops.gemv_grouped(x, [_seg(layer, 3, n, y)], k, x_activated=True)
    torch.cuda.synchronize()


def test_groups_of_64_refuse_the_new_forms():
    """groups of 64 / 32 keep AMQ_PRO_SILU_MUL: the validator says so instead of running another kernel"""
    from amq_amd import ops
    from amq_amd._lib import AmqError
    from amq_amd.hqq_format import random_hqq
    k, n = 1024, 32
    h = random_hqq(n, k, 4, seed=5, group=64).to(DEV)
    qn, mn = ops.repack_from_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), 4, n, k, group=64)
    x, up = _rand(1, k, seed=1), _rand(1, k, seed=2)
    y = torch.empty(1, n, dtype=torch.float16, device=DEV)
    seg = dict(qn=qn, mn=mn, bits=4, mode=ops.MODE_HQQ, N=n, y=y)
    ops.gemv_grouped(x, [seg], k, prologue=ops.PRO_SILU_MUL, x2=up)
    with pytest.raises(AmqError):
        ops.gemv_grouped(x, [seg], k, prologue=ops.PRO_SILU_MUL, x2=up, x_activated=True)
    with pytest.raises(AmqError):
        ops.gemv_grouped(x, [dict(seg, act=True)], k)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 2. PRO_MUL == PRO_SILU_MUL
# K, waves per workgroup (None: the launch plan's own), rows
MUL_SHAPES = [(1408, None, (1, 2, 4)),              # 11 tiles, 176 chunks: neither a multiple of the wave count
              (4224, 8, (1, 2, 4)),                 # two chunks per thread on 8 waves
              (11008, 16, (1, 2, 4)),               # the 7B down_proj
              (11008, None, (8,)),                  # ... at 8 rows: two K phases (the launch plan's own choice only)
              (28672, 16, (1, 2, 4))]               # four chunks per thread (70B down_proj)


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("k,waves,rows", MUL_SHAPES, ids=[f"K{k}-w{w}-m{'_'.join(map(str, r))}" for k, w, r in MUL_SHAPES])
def test_mul_prologue_over_activated_gate_equals_silu_mul(k, waves, rows, bits):
    from amq_amd import ops
    from amq_amd._lib import AmqError
    n = 32
    layer = _layer(bits, n, k, 30 + bits)
    opts = None if waves is None else ops.GemvOpts(waves=waves)
    fits = ops.gemv_max_rows(k, plain=waves is None, norm=False)
    for m in rows:
        gate, up, res = _rand(m, k, seed=k + m, scale=2.0), _rand(m, k, seed=k + m + 1), _rand(m, n, seed=7)
        y_old, y_new = (torch.empty(m, n, dtype=torch.float16, device=DEV) for _ in range(2))
        if m > fits:                                # (4 rows of K = 28672 do not fit LDS: refused alike under either prologue)
            for kw in (dict(), dict(x_activated=True)):
                with pytest.raises(AmqError):
                    ops.gemv_grouped(gate, [_seg(layer, bits, n, y_old, residual=res)], k, prologue=ops.PRO_SILU_MUL, x2=up, opts=opts, **kw)
            continue
        ops.gemv_grouped(gate, [_seg(layer, bits, n, y_old, residual=res)], k, prologue=ops.PRO_SILU_MUL, x2=up, opts=opts)
        act = ops.silu_mul(gate, torch.ones_like(gate))
        ops.gemv_grouped(act, [_seg(layer, bits, n, y_new, residual=res)], k, prologue=ops.PRO_SILU_MUL, x2=up, opts=opts, x_activated=True)
        assert bool(torch.isfinite(y_old.float()).all()) and not torch.equal(y_old, res)
        assert torch.equal(y_new, y_old), (k, waves, m, bits)


# ------------------------------------------------------------------------------------------------------------------ 3. the token step
def _run_steps(cfg, gate_act, monkeypatch, use_graph):
    from amq_amd.llama import QuantLlama
    monkeypatch.setattr(QuantLlama, "GATE_ACT", gate_act)
    m = QuantLlama(cfg, max_seq=32, device=DEV, batch=1)
    ids = torch.randint(0, 1023, (4,), generator=torch.Generator().manual_seed(1))
    m.prefill(ids, use_graph=False)
    if use_graph:
        m.capture()
    trail = []
    for _ in range(8):
        m.decode_step(use_graph=use_graph)
        trail.append((m.logits.clone(), m.token.clone(), [b["kc"].clone() for b in m.blocks], [b["vc"].clone() for b in m.blocks]))
    torch.cuda.synchronize()
    m.check()
    return trail


def _same_trail(a, b):
    for step, ((la, ta, ka, va), (lb, tb, kb, vb)) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(la.float()).all())
        assert torch.equal(la, lb), f"logits differ at step {step}"
        assert torch.equal(ta, tb), f"token differs at step {step}"
        assert all(torch.equal(x, y) for x, y in zip(ka, kb)) and all(torch.equal(x, y) for x, y in zip(va, vb)), f"KV cache differs at step {step}"


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_step_is_the_same_bits_with_the_gate_activated(use_graph, monkeypatch):
    from amq_amd import arch
    cfg = arch._cfg(2, 4096, 11008, 32, 32, 1, vocab=1024)
    _same_trail(_run_steps(cfg, False, monkeypatch, use_graph), _run_steps(cfg, True, monkeypatch, use_graph))


def test_step_is_the_same_bits_grouped_query_8192_wide(monkeypatch):
    """hidden size 8192 with grouped-query attention: gate / up run the two-chunk 8-wave kernel (4096 < K <= 8192), down_proj K = 28672 four chunks"""
    from amq_amd import arch
    cfg = arch._cfg(1, 8192, 28672, 64, 8, 1, vocab=1024)
    _same_trail(_run_steps(cfg, False, monkeypatch, True), _run_steps(cfg, True, monkeypatch, True))


def test_step_launches_what_it_says(monkeypatch):
    """the switch reaches the library: gate_proj's segment is marked, down_proj's call says its x is activated (and neither without the switch)"""
    from amq_amd import arch, ops
    from amq_amd.llama import QuantLlama
    seen = []
    real = ops.gemv_grouped

    def spy(x, segments, K, **kw):
        seen.append((kw.get("prologue", ops.PRO_NONE), [bool(s.get("act")) for s in segments], bool(kw.get("x_activated"))))
        return real(x, segments, K, **kw)

    for on in (False, True):
        monkeypatch.setattr(QuantLlama, "GATE_ACT", on)
        m = QuantLlama(arch._cfg(1, 4096, 11008, 32, 32, 1, vocab=1024), max_seq=32, device=DEV, batch=1)
        m.prefill(torch.randint(0, 1023, (4,), generator=torch.Generator().manual_seed(1)), use_graph=False)
        seen.clear()
        monkeypatch.setattr(ops, "gemv_grouped", spy)
        m._step()
        monkeypatch.setattr(ops, "gemv_grouped", real)
        torch.cuda.synchronize()
        assert seen == [(ops.PRO_RMSNORM, [False] * 3, False), (ops.PRO_NONE, [False], False), (ops.PRO_RMSNORM, [on, False], False),
                        (ops.PRO_SILU_MUL, [False], on)]


def test_two_rows_with_down_proj_kept_fused_are_untouched_by_the_switch(monkeypatch):
    """DOWN_FUSED_ROWS raised (the A/B plan of DESIGN.md section 4: SiLU*mul stays in down_proj's prologue at 2 .. 4 rows, the norms ride on partial
    sums): the switch is for one row -- such a step runs, and is the same bits, with it off and on"""
    from amq_amd import arch
    from amq_amd.llama import QuantLlama, DOWN_FUSED, NORM_FROM_SUMS
    cfg = arch._cfg(2, 4096, 11008, 32, 32, 1, vocab=1024)
    monkeypatch.setattr(QuantLlama, "DOWN_FUSED_ROWS", 4)
    trails = {}
    for on in (False, True):
        monkeypatch.setattr(QuantLlama, "GATE_ACT", on)
        m = QuantLlama(cfg, max_seq=32, device=DEV, batch=2)
        assert (m.plan.down, m.plan.norm) == (DOWN_FUSED, NORM_FROM_SUMS)
        m.prefill(torch.randint(0, 1023, (2, 4), generator=torch.Generator().manual_seed(1)), use_graph=False)
        trail = []
        for use_graph in (False, True, True):
            m.decode_step(use_graph=use_graph)
            trail.append((m.logits.clone(), m.token.clone(), [b["kc"].clone() for b in m.blocks], [b["vc"].clone() for b in m.blocks]))
        torch.cuda.synchronize()
        m.check()
        trails[on] = trail
    _same_trail(trails[False], trails[True])
