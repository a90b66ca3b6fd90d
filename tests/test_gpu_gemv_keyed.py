"""One-row GEMV launches whose segments' bit-widths are fixed at compile time (gemv_kernel_keyed; include/amq_hip.h amq_gemv_route) against the
generic kernel forced onto the same launch (GemvOpts.depth = GEMV_DEPTH_GENERIC: same geometry, same segment order, same buffers).

The keyed kernels run the same bodies on the same tiles in the same order, so everything is compared with torch.equal; one case per bit-width is
also held against F.linear over the dequantized weights on the CPU, at the project's bar |dy| <= 1e-3 |y| + 1e-3 rms(y).  Shapes below K = 2048
(and K = 1408 on 16 waves) pass the waves explicitly: left alone such launches run 4 waves per workgroup, which the keyed kernels do not cover."""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = (2, 3, 4)


@functools.lru_cache(maxsize=None)
def _layer(bits, n, k, seed, bias=False):
    from amq_amd import ops
    from amq_amd.hqq_format import random_hqq
    h = random_hqq(n, k, bits, seed=seed, bias=bias).to(DEV)
    qn, mn = ops.repack_from_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), bits, n, k)
    return qn, mn, h.bias


@functools.lru_cache(maxsize=None)
def _rand(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.float16).to(DEV)


@functools.lru_cache(maxsize=None)
def _gamma(k):
    return (1.0 + 0.1 * torch.randn(k, generator=torch.Generator().manual_seed(3))).to(torch.float16).to(DEV)


def _opts(waves, generic):
    from amq_amd import _lib, ops
    return ops.GemvOpts(waves=waves or 0, depth=_lib.GEMV_DEPTH_GENERIC if generic else 0)


def _both_routes(x, k, layers, bits, ns, waves, prologue, bias=False, act=(), residual=None, **kw):
    """the launch under either route -> ({route: [y per segment]}); asserts the default route IS the keyed one"""
    from amq_amd import _lib, ops
    pro_lib = _lib.PRO_MUL if kw.get("x_activated") else prologue
    assert ops.gemv_route(pro_lib, 1, k, list(bits), opts=_opts(waves, False)) == _lib.GEMV_ROUTE_KEYED
    assert ops.gemv_route(pro_lib, 1, k, list(bits), opts=_opts(waves, True)) == _lib.GEMV_ROUTE_GENERIC
    outs = {}
    for generic in (False, True):
        ys = [torch.full((1, n), float("nan"), dtype=torch.float16, device=DEV) for n in ns]
        segs = [dict(qn=l[0], mn=l[1], bits=b, mode=ops.MODE_HQQ, N=n, y=y, bias=l[2] if bias else None, act=i in act, residual=residual)
                for i, (l, b, n, y) in enumerate(zip(layers, bits, ns, ys))]
        ops.gemv_grouped(x, segs, k, prologue=prologue, opts=_opts(waves, generic), **kw)
        outs[generic] = ys
    return outs


def _assert_same(outs, what):
    for i, (a, b) in enumerate(zip(outs[False], outs[True])):
        assert bool(torch.isfinite(b.float()).all()), (what, i)          # every element written (the outputs start as NaN)
        assert torch.equal(a, b), (what, "segment", i)
    for (i, a), (j, b) in itertools.combinations(enumerate(outs[False]), 2):
        n = min(a.shape[1], b.shape[1])
        assert not torch.equal(a[:, :n], b[:, :n]), (what, "segments", i, j, "hold the same values")


# ------------------------------------------------------------------------------------------------------------------ q/k/v
QKV_ROWS = (48, 16, 32)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("k,waves,orders", [(256, 8, "all"), (1024, 8, "all"), (4096, None, "three")],
                         ids=["K256-two-tiles", "K1024-tile-per-wave", "K4096"])
def test_qkv_every_order_of_widths(k, waves, orders, bias):
    from amq_amd import ops
    x, gamma = _rand(1, k, seed=k), _gamma(k)
    todo = list(itertools.product(WIDTHS, repeat=3)) if orders == "all" else [(4, 3, 2), (3, 2, 3), (2, 2, 2)]
    assert len(todo) == (27 if orders == "all" else 3)
    for bits in todo:
        layers = [_layer(b, n, k, 100 + 10 * i + b, bias) for i, (b, n) in enumerate(zip(bits, QKV_ROWS))]
        outs = _both_routes(x, k, layers, bits, QKV_ROWS, waves, ops.PRO_RMSNORM, bias=bias, gamma=gamma, eps=1e-5)
        _assert_same(outs, (k, bits, bias))


# ------------------------------------------------------------------------------------------------------------------ gate/up
@pytest.mark.parametrize("act", [False, True], ids=["plain", "gate-activated"])
def test_gate_up_every_order_of_widths(act):
    from amq_amd import ops
    k, n = 1024, 48
    x, gamma = _rand(1, k, seed=k + 1), _gamma(k)
    for bits in itertools.product(WIDTHS, repeat=2):
        layers = [_layer(b, n, k, 200 + 10 * i + b) for i, b in enumerate(bits)]
        outs = _both_routes(x, k, layers, bits, (n, n), 8, ops.PRO_RMSNORM, act=(0,) if act else (), gamma=gamma, eps=1e-5)
        _assert_same(outs, (bits, act))
        if act:                                     # the activated output belongs to the gate wherever the sort put it
            plain = _both_routes(x, k, layers, bits, (n, n), 8, ops.PRO_RMSNORM, gamma=gamma, eps=1e-5)[False]
            assert torch.equal(outs[False][0], ops.silu_mul(plain[0], torch.ones_like(plain[0]))) and torch.equal(outs[False][1], plain[1])


def test_gate_up_workgroups_walk_two_row_tiles():
    """770 row-tiles on 768 workgroup slots: the launch runs 2 x 193 workgroups, all but one per segment walk two row-tiles"""
    from amq_amd import ops
    k, n, bits = 256, 6160, (4, 2)
    x, gamma = _rand(1, k, seed=9), _gamma(k)
    layers = [_layer(b, n, k, 300 + b) for b in bits]
    outs = _both_routes(x, k, layers, bits, (n, n), 8, ops.PRO_RMSNORM, act=(0,), gamma=gamma, eps=1e-5)
    _assert_same(outs, "770 row-tiles")


# ------------------------------------------------------------------------------------------------------------------ single segment
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("k,waves", [(256, 8), (4096, None)], ids=["K256", "K4096"])
def test_o_proj_with_residual(k, waves, bits):
    from amq_amd import ops
    n = 32
    x, res = _rand(1, k, seed=k + 2), _rand(1, n, seed=5)
    outs = _both_routes(x, k, [_layer(bits, n, k, 400 + bits)], (bits,), (n,), waves, ops.PRO_NONE, residual=res)
    _assert_same(outs, (k, bits))
    assert not torch.equal(outs[False][0], res)


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("activated", [True, False], ids=["PRO_MUL", "PRO_SILU_MUL"])
@pytest.mark.parametrize("k,waves", [(1408, 16), (11008, None)], ids=["K1408-11-tiles", "K11008"])
def test_down_proj(k, waves, activated, bits):
    from amq_amd import ops
    n = 32
    gate, up, res = _rand(1, k, seed=k + 3, scale=2.0), _rand(1, k, seed=k + 4), _rand(1, n, seed=6)
    outs = _both_routes(gate, k, [_layer(bits, n, k, 500 + bits)], (bits,), (n,), waves, ops.PRO_SILU_MUL, residual=res, x2=up, x_activated=activated)
    _assert_same(outs, (k, bits, activated))
    assert not torch.equal(outs[False][0], res)


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("bits", WIDTHS)
def test_against_dequantized_weights_on_the_cpu(bits):
    import torch.nn.functional as F
    from amq_amd import ops
    k, n = 4096, 32
    layer = _layer(bits, n, k, 600 + bits)
    x = _rand(1, k, seed=11)
    y = _both_routes(x, k, [layer], (bits,), (n,), None, ops.PRO_NONE)[False][0]
    w = ops.dequantize(layer[0], layer[1], bits, ops.MODE_HQQ, n, k)
    ref = F.linear(x.cpu().double(), w.cpu().double())
    err = (y.cpu().double() - ref).abs()
    bar = 1e-3 * ref.abs() + 1e-3 * ref.pow(2).mean().sqrt()
    print(f"bits {bits}: worst |dy| / bar = {float((err / bar).max()):.3f}")
    assert bool((err <= bar).all())


# ------------------------------------------------------------------------------------------------------------------ the token step
def _run_steps(generic, monkeypatch, use_graph):
    """two blocks of hidden 256 / intermediate 512 with a different width on every linear; the one-row launches are given the waves of the 7B step
    (8; 16 for down_proj) so that they are the keyed geometry, and either route"""
    from amq_amd import _lib, arch, ops
    from amq_amd.llama import QuantLlama
    cfg = arch._cfg(2, 256, 512, 2, 2, 1, vocab=1024)
    widths = {"self_attn.q_proj": [4, 2], "self_attn.k_proj": [2, 3], "self_attn.v_proj": [3, 3], "self_attn.o_proj": [3, 4],
              "mlp.gate_proj": [4, 2], "mlp.up_proj": [2, 2], "mlp.down_proj": [2, 3]}
    real, routes = ops.gemv_grouped, []

    def routed(x, segments, K, **kw):
        if x.numel() == K and kw.get("opts") is None:
            pro = kw.get("prologue", ops.PRO_NONE)
            kw["opts"] = _opts(16 if pro == ops.PRO_SILU_MUL else 8, generic)
            routes.append(ops.gemv_route(_lib.PRO_MUL if kw.get("x_activated") else pro, 1, K, [s["bits"] for s in segments], opts=kw["opts"]))
        return real(x, segments, K, **kw)

    monkeypatch.setattr(ops, "gemv_grouped", routed)
    m = QuantLlama(cfg, arch_linear=widths, max_seq=32, device=DEV, batch=1)
    m.prefill(torch.randint(0, 1023, (4,), generator=torch.Generator().manual_seed(1)), use_graph=False)
    if use_graph:
        m.capture()
    routes.clear()
    trail = []
    for _ in range(8):
        m.decode_step(use_graph=use_graph)
        trail.append((m.logits.clone(), m.token.clone(), [b["kc"].clone() for b in m.blocks], [b["vc"].clone() for b in m.blocks]))
    torch.cuda.synchronize()
    m.check()
    monkeypatch.setattr(ops, "gemv_grouped", real)
    if not use_graph:                               # (a replayed step makes no Python calls)
        want = _lib.GEMV_ROUTE_GENERIC if generic else _lib.GEMV_ROUTE_KEYED
        assert routes == [want] * (8 * 2 * 4), routes
    return trail


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_token_step_is_the_same_bits_under_either_route(use_graph, monkeypatch):
    a, b = _run_steps(False, monkeypatch, use_graph), _run_steps(True, monkeypatch, use_graph)
    for step, ((la, ta, ka, va), (lb, tb, kb, vb)) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(la.float()).all())
        assert torch.equal(la, lb), f"logits differ at step {step}"
        assert torch.equal(ta, tb), f"token differs at step {step}"
        assert all(torch.equal(x, y) for x, y in zip(ka, kb)) and all(torch.equal(x, y) for x, y in zip(va, vb)), f"KV cache differs at step {step}"
