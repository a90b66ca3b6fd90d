"""Mixed-precision Llama decode runner: the caller side of the hot path.

Counterpart of what ``amq_speed_benchmark.py:231-256`` assembles (a Llama whose
7 linears per block are 2/3/4-bit modules chosen by the arch JSON) and of the
patched forward in ``kernel/monkeypatch/ftllama_modeling.py:70-341`` (static
batch-1 KV cache, ``start_pos``), built MI355X-first:

  * one token step = 5 launches per block (fused-RMSNorm q/k/v GEMV with three
    bit-widths in one launch, RoPE+KV-append+attention, o_proj GEMV with
    residual epilogue, fused-RMSNorm gate/up GEMV, SiLU*mul-prologue down GEMV
    with residual epilogue) + fused final-norm lm_head GEMV + argmax;
  * the whole step is captured once into a hipGraph and replayed per token
    (position and token id live in device memory), so the ~165 launches cost
    device-side boundaries only, no Python/ctypes time;
  * prefill runs the same weights through the tiled MFMA GEMM.

Weights: real HQQ layers via ``from_hqq_weights`` (tests, real checkpoints) or
synthetic native payloads of the real shapes (``synthetic=True``; there is no
network for checkpoints -- values do not affect speed).
"""
import math
from typing import NamedTuple

import torch

from . import ops
from .arch import MODEL_CONFIGS, arch_bits, rope_inv_freq, uniform_arch
from .hqq_format import HQQWeights

EPS = 1e-5
ROPE_THETA = 10000.0


class _Lin:
    """native weights of one linear (+ its fp16 bias: Qwen2's q / k / v projections carry one).  An OWQ layer (HIPOWQLinear) also carries
    ``perm`` int32 [Kp], ``out_ids`` int32 [n_out] and ``W_out`` fp16 [N, n_out]: K is then the width of its input, ``Kp`` that of the packed
    layer (qn / mn are [N, Kp]); every other layer has Kp == K and the three fields None."""
    __slots__ = ("qn", "mn", "bits", "mode", "N", "K", "bias", "perm", "out_ids", "W_out", "Kp")

    def __init__(self, qn, mn, bits, mode, N, K, bias=None, perm=None, out_ids=None, W_out=None, Kp=None):
        self.qn, self.mn, self.bits, self.mode, self.N, self.K, self.bias = qn, mn, bits, mode, N, K, bias
        self.perm, self.out_ids, self.W_out, self.Kp = perm, out_ids, W_out, K if Kp is None else Kp

    @property
    def owq(self):
        return self.W_out is not None

    def seg(self, y, residual=None, act=False):
        return dict(qn=self.qn, mn=self.mn, bits=self.bits, mode=self.mode, N=self.N, y=y, residual=residual, bias=self.bias, act=act)

    def nbytes(self):
        own = 0 if self.W_out is None else self.W_out.numel() * 2 + self.perm.numel() * 4 + self.out_ids.numel() * 4
        return self.qn.numel() * 4 + self.mn.numel() * 2 + (0 if self.bias is None else self.bias.numel() * 2) + own


def _synthetic_linear(n, k, bits, gen, device, group=128):
    """Random native payload + (scale, zero) giving roughly unit-gain layers:
    any bit pattern is a valid weight matrix in the native layout (group: 128, or 64 / 32 = two / four pairs per tile row)."""
    qb, mb = ops.native_sizes(bits, n, k, group)
    qn = torch.randint(-2 ** 31, 2 ** 31 - 1, (qb // 4,), dtype=torch.int32, device=device, generator=gen)
    std_q = math.sqrt((4.0 ** bits - 1.0) / 12.0)
    s0 = 0.5 / (math.sqrt(k) * std_q)
    r = torch.rand(mb // 4, 2, device=device, generator=gen)
    meta = torch.empty(mb // 4, 2, dtype=torch.float16, device=device)
    meta[:, 0] = (s0 * (0.75 + 0.5 * r[:, 0])).to(torch.float16)
    meta[:, 1] = ((2 ** bits - 1) / 2.0 + (r[:, 1] - 0.5)).to(torch.float16)
    return _Lin(qn, meta.reshape(-1).contiguous(), bits, ops.MODE_HQQ, n, k)


def lm8_logits_sliced(xn, w8, out, scratch):
    """out [n, vocab] = xn [n, H] . W^T over the 8-bit lm_head ``w8`` (xn already normed), a slice of ``scratch.shape[0]`` vocabulary rows at a
    time (a multiple of 16, as the vocabulary): ops.lm8_dequantize into the scratch, the fp16 GEMM into the slice's columns of ``out``"""
    vocab, step = w8.shape[0], scratch.shape[0]
    if vocab % 16 or step % 16:
        raise ValueError(f"the fp16 GEMM writes 16-column blocks: a vocabulary of {vocab} in slices of {step} rows is not served")
    for n0 in range(0, vocab, step):
        rows = min(step, vocab - n0)
        w = ops.lm8_dequantize(w8, n0, rows, out=scratch[:rows])
        ops.gemm_f16w(xn, w, out=out if rows == vocab else out[:, n0:n0 + rows])
    return out


_GRAPH_STATE_PRIMED = set()


class _no_gc:
    """no cyclic garbage collection while a hipGraph is being captured: a collection that happens to run inside the capture may finalise a DEAD runner
    (HF models sit in reference cycles: they die only when the collector runs) -- its hipGraph and pool memory are then destroyed in the middle of the
    stream capture, which HIP answers by aborting the process.  (``torch.cuda.graph`` collects once on entry; this keeps it from happening again
    before the capture has ended.)"""

    def __enter__(self):
        import gc
        self.was = gc.isenabled()
        gc.collect()
        gc.disable()

    def __exit__(self, *exc):
        import gc
        if self.was:
            gc.enable()
        return False


def _prime_graph_state(dev):
    """torch allocates the per-device tensors its hipGraph captures keep the RNG seed / offset in at the FIRST capture, in whatever mode is current, and
    updates them in place at every later capture.  A first capture under ``torch.inference_mode()`` (the reference's harness decorates every loop with
    it, amq/utils/speed.py:14, 21, 49, 129) makes them inference tensors, and the next capture outside it raises "Inplace update to inference tensor":
    one empty capture outside inference mode, once per device, before any runner captures."""
    key = (dev.type, dev.index)
    if key in _GRAPH_STATE_PRIMED or dev.type != "cuda":
        return
    with torch.inference_mode(False):
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            keep = torch.zeros(1, device=dev)
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                keep += 1
        side.synchronize()
    _GRAPH_STATE_PRIMED.add(key)


def capture_graph(dev, fn, restore=None):
    """``fn()`` captured into a hipGraph on a side stream: one un-captured call first (allocator, lazy init), then ``restore()`` (puts back what that
    call consumed), then the capture -- with no garbage collection inside it (``_no_gc``) -- and the streams joined.  Returns the graph."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        if restore is not None:
            restore()
        g = torch.cuda.CUDAGraph()
        with _no_gc(), torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    return g


def _ints(values, n, lo, hi, message):
    """``n`` ints in lo .. hi from an int (taken ``n`` times), a list or a tensor; otherwise ValueError(message.format(got=...))"""
    each = [int(values)] * n if isinstance(values, int) else [int(v) for v in (values.reshape(-1).tolist() if isinstance(values, torch.Tensor) else values)]
    if len(each) != n or not all(lo <= v <= hi for v in each):
        raise ValueError(message.format(got=each))
    return each


def check_kv_bits(kv_bits):
    if kv_bits not in (8, 16):
        raise ValueError(f"kv_bits must be 16 (fp16 cache) or 8 (int8 rows with a scale per row), got {kv_bits!r}")
    return int(kv_bits)


def check_lm_head_bits(lm_head_bits):
    if lm_head_bits not in (16, 8, 4):
        raise ValueError(f"lm_head_bits must be 16 (fp16 lm_head), 8 (the LM8 layer) or 4 (a packed 4-bit layer), got {lm_head_bits!r}")
    return int(lm_head_bits)


# The two A/B routes of the token step, as the messages call them: the one-launch-per-token engine (ops.DecodeEngine; engine=True) and q/k/v +
# attention as one launch (ops.gemv_qkv_attn; the class switch FUSE_QKV_ATTN).  Both run ONE row at ONE position over a short fp16 cache in front of
# the fp16 lm_head.  What they require is written twice only: runner_options' no_route calls (an option that excludes them) and route_reasons.
ROUTES = {"engine": "the decode engine", "fuse_qkv_attn": "the fused q/k/v + attention launch"}
ENGINE_MAX_SEQ = 512            # the single-workgroup-per-head attention regime (the same bound as ops.ATTN_SPLIT_FROM)
FUSE_UNFIT = "the fused q/k/v + attention launch needs batch 1, a short cache, hidden_size <= 8192, groups of 128 and no biases"     # (never raised)
RunnerOptions = NamedTuple("RunnerOptions", [("B", int), ("R", int), ("ragged", bool), ("lookup", int), ("ngram_max", int), ("lookup_sampling", bool),
                                             ("kv_bits", int), ("lm_head_bits", int), ("engine", object)])


def runner_options(batch=1, ragged=False, lookup=0, ngram_max=2, lookup_sampling=False, kv_bits=16, lm_head_bits=16, engine=None,
                   fuse_qkv_attn=False, qk_norm=False):
    """A runner's options checked against each other, the two A/B routes (``engine`` as requested, ``fuse_qkv_attn``: the class switch) and the
    config's ``qk_norm`` -- host logic, before anything is built: ValueError for what is not offered (the first broken rule wins), else RunnerOptions
    (R: rows of a token step -- B, or lookup + 1 rows of the one sequence; engine: as requested -- None = QuantLlama.ENGINE_DEFAULT)"""
    def no_route(*messages):        # an option neither A/B route serves: (the engine's message, the fused launch's)
        for asked, message in zip((engine, fuse_qkv_attn), messages):
            if asked:
                raise ValueError(message)

    kv_bits, lm_head_bits = check_kv_bits(kv_bits), check_lm_head_bits(lm_head_bits)
    if lm_head_bits != 16:
        no_route(f"lm_head_bits={lm_head_bits}: not offered with the decode engine (an A/B route: it is followed by the fp16 lm_head only)",
                 f"lm_head_bits={lm_head_bits}: not offered with the fused q/k/v + attention launch (an A/B route: fp16 lm_head only)")
    if kv_bits == 8:
        if ragged:
            raise ValueError("kv_bits=8: the 8-bit attention kernel keeps one position for the batch: not offered with ragged=True")
        if lookup:
            raise ValueError("kv_bits=8: a verify step runs 2 .. 8 rows of one sequence, the 8-bit attention kernel one: not offered with lookup=")
        if qk_norm:
            raise ValueError("kv_bits=8: the 8-bit attention kernel has no per-head q / k norm: not offered for a qk_norm model")
        no_route("kv_bits=8: the decode engine reads an fp16 cache", "kv_bits=8: the fused q/k/v + attention launch reads an fp16 cache")
    if not 1 <= int(batch) <= 8:
        raise ValueError("batch must be 1..8")
    B, ragged, D = int(batch), bool(ragged), int(lookup or 0)
    if lookup_sampling and not D:
        raise ValueError("lookup_sampling: sampled verify steps need a runner built with lookup=D (a plain runner samples after set_sampling)")
    if D:
        if not 1 <= D <= ops.LOOKUP_MAX_ROWS - 1:
            raise ValueError(f"lookup: 1..{ops.LOOKUP_MAX_ROWS - 1} drafts per step (the 2 .. 8-row launches), got {lookup}")
        if not 1 <= int(ngram_max) <= 4:
            raise ValueError(f"ngram_max must be 1..4, got {ngram_max}")
        if B != 1:
            raise ValueError("lookup: the rows of a step are the drafts of ONE sequence (batch 1); batches are not served")
        if ragged:
            raise ValueError("lookup: a ragged runner's step-state blocks are sequences, a lookup runner's are the rows of one sequence: not offered with ragged=True")
        no_route("lookup: the decode engine runs one row per launch; a verify step runs 2 .. 8",
                 "lookup: the fused q/k/v + attention launch runs one row; a verify step runs 2 .. 8")
    if ragged:
        no_route("the decode engine keeps one position (batch 1): not offered with ragged=True",
                 "the fused q/k/v + attention launch keeps one position (batch 1): not offered with ragged=True")
    return RunnerOptions(B, D + 1 if D else B, ragged, D, int(ngram_max), bool(lookup_sampling), kv_bits, lm_head_bits, engine)


def route_reasons(route, *, R, ragged, kv_bits, fine, owq, has_bias, qk_norm, qd, H, max_seq):
    """Why ``route`` (a key of ROUTES) cannot serve a runner of these options and model facts (fine: groups of 64 / 32; qd: heads * 128), in the
    order a request is refused with them: what has a message of its own first, the generic line for everything else last; [] = it can"""
    what, reasons = ROUTES[route], []
    if fine and route == "engine":
        reasons.append("the decode engine serves groups of 128")
    if owq:
        reasons.append(what + " does not serve a model with OWQ layers: their gather and outlier columns run as a stage launch in front of each "
                       "packed GEMV (the five-launch step's staged plan)")
    if qk_norm or qd != H:      # both rotate inside launches of their own, which carry no per-head norm and take q / o of hidden_size: not for Qwen3
        reasons.append(what + " does not serve this model: "
                       + ("it has no per-head q / k norm" if qk_norm else f"q / o widths of heads * 128 = {qd} != hidden_size {H}"))
    fits = R == 1 and not fine and not has_bias and not ragged and kv_bits == 16
    if route == "engine" and not (fits and max_seq <= ENGINE_MAX_SEQ):
        reasons.append("the decode engine needs batch 1 and max_seq <= %d" % ENGINE_MAX_SEQ)
    if route == "fuse_qkv_attn" and not (fits and max_seq <= ops.ATTN_SPLIT_FROM and H <= 8192):
        reasons.append(FUSE_UNFIT)
    return reasons


# how a norm of the token step runs / which form down_proj takes (StepPlan)
NORM_FUSED, NORM_LAUNCH, NORM_FROM_SUMS = "fused", "launch", "sums"
DOWN_FUSED, DOWN_GEMV, DOWN_GEMV_SUMS, DOWN_GEMM = "silu_mul prologue", "silu_mul + gemv", "silu_mul + gemv leaving sums", "silu_mul + gemm"


class StepPlan(NamedTuple):
    """the launches of a token step of R rows that depend on R"""
    first_norm: str     # block 0's first norm (its x comes from the embedding: nothing left sums for it): NORM_FUSED | NORM_LAUNCH
    norm: str           # every other norm: NORM_FUSED (RMSNorm prologue of the q/k/v and gate/up launches) | NORM_LAUNCH (an rmsnorm launch in front
    #                     of them) | NORM_FROM_SUMS (from the partial sums of squares the o_proj / down_proj launch left: ops.gemv_grouped_sums)
    down: str           # down_proj: DOWN_FUSED (the GEMV with the SiLU*mul prologue) | silu_mul and DOWN_GEMV (the plain GEMV) | DOWN_GEMV_SUMS (the
    #                     GEMV leaving sums) | DOWN_GEMM (the few-row MFMA kernel: the rows do not fit the GEMV's LDS stage even in two K phases)
    staged: bool = False    # a model with OWQ layers: every sibling set runs ops.owq_stage (its norm / SiLU*mul, the gathers, the outlier partials) and
    #                         then one plain GEMV per sibling (QuantLlama._step_staged); first_norm / norm / down are then not looked at

    @property
    def block_norm(self):
        """the first norm of blocks 1 ..: rides on down_proj's sums only where down_proj leaves them"""
        return self.first_norm if self.norm == NORM_FROM_SUMS and self.down != DOWN_GEMV_SUMS else self.norm


def step_plan(R, H, I, fine, rows_h, rows_i, rows_i_phased, norm_sums=True, norm_fused_rows=4, down_fused_rows=1, rows_q=None):
    """The StepPlan of R rows at hidden size H / intermediate size I (``fine``: groups of 64 / 32).  rows_h, rows_i, rows_i_phased: the rows the
    GEMV stages in LDS -- ops.gemv_max_rows(H, plain=True), (I, plain=not fine) and (I, plain=not fine, norm=False: in two K phases).
    norm_sums, norm_fused_rows, down_fused_rows: QuantLlama.NORM_SUMS, NORM_FUSED_ROWS, DOWN_FUSED_ROWS.
    rows_q: ops.gemv_max_rows(heads * 128, plain=True) where o_proj's input is not H wide (Qwen3: q / o widths of heads * 128) -- the launch that
    leaves the sums stages rows of THAT width; None: H, as for every other family.
    A fused prologue is paid once per WORKGROUP, on R times the one-row bytes, a separate launch once per token: SiLU*mul leaves the GEMV from 2
    rows, the norms from 5 (profiles/r05_decode_batch.txt) -- where at 2 .. 8 rows they ride on partial sums instead (no pass over x for the
    statistic, no rmsnorm launch: profiles/r06_decode_batch.txt).  Past the whole-row LDS stage (7B: 7 - 8 rows of 11008) the plain GEMV stages x
    in two K phases (a fused prologue there would take in gate AND up per workgroup -- 352 KB per CU at 8 rows: 23.9 us against 4.9 + ~11)."""
    own = NORM_LAUNCH if R > norm_fused_rows else NORM_FUSED
    sums = norm_sums and 2 <= R <= 8 and not fine and 2048 <= H <= 8192 and I >= 2048 and R <= rows_h and (rows_q is None or R <= rows_q)
    if R <= min(rows_i, down_fused_rows):
        down = DOWN_FUSED
    elif R <= rows_i_phased:
        down = DOWN_GEMV_SUMS if sums else DOWN_GEMV
    else:
        down = DOWN_GEMM
    return StepPlan(own, NORM_FROM_SUMS if sums else own, down)


class _held_back:
    """token ids (the EOS ids) held back from a runner's choice until ``release()`` -- the first ``min_new_tokens`` tokens of a generate loop --;
    what was suppressed before is back on exit, however the loop ends"""

    def __init__(self, runner, ids, hold):
        self.runner, self.ids, self.held = runner, tuple(ids), bool(hold)

    def __enter__(self):
        self.before = self.runner.suppressed
        if self.held:
            self.runner.set_suppressed(self.before + tuple(e for e in self.ids if e not in self.before))
        return self

    def release(self):
        if self.held:
            self.runner.set_suppressed(self.before)
            self.held = False

    def __exit__(self, *exc):
        self.runner.set_suppressed(self.before)
        return False


class QuantLlama:
    ENGINE_MAX_SEQ = ENGINE_MAX_SEQ     # (decode steps run as ONE launch per token, ops.DecodeEngine, where asked for and route_reasons has nothing against it)
    # rows up to which down_proj's SiLU*mul stays fused into its GEMV's prologue (beyond: one silu_mul launch + the GEMV without a prologue -- every
    # workgroup of a fused launch takes in gate AND up and repeats the transform on all rows, which from 2 rows on costs more than the extra launch:
    # profiles/r05_decode_batch.txt)
    DOWN_FUSED_ROWS = 1
    # rows up to which the two RMSNorms stay fused into the q/k/v and gate/up launches (beyond: one rmsnorm launch + the grouped GEMV without a prologue)
    NORM_FUSED_ROWS = 4
    # one row (R == 1, plan.down == DOWN_FUSED): gate_proj's epilogue stores fp16(silu(gate)) and down_proj's prologue only multiplies by up -- SiLU once
    # per element (16 threads of the workgroup that owns the row-tile) instead of once per element in EVERY workgroup of the down_proj launch
    # (256 x 11008 on 7B), ahead of its first MFMA.  The same bits (tests/test_gpu_gate_act.py); profiles/silu_epilogue.txt.  False = A/B: SiLU*mul
    # in down_proj's prologue.  Groups of 64 / 32 (``fine``) keep the old prologue: the library offers the new forms at groups of 128 only.
    GATE_ACT = True
    NORM_SUMS = True            # (A/B switch of the partial-sum RMSNorm at 2 .. 8 rows: False = fused prologue up to NORM_FUSED_ROWS, one rmsnorm launch per norm beyond)
    # q/k/v + attention of a block as ONE launch (ops.gemv_qkv_attn; batch 1, short cache, hidden <= 8192): 4 launches per block
    # instead of 5.  Built, bit-identical (tests/test_gpu_qkv_attn.py) and SLOWER -- 15.7 us per fused launch against 9.2 + 5.1,
    # 755 vs 830 tokens/s (profiles/r03_qkv_attn_fused_negative.txt) -- so it is off unless a caller sets fuse_qkv_attn.
    FUSE_QKV_ATTN = False
    # cache length (max_seq) from which a lookup runner of a grouped-query model (2 .. 16 query heads per kv head) takes the matrix-core rows attention
    # (ops.attn_decode_rows(grouped=True)); None: never.
    # Measured per launch (profiles/lookup_gqa.json): at 2048 / 8192 / 32768 rows of cache it wins at every measured (heads, R) -- 13.2 -> 11.1 us
    # (32/8 heads, R = 2, 2048) up to 787 -> 63 us (64/8, R = 8, 32768) -- so the threshold is its floor; shorter caches were not measured and keep the
    # per-head kernels (every grouped-query lookup runner of the older tests keeps its arithmetic).
    ROWS_GQA_FROM = 2048
    # many-row logits over the 8-bit lm_head: vocabulary rows dequantized at a time (the fp16 scratch: 128 MB at H = 4096), and the row count from
    # which that route is taken.  One pass of the dequantize kernel over the whole layer moves what about three 8-row launches of the
    # weight-streaming kernel move (codes read, fp16 written), and the GEMM comes on top: 64 rows = 8 launches is past that by a safe factor.
    # Reasoned, not tuned; profiles/lm_head_bits.json has both routes at 2048 rows.
    LM8_SLICE_ROWS = 16384
    LM8_SLICED_FROM = 64
    _lm8_scratch = None
    ENGINE_DEFAULT = False      # what engine=None means (the engine is opt-in until it beats the five-launch step: HISTORY.md 3.2b)
    # prompt passes also leave the logits of EVERY prompt row in self.logits_rows [B, S, vocab] (HF's forward returns them all; the runner's own
    # generate loop needs the last row only): final norm + one fp16 GEMM over the prompt rows, inside the captured prompt graph (hf_fast.py sets it)
    all_logits = False
    engine = None               # the ops.DecodeEngine of a runner that takes that route (set by _take_routes)
    fine = False                # any layer with groups of 64 / 32 (set by __init__)
    owq = False                 # any OWQ layer (set by __init__): the staged token step, the plain prompt passes

    @classmethod
    def rows_attention_grouped(cls, n_heads, n_kv_heads, max_seq):
        """whether a lookup runner of these heads and this cache length takes the grouped rows attention (the ``grouped=`` of ops.attn_decode_rows)"""
        if cls.ROWS_GQA_FROM is None or n_kv_heads < 1 or n_heads % n_kv_heads:
            return False
        return 2 <= n_heads // n_kv_heads <= 16 and max_seq >= cls.ROWS_GQA_FROM

    def __init__(self, config, arch_linear=None, device="cuda:0", max_seq=256, seed=0, synthetic=True,
                 hqq_layers=None, dense=None, batch=1, engine=None, prebuilt=None, group=128, rope=None, ragged=False, lookup=0, ngram_max=2,
                 lookup_sampling=False, kv_bits=16, lm_head_bits=16, lm_head_packed=None):
        """config: an entry of arch.MODEL_CONFIGS (or its name).
        arch_linear: {'self_attn.q_proj': [bits]*n_block, ...}; default uniform 4.
        hqq_layers: {(block, name): HQQWeights} real quantized layers (else synthetic).
        dense: {'embed','lm_head','norm','ln1'[n_block],'ln2'[n_block]} fp16 tensors (else synthetic); a config with ``qk_norm`` (Qwen3) also
        'qn'[n_block], 'kn'[n_block]: the per-head q / k RMSNorm weights, fp16 [128] each.
        prebuilt: {(block, name): _Lin} linears already in the native layout (from_hf: shared with the modules that own them).
        group: group size of the SYNTHETIC layers (128; 64 / 32: see ``fine``).
        batch: sequences decoded together, 1 .. 8 (same prompt length; one step = the same launches with ``batch`` rows: the
        weights are streamed once per step for all of them).  batch = 1 is the reference's FT configuration.
        ragged: every sequence keeps a position of its own (prompts of unequal length: ``prefill(ids, lengths=...)``): one step-state block per
        sequence, the per-sequence forms of the attention / tail / set_token launches.  False: ONE position for the batch -- the object, graphs and
        bits the runner has always had.
        lookup: D = 1 .. 7 -- prompt-lookup speculative decoding (greedy, batch 1): every step runs R = D + 1 rows of the ONE sequence, the current token
        and D continuations guessed from the sequence's own history (the most recent earlier occurrence of its last ``ngram_max`` .. 1 tokens), verifies
        them in one pass of the weights and emits 1 + (accepted drafts) tokens: ``generate`` / ``verify_step`` / ``lookup_stats``.  The output is a
        greedy decode whatever is proposed.  0: off -- the object, graphs and bits the runner has always had.
        lookup_sampling: a lookup runner that also serves ``set_sampling``: the verify step then ends in the sampled lookup tail (every row's token is
        DRAWN, a draft is accepted while it equals the draw of the row in front of it, and the token emitted at index i is always drawn with draw
        counter i), so the output is what one-row sampled decoding draws from the same logits, whatever is proposed.  False: ``set_sampling`` is
        refused, as lookup runners always have.
        rope: (inv_freq fp32 [64], attention_scaling) of the rotary embedding when it is not the plain ``rope_theta`` form (from_hf hands over
        the HF module's own; otherwise derived from config["rope_scaling"]: Llama-3.1's "llama3").
        kv_bits: 16 -- the fp16 KV cache, the object, graphs and bits the runner has always had; 8 -- int8 rows with one fp32 scale per (sequence,
        kv head, position) (blocks hold kc8 / ks / vc8 / vs, 132 bytes per row instead of 256; the token step issues
        ops.attn_decode_kv8, the prompt pass stays exact fp16 and stores its rows with one ops.kv8_store; no prompt pass at start_pos > 0).
        lm_head_bits: 16 -- the fp16 lm_head, the object, graphs and bits the runner has always had; 8 -- the lm_head is quantized once, here, to
        the LM8 layer (hqq_format.quantize_lm8) and every logit comes from ops.lm8_gemv; 4 -- ops.hqq_quantize(W, 4) and the packed
        GEMV / GEMM kernels of the block linears.  The runner then keeps no fp16 lm_head (self.lm_head is None; self.lm_head_q is the packed layer).
        lm_head_packed: the packed layer of an earlier runner over the same weights (hf_fast shares one among the runners it builds), instead of
        quantizing again.  What is not offered with what: runner_options, route_reasons ("Runner options")."""
        config = MODEL_CONFIGS[config] if isinstance(config, str) else config
        opts = runner_options(batch, ragged, lookup, ngram_max, lookup_sampling, kv_bits, lm_head_bits, engine, self.FUSE_QKV_ATTN, config.get("qk_norm"))
        self._frame(config, device, max_seq, opts)
        self.arch_linear = arch_linear or uniform_arch(config, 4)["linear"]
        gen = torch.Generator(device=self.dev).manual_seed(seed)
        self.blocks = [{**{name: self._linear(b, name, gen, prebuilt, hqq_layers, synthetic, group) for name in config["linear"]},
                        **self._block_norms(b, gen, dense), **self._alloc_cache()} for b in range(self.nb)]
        self._dense_tensors(gen, dense, lm_head_packed)
        self._model_facts()
        self._alloc_step_buffers()
        # the cos/sin table every rotating kernel reads: plain rope_theta frequencies, or the rotary embedding's own (rope_scaling)
        self._init_step_state(rope if rope is not None else rope_inv_freq(config))
        self._plan_step()
        self._take_routes(opts.engine)

    # ----------------------------------------------------------------- construction, step by step (DenseLlama takes the same steps around its linears)
    def _frame(self, config, device, max_seq, opts):
        """what a runner knows before it has weights: its options (a RunnerOptions) and the model's dimensions"""
        self.B, self.R, self.ragged, self.lookup, self.ngram_max, self.lookup_sampling, self.kv_bits, self.lm_head_bits = opts[:8]
        self.cache_keys = ("kc8", "ks", "vc8", "vs") if self.kv_bits == 8 else ("kc", "vc")     # a block's cache tensors: codes and scales, or fp16 rows
        self.cfg, self.dev = config, torch.device(device)
        _prime_graph_state(self.dev)
        self.H, self.I = config["hidden_size"], config["intermediate_size"]
        self.nh, self.nkv = config["num_heads"], config["num_kv_heads"]
        if config["head_dim"] != 128:
            raise ValueError("head_dim must be 128")
        self.kvd, self.qd = self.nkv * 128, self.nh * 128       # qd: width of q and of the attention output = o_proj's K (Qwen3: not H at every size)
        self.qk_norm = bool(config.get("qk_norm"))      # Qwen3: q and k are RMS-normalised per head in front of the rotation, inside the rotating kernels
        self.nb, self.vocab, self.max_seq = config["n_block"], config["vocab_size"], max_seq
        self.eps = float(config.get("rms_norm_eps", EPS))
        self.theta = float(config.get("rope_theta", ROPE_THETA))

    def _linear(self, block, name, gen, prebuilt=None, hqq_layers=None, synthetic=True, group=128):
        """the _Lin of a block's linear: the prebuilt one, the HQQ layer repacked, or a synthetic one (with the q/k/v bias of a qkv_bias config)"""
        config, dev = self.cfg, self.dev
        n, k = config["linear_shape"][name]
        bits = arch_bits(self.arch_linear, name, block)
        if prebuilt is not None:
            l = prebuilt[(block, name)]
            assert l.bits == bits and (l.N, l.K) == (n, k) and l.qn.device == dev
            return l
        if hqq_layers is not None:
            h: HQQWeights = hqq_layers[(block, name)].to(dev)
            assert h.nbits == bits and tuple(h.shape) == (n, k)
            qn, mn = ops.repack_from_hqq(h.W_q.contiguous(), h.scale.reshape(-1).contiguous(),
                                         h.zero.reshape(-1).contiguous(), bits, n, k, group=h.group_size)
            return _Lin(qn, mn, bits, ops.MODE_HQQ, n, k, None if h.bias is None else h.bias.to(dev, torch.float16).contiguous())
        if not synthetic:
            raise ValueError("no weights given")
        l = _synthetic_linear(n, k, bits, gen, dev, group)
        if config.get("qkv_bias") and name in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"):
            l.bias = (0.1 * torch.randn(n, device=dev, generator=gen)).to(torch.float16)
        return l

    def _block_norms(self, b, gen, dense=None):
        """block b's norm weights -- ln1, ln2 and (qk_norm) qn, kn: ``dense``'s, or synthetic ones drawn in that order"""
        names = ("ln1", "ln2") + (("qn", "kn") if self.qk_norm else ())
        if dense is not None:
            return {name: dense[name][b].to(self.dev) for name in names}
        return {name: (1.0 + 0.05 * torch.randn(128 if name in ("qn", "kn") else self.H, device=self.dev, generator=gen)).to(torch.float16)
                for name in names}

    def _alloc_cache(self):
        """a block's cache tensors, zeroed, under self.cache_keys"""
        if self.kv_bits == 8:
            return dict(zip(self.cache_keys, ops.kv8_alloc(self.B, self.nkv, self.max_seq, self.dev)))
        return {key: torch.zeros(self.B, self.nkv, self.max_seq, 128, dtype=torch.float16, device=self.dev) for key in self.cache_keys}

    def _dense_tensors(self, gen, dense=None, lm_head_packed=None):
        """embedding, lm_head and final norm: ``dense``'s, or synthetic ones drawn in that order (after every block's draws); then the packed lm_head"""
        if dense is not None:
            self.embed, self.lm_head, self.norm = (dense[name].to(self.dev) for name in ("embed", "lm_head", "norm"))
        else:
            self.embed = (torch.randn(self.vocab, self.H, device=self.dev, generator=gen)).to(torch.float16)
            self.lm_head = (torch.randn(self.vocab, self.H, device=self.dev, generator=gen) / math.sqrt(self.H)).to(torch.float16)
            self.norm = (1.0 + 0.05 * torch.randn(self.H, device=self.dev, generator=gen)).to(torch.float16)
        self.lm_head_q = None
        if self.lm_head_bits != 16:
            # quantized once, here; the fp16 tensor is dropped (from_hf: the HF module keeps its own) so that no path can read a dense lm_head
            self.lm_head_q = lm_head_packed if lm_head_packed is not None else self.pack_lm_head(self.lm_head, self.lm_head_bits)
            self._check_lm_head_q()
            self.lm_head = None

    def _model_facts(self):
        """what the weights as built say about the model -- fine, owq, has_bias -- and the refusals of a model no token step serves"""
        linears = [blk[n] for blk in self.blocks for n in self.cfg["linear"]]
        # layers with groups of 64 / 32 (HQQ's default group_size is 64): the decode step is the same five launches (amq_gemv_grouped_f16 takes the
        # group size); the prompt pass leaves the fragment-ordered few-row kernels alone (they read one (scale, zero) pair per tile) and runs
        # dequantize-once + the fp16 GEMM per linear; the A/B step forms are not offered
        self.fine = any(l.mn.numel() != ops.native_sizes(l.bits, l.N, l.Kp)[1] // 2 for l in linears)
        # OWQ layers (from_hf over HIPOWQLinear modules): the token step runs the staged plan (_step_staged), the prompt passes their plain forms
        self.owq = any(l.owq for l in linears)
        self.has_bias = any(l.bias is not None for l in linears)
        if self.owq and self.fine:
            raise ValueError("a model with OWQ layers runs the staged token step, which serves groups of 128 only")
        # q/k/v and gate/up run as segments of ONE launch, which takes one group size: refuse a model that mixes them inside a sibling set here, at
        # build time (amq_gemv_grouped_f16 would refuse it at the first decode step; patching._same_group keeps such siblings apart on the HF side)
        for bi, blk in enumerate(self.blocks):
            for sibs in (("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), ("mlp.gate_proj", "mlp.up_proj")):
                pairs = {blk[n].mn.numel() * 128 // (2 * blk[n].N * blk[n].Kp) for n in sibs}      # (scale, zero) pairs per 128 columns: 1 / 2 / 4
                if len(pairs) != 1:
                    raise ValueError(f"block {bi}: {', '.join(sibs)} mix group sizes ({sorted(128 // p for p in pairs)}); the runner issues them as "
                                     "one grouped launch, which needs one group size per sibling set")

    def _alloc_step_buffers(self):
        """the activations of a token step of R rows (xn: normed rows, NORM_LAUNCH)"""
        for name, width in (("x", self.H), ("xn", self.H), ("q", self.qd), ("k", self.kvd), ("v", self.kvd), ("att", self.qd), ("gate", self.I), ("up", self.I)):
            setattr(self, name, torch.zeros(self.R, width, dtype=torch.float16, device=self.dev))

    def _plan_step(self):
        """which launches make up a step of R rows: decided here, once (the class switches as they stand now), walked by _step"""
        R = self.R
        self.plan = step_plan(R, self.H, self.I, self.fine, ops.gemv_max_rows(self.H, plain=True), ops.gemv_max_rows(self.I, plain=not self.fine),
                              ops.gemv_max_rows(self.I, plain=not self.fine, norm=False), self.NORM_SUMS, self.NORM_FUSED_ROWS, self.DOWN_FUSED_ROWS,
                              rows_q=None if self.qd == self.H else ops.gemv_max_rows(self.qd, plain=True))
        self._staged = None
        if self.owq:
            # no prologue, no partial sums, no activated gate: the stage launch forms the activation; a model without OWQ layers keeps the plan above
            self.plan = StepPlan(NORM_LAUNCH, NORM_LAUNCH, DOWN_GEMV, staged=True)
            self._staged = self._build_staged()
        # the sums of squares of self.x's rows, per 16 columns: written by the launch that produced the rows, read by the one that normalises them
        self.ss = torch.zeros(R, self.H // 16, dtype=torch.float32, device=self.dev) if self.plan.norm == NORM_FROM_SUMS else None

    def _take_routes(self, engine):
        """the two A/B routes by the one rule: can_fuse_qkv_attn / fuse_qkv_attn, and the engine where asked for (``engine``: None = ENGINE_DEFAULT)"""
        why_not = {route: route_reasons(route, R=self.R, ragged=self.ragged, kv_bits=self.kv_bits, fine=self.fine, owq=self.owq, has_bias=self.has_bias,
                                        qk_norm=self.qk_norm, qd=self.qd, H=self.H, max_seq=self.max_seq) for route in ROUTES}
        for route, asked in (("engine", engine), ("fuse_qkv_attn", self.FUSE_QKV_ATTN)):
            # a requested route with reasons: the first one (FUSE_QKV_ATTN holds for every runner of a class: where the launch merely does not fit
            # -- FUSE_UNFIT alone -- it stays off, silently)
            if asked and why_not[route] and why_not[route][0] != FUSE_UNFIT:
                raise ValueError(why_not[route][0])
        self.can_fuse_qkv_attn = not why_not["fuse_qkv_attn"]
        self.fuse_qkv_attn = self.FUSE_QKV_ATTN and self.can_fuse_qkv_attn
        self._tickets = torch.zeros(max(self.nh, 64), dtype=torch.int32, device=self.dev)
        if (self.ENGINE_DEFAULT if engine is None else engine) and not why_not["engine"]:
            self.engine = ops.DecodeEngine(
                [dict({n: dict(qn=blk[n].qn, mn=blk[n].mn, bits=blk[n].bits, mode=blk[n].mode, N=blk[n].N) for n in ops.ENGINE_LINEARS},
                      ln1=blk["ln1"], ln2=blk["ln2"], kc=blk["kc"], vc=blk["vc"]) for blk in self.blocks],
                self.H, self.I, self.nh, self.nkv, self.max_seq, self.eps, self.x.view(-1), self.rope_cur)

    def _init_step_state(self, rope):
        """everything a runner keeps besides weights, caches and activations (needs B, R, ragged, lookup, ngram_max, vocab, max_seq, theta, dev);
        ``rope``: (inv_freq fp32 [64] or None = plain rope_theta, attention_scaling)"""
        dev, R, max_seq = self.dev, self.R, self.max_seq
        self.logits = torch.zeros(self.vocab, dtype=torch.float16, device=dev) if R == 1 else torch.zeros(R, self.vocab, dtype=torch.float16, device=dev)
        self.logits_rows = None     # all_logits: [B, S, vocab] of the last prompt pass
        self.token = torch.zeros(R, dtype=torch.int64, device=dev)
        self.inv_freq, self.rope_scale = rope
        self.rope_tab = ops.rope_table(max_seq, self.theta, dev, inv_freq=self.inv_freq, scale=self.rope_scale)
        # step state: cos/sin row of self.pos + the position itself in one block (set_token / the step's tail keep it)
        # (ragged: one block per sequence -- rope_cur [B, 128], pos [B], step_err [B] -- and the prompt lengths the captured prompt pass reads)
        # (lookup: one block per ROW of the step -- block j at position p + j)
        self.rope_cur, self.pos, self.step_err = ops.new_step_state(dev, batch=R) if self.ragged or self.lookup else ops.new_step_state(dev)
        self.rope_cur.copy_(self.rope_tab.view(max_seq, 128)[0])
        self.host_pos = 0          # host mirror of self.pos (decode_step refuses to run past the cache without a device sync); ragged: of the LARGEST position
        self.lengths = torch.ones(R, dtype=torch.int64, device=dev) if self.ragged else None
        self.lookup_state = self.history = None
        if self.lookup:
            # the device block the verify-and-propose tail reads and keeps, and the token history (prompt + everything emitted)
            self.lookup_state, self.history = ops.new_lookup_state(dev, self.lookup, self.ngram_max, max_seq)
            self._row_offsets = torch.arange(R, dtype=torch.int32, device=dev)
            self._tok_in = torch.zeros(R, dtype=torch.int64, device=dev)
            self._prompt_len = 0
        # token ids the greedy choice never takes (8 slots, -1 = unused; read by the step's tail kernel): what HF's min_new_tokens does to the EOS ids
        # (set_suppressed; the values may change between replays of the captured step)
        self.suppress = torch.full((8,), -1, dtype=torch.int32, device=dev)
        self.suppressed = ()        # what self.suppress holds (read-only: set_suppressed)
        # sampled decoding (set_sampling / set_eos): the device block the sampled tail reads on every replay, and the sampled step's own graph beside
        # the greedy one (captured on first use; self.graph stays the greedy step)
        self.sampling = None        # None = greedy; else dict(temperature, top_k, top_p, seed)
        self.eos, self.pad_id = (), 0
        self.sample_state = None
        self._greedy_eos = False    # generate() runs greedy with EOS stop: the sampled tail taking the first maximum
        self.graph = self.sample_graph = None
        self._prefill_graphs = {}   # (prompt length, start_pos) -> (graph, its ids buffer, its logits_rows or None)

    def _qkn(self, blk):
        """what a rotating op of block ``blk`` takes besides its own arguments: the block's per-head q / k norm weights (Qwen3), or nothing"""
        return dict(q_norm=blk["qn"], k_norm=blk["kn"], norm_eps=self.eps) if self.qk_norm else {}

    # model families whose decoder is the Llama block -- RMSNorm, rotary q / k, (grouped-query) softmax attention, SiLU-gated MLP --
    # and differs only in shapes, rope settings, projection biases and (Qwen3) a per-head RMSNorm of q / k in front of the rotation: what the
    # reference lists (README.md:90-92; amq/configs/{llama,mistral,qwen2}.json) and Qwen3 dense
    HF_MODEL_TYPES = ("llama", "mistral", "qwen2", "qwen3")

    @classmethod
    def check_hf(cls, model, max_seq=None):
        """What ``from_hf`` needs of a swapped HF causal LM, checked without building anything: raises ValueError with the reason, returns
        (runner config, (inv_freq, attention_scaling) or None)."""
        from .checkpoint import runner_config
        hf = model.config.to_dict()
        mt = hf.get("model_type", "llama")
        if mt not in cls.HF_MODEL_TYPES:
            raise ValueError(f"from_hf: model_type '{mt}' is not one of {cls.HF_MODEL_TYPES} (a Llama-shaped decoder is required)")
        if hf.get("hidden_act", "silu") != "silu":
            raise ValueError("from_hf: a SiLU-gated MLP is required")
        for li, layer in enumerate(model.model.layers):
            cls._check_qk_norm(layer.self_attn, mt, float(hf.get("rms_norm_eps", 1e-5)), li)
        attn0 = model.model.layers[0].self_attn
        from .quant_linear import HIPOWQLinear, HIPQuantLinear
        if not isinstance(getattr(attn0, "q_proj", None), (HIPQuantLinear, HIPOWQLinear)):
            raise ValueError("from_hf: the decoder linears are not HIPQuantLinear modules: run prepare_for_inference(model, backend='hip') first")
        rp = hf.get("rope_parameters") or {}
        if hf.get("rope_theta") is None:
            hf["rope_theta"] = rp.get("rope_theta", 10000.0)
        rot = getattr(model.model, "rotary_emb", None)
        kind = getattr(rot, "rope_type", None) or rp.get("rope_type") or (hf.get("rope_scaling") or {}).get("rope_type", "default")
        rope = None
        if kind != "default":
            if kind not in ("llama3", "linear", "yarn") or rot is None or getattr(rot, "inv_freq", None) is None:
                raise ValueError(f"from_hf: rope type '{kind}' is not served (default, linear, llama3, yarn: the static ones)")
            rope = (rot.inv_freq.detach().to(torch.float32), float(getattr(rot, "attention_scaling", 1.0)))
            if rope[0].numel() != 64:
                raise ValueError("from_hf: head_dim must be 128")
        sw = hf.get("sliding_window")
        sliding = sw is not None and hf.get("use_sliding_window", True) is not False and \
            (not hf.get("layer_types") or any(t == "sliding_attention" for t in hf["layer_types"]))
        if sliding and max_seq is not None and max_seq > int(sw):
            raise ValueError(f"from_hf: max_seq {max_seq} exceeds the model's sliding window ({sw}): the runner attends the whole cache")
        cfg = runner_config(hf)
        return cfg, rope

    @staticmethod
    def _check_qk_norm(attn, model_type, eps, layer):
        """Qwen3's q_norm / k_norm: both RMSNorm modules over a head's 128 values with the model's rms_norm_eps -- what the rotating kernels apply;
        a model of another family has neither.  Anything else is refused with its reason."""
        qn, kn = getattr(attn, "q_norm", None), getattr(attn, "k_norm", None)
        where = f"from_hf: model.layers.{layer}.self_attn"
        if model_type != "qwen3":
            if qn is not None or kn is not None:
                raise ValueError(f"{where}: per-head q / k norms are not part of a '{model_type}' block (they are served for model_type 'qwen3')")
            return
        if qn is None and kn is None:
            raise ValueError(f"{where}: a qwen3 block without q_norm / k_norm")
        if qn is None or kn is None:
            raise ValueError(f"{where}: a norm on only one of q / k ({'q_norm' if kn is None else 'k_norm'} alone) is not served: the kernels "
                             "normalise both")
        for name, m in (("q_norm", qn), ("k_norm", kn)):
            w = getattr(m, "weight", None)
            if "RMSNorm" not in type(m).__name__ or w is None or tuple(w.shape) != (128,):
                raise ValueError(f"{where}.{name}: expected an RMSNorm over the 128 values of a head, got {type(m).__name__}"
                                 f"{'' if w is None else ' of width ' + 'x'.join(str(d) for d in w.shape)}")
            m_eps = getattr(m, "variance_epsilon", getattr(m, "eps", None))
            if m_eps is None or float(m_eps) != eps:
                raise ValueError(f"{where}.{name}: eps {m_eps} is not the model's rms_norm_eps {eps} (the runner keeps one eps)")

    @classmethod
    def from_hf(cls, model, max_seq=256, batch=1, engine=None, ragged=False, lookup=0, ngram_max=2, lookup_sampling=False, kv_bits=16,
                lm_head_bits=16, lm_head_packed=None):
        """The hipGraph runner over a SWAPPED HF causal LM of the Llama family (``HF_MODEL_TYPES``: Llama 2 / 3.x, Mistral, Qwen2.5) -- what
        ``prepare_for_inference(model, backend="hip")`` (or the reference's deepcopy + setattr assembly of a mixed-precision model,
        amq_speed_benchmark.py:231-256) leaves behind.  The runner shares the modules' native weight buffers and biases, the embedding, lm_head and
        norm weights (no copies) and the rotary embedding's own frequencies (rope_scaling: Llama-3.1); it is to the swapped model what the
        reference's ``use_ft`` monkeypatch is to its HF model (kernel/monkeypatch/ftllama_modeling.py): the same weights behind a static-cache,
        fused token step.  Needs fp16 weights on one GPU, head_dim 128, SiLU."""
        from .quant_linear import HIPOWQLinear, HIPQuantLinear
        cfg, rope = cls.check_hf(model, max_seq)
        layers = model.model.layers
        pre, arch_linear = {}, {name: [] for name in cfg["linear"]}
        dev = None
        f16 = lambda t: t.detach() if t.dtype is torch.float16 else t.detach().to(torch.float16)
        for b, layer in enumerate(layers):
            for name in cfg["linear"]:
                parent, attr = name.split(".")
                m = getattr(getattr(layer, parent), attr)
                if isinstance(m, HIPOWQLinear) and m.inner.qweight.is_cuda:
                    # an OWQ layer: the packed inner layer [N, Kp] (it holds the bias) and the module's own perm / out_ids / W_out, all shared
                    i = m.inner
                    if i.is_bf16:
                        raise ValueError(f"model.layers.{b}.{name}: a bfloat16 module -- the decode runner is fp16")
                    if m.perm.dtype is not torch.int32 or m.out_ids.dtype is not torch.int32 or m.W_out.dtype is not torch.float16 or \
                            tuple(m.W_out.shape) != (m.outfeatures, m.n_out) or m.perm.numel() != i.infeatures or m.out_ids.numel() != m.n_out:
                        raise ValueError(f"model.layers.{b}.{name}: the OWQ layer's perm / out_ids / W_out do not have the shapes of its packed layer")
                    dev = dev or i.qweight.device
                    pre[(b, name)] = _Lin(i.qweight, i.meta, i.bits, i.mode, m.outfeatures, m.infeatures, None if i.bias is None else f16(i.bias),
                                          perm=m.perm.contiguous(), out_ids=m.out_ids.contiguous(), W_out=m.W_out.contiguous(), Kp=i.infeatures)
                    arch_linear[name].append(i.bits)
                    continue
                if not isinstance(m, HIPQuantLinear) or not m.qweight.is_cuda:
                    raise ValueError(f"model.layers.{b}.{name}: expected a HIPQuantLinear on the GPU (run prepare_for_inference first)")
                if m.is_bf16:
                    raise ValueError(f"model.layers.{b}.{name}: a bfloat16 module -- the decode runner is fp16 (the reference's kernels are, ft.py:62); "
                                     "bf16 models run through the modules' own forward")
                dev = dev or m.qweight.device
                pre[(b, name)] = _Lin(m.qweight, m.meta, m.bits, m.mode, m.outfeatures, m.infeatures, None if m.bias is None else f16(m.bias))
                arch_linear[name].append(m.bits)
        dense = {"embed": f16(model.model.embed_tokens.weight), "lm_head": f16(model.lm_head.weight), "norm": f16(model.model.norm.weight),
                 "ln1": [f16(l.input_layernorm.weight) for l in layers], "ln2": [f16(l.post_attention_layernorm.weight) for l in layers]}
        if cfg.get("qk_norm"):                  # the HF modules' own tensors (no copy when they are fp16 and contiguous)
            dense["qn"] = [f16(l.self_attn.q_norm.weight).contiguous() for l in layers]
            dense["kn"] = [f16(l.self_attn.k_norm.weight).contiguous() for l in layers]
        return cls(cfg, arch_linear, device=dev, max_seq=max_seq, dense=dense, batch=batch, engine=engine, prebuilt=pre, synthetic=False, rope=rope,
                   ragged=ragged, lookup=lookup, ngram_max=ngram_max, lookup_sampling=lookup_sampling, kv_bits=kv_bits,
                   lm_head_bits=lm_head_bits, lm_head_packed=lm_head_packed)

    # ----------------------------------------------------------------- the lm_head
    @staticmethod
    def pack_lm_head(W, bits):
        """the packed lm_head of ``bits`` (8: hqq_format.LM8Weights; 4: a _Lin in the native layout) from the fp16 weights W [vocab, H] on the GPU"""
        vocab, H = W.shape
        if bits == 8:
            from .hqq_format import quantize_lm8
            if H % 128:
                raise ValueError(f"lm_head_bits=8: the LM8 layer has groups of 128 along the hidden size (got {H})")
            return quantize_lm8(W.contiguous())
        if vocab % 16 or H % 128:
            raise ValueError(f"lm_head_bits=4: the packed kernels need N % 16 == 0 and K % 128 == 0 (got a vocabulary of {vocab}, hidden size {H})")
        h = ops.hqq_quantize(W.contiguous(), 4)
        qn, mn = ops.repack_from_hqq(h.W_q.contiguous(), h.scale.reshape(-1).contiguous(), h.zero.reshape(-1).contiguous(), 4, vocab, H)
        return _Lin(qn, mn, 4, ops.MODE_HQQ, vocab, H)

    def _check_lm_head_q(self):
        q, want = self.lm_head_q, (self.vocab, self.H)
        if self.lm_head_bits == 8:
            ok = tuple(getattr(q, "shape", ())) == want and getattr(q, "nbits", 0) == 8 and q.codes.device == self.dev
        else:
            ok = isinstance(q, _Lin) and (q.N, q.K, q.bits) == want + (4,) and q.qn.device == self.dev
        if not ok:
            raise ValueError(f"lm_head_packed is not a {self.lm_head_bits}-bit lm_head of shape {want} on {self.dev}")

    def lm_head_bytes(self):
        """bytes of the lm_head a token step streams: fp16, or the packed layer's codes + meta"""
        return self.lm_head.numel() * 2 if self.lm_head_bits == 16 else self.lm_head_q.nbytes()

    def lm_head_weights(self):
        """the fp16 weights [vocab, H] the lm_head stands for (a packed one: dequantized, a new tensor)"""
        if self.lm_head_bits == 16:
            return self.lm_head
        if self.lm_head_bits == 8:
            return ops.lm8_dequantize(self.lm_head_q)
        q = self.lm_head_q
        return ops.dequantize(q.qn, q.mn, q.bits, q.mode, q.N, q.K)

    def _lm_logits(self, x, out):
        """out = lm_head(final RMSNorm(x)) for up to 8 hidden rows -- x [H] -> out [vocab], or x [M, H] -> out [M, vocab] --: the ONE place a token
        step, a prompt pass' last rows and the streamed many-row loop form logits.  16: the fp16 weight-streaming kernel with the norm as its
        prologue; 8: ops.lm8_gemv, the same shape; 4: the packed GEMV with the RMSNorm prologue as far as its LDS stage reaches
        (ops.gemv_max_rows(H)), an rmsnorm launch + the plain GEMV beyond (what _behind_norm does), the GEMM past that"""
        if self.lm_head_bits == 16:
            return ops.gemv_f16w(x, self.lm_head, gamma=self.norm, eps=self.eps, out=out)
        if self.lm_head_bits == 8:
            return ops.lm8_gemv(x, self.lm_head_q, gamma=self.norm, eps=self.eps, out=out)
        q = self.lm_head_q
        x2, y = x.reshape(-1, self.H), out.view(-1, self.vocab)
        M = x2.shape[0]
        if M <= ops.gemv_max_rows(self.H):
            ops.gemv_grouped(x2, [q.seg(y)], self.H, prologue=ops.PRO_RMSNORM, gamma=self.norm, eps=self.eps)
        elif M <= ops.gemv_max_rows(self.H, plain=True, norm=False):
            ops.gemv_grouped(ops.rmsnorm(x2, self.norm, self.eps), [q.seg(y)], self.H)
        else:
            ops.gemm(ops.rmsnorm(x2, self.norm, self.eps), q.qn, q.mn, q.bits, q.mode, q.N, q.K, out=y)
        return out

    def _lm_logits_many(self, x, out=None):
        """out [n, vocab] = lm_head(final RMSNorm(x [n, H])) for any number of rows (an all-logits prompt pass, a piece of score_rows).  16: one
        fp16 MFMA GEMM (the weight-streaming kernel, 8 rows a launch, for a vocabulary that is no multiple of 16: test models); 4: ops.gemm over
        the packed layer; 8: from LM8_SLICED_FROM rows on (and a vocabulary the fp16 GEMM takes) slices of LM8_SLICE_ROWS vocabulary rows dequantized
        into one bounded fp16 scratch and the fp16 GEMM on each slice, writing its columns of ``out`` (lm8_logits_sliced); fewer rows: the
        weight-streaming kernel, 8 rows a launch.  profiles/lm_head_bits.json has what a 2048-row window costs either way."""
        n = x.shape[0]
        if self.lm_head_bits == 8 and n >= self.LM8_SLICED_FROM and self.vocab % 16 == 0:
            if out is None:
                out = torch.empty(n, self.vocab, dtype=torch.float16, device=x.device)
            rows = min(int(self.LM8_SLICE_ROWS), self.vocab)
            if self._lm8_scratch is None or self._lm8_scratch.shape[0] != rows:
                self._lm8_scratch = torch.empty(rows, self.H, dtype=torch.float16, device=self.dev)
            return lm8_logits_sliced(ops.rmsnorm(x, self.norm, self.eps), self.lm_head_q, out, self._lm8_scratch)
        if self.lm_head_bits == 16 and self.vocab % 16 == 0:
            return ops.gemm_f16w(ops.rmsnorm(x, self.norm, self.eps), self.lm_head, out=out)
        if out is None:
            out = torch.empty(n, self.vocab, dtype=torch.float16, device=x.device)
        if self.lm_head_bits == 4:
            q = self.lm_head_q
            ops.gemm(ops.rmsnorm(x, self.norm, self.eps), q.qn, q.mn, q.bits, q.mode, q.N, q.K, out=out)
            return out
        return self._lm_head_streamed(x, out)

    # ----------------------------------------------------------------- sizes
    def linear_bytes_per_token(self):
        """algorithmic bytes of the quantized linears per decode token"""
        return sum(blk[name].nbytes() for blk in self.blocks for name in self.cfg["linear"])

    def total_bytes_per_token(self, context):
        kv = 2 * self.nb * self.nkv * (ops.KV8_ROW_BYTES if self.kv_bits == 8 else 256) * context       # K and V rows: 256 bytes of fp16, or 128 codes + a scale
        return self.linear_bytes_per_token() + self.lm_head_bytes() + kv

    # ----------------------------------------------------------------- decode
    def _step(self, sampled=False):
        """one token: reads self.x (= embed[self.token], kept in step by set_token / the step's own tail) and self.pos
        (device), writes self.logits, self.token, self.pos and the next step's self.x.  The launches are self.plan's."""
        H, plan = self.H, self.plan
        if plan.staged:
            return self._step_staged(sampled)
        if self.engine is not None:
            self.engine.step()
            self._lm_logits(self.x.reshape(-1), self.logits)
            self._tail(sampled)
            return
        if self.ragged and self.fuse_qkv_attn:
            raise ValueError("the fused q/k/v + attention launch keeps one position (batch 1): not offered with ragged=True")
        from_sums = plan.norm == NORM_FROM_SUMS
        first = plan.first_norm
        for blk in self.blocks:
            if self.fuse_qkv_attn:
                ops.gemv_qkv_attn(self.x, [blk["self_attn.q_proj"].seg(self.q.view(-1)), blk["self_attn.k_proj"].seg(self.k.view(-1)),
                                           blk["self_attn.v_proj"].seg(self.v.view(-1))], H, blk["ln1"], self.eps, blk["kc"], blk["vc"],
                                  self.att.view(-1), self.rope_cur, self.nh, self.nkv, self._tickets)
            else:
                self._behind_norm(first, blk["ln1"], [blk["self_attn.q_proj"].seg(self.q), blk["self_attn.k_proj"].seg(self.k),
                                                      blk["self_attn.v_proj"].seg(self.v)])
                self._step_attention(blk)
            o_proj, down = [blk["self_attn.o_proj"].seg(self.x, residual=self.x)], [blk["mlp.down_proj"].seg(self.x, residual=self.x)]
            if from_sums:
                ops.gemv_grouped_sums(self.att, o_proj, self.qd, sums_out=self.ss)
            else:
                ops.gemv_grouped(self.att, o_proj, self.qd)
            # (one row only: with DOWN_FUSED_ROWS raised a step of 2 .. 8 rows keeps SiLU*mul in down_proj's prologue -- its gate/up launch may be the
            #  partial-sum one, which takes no activated segment, and the activated gate at several rows is not measured)
            gate_act = self.GATE_ACT and self.R == 1 and plan.down == DOWN_FUSED and not self.fine
            self._behind_norm(plan.norm, blk["ln2"], [blk["mlp.gate_proj"].seg(self.gate, act=gate_act), blk["mlp.up_proj"].seg(self.up)])
            if plan.down == DOWN_FUSED:
                ops.gemv_grouped(self.gate, down, self.I, prologue=ops.PRO_SILU_MUL, x2=self.up, x_activated=gate_act)
            elif plan.down == DOWN_GEMV_SUMS:
                ops.gemv_grouped_sums(ops.silu_mul(self.gate, self.up, out=self.gate), down, self.I, sums_out=self.ss)
            elif plan.down == DOWN_GEMV:
                ops.gemv_grouped(ops.silu_mul(self.gate, self.up, out=self.gate), down, self.I)
            else:
                d = blk["mlp.down_proj"]
                ops.gemm(ops.silu_mul(self.gate, self.up, out=self.gate), d.qn, d.mn, d.bits, d.mode, d.N, d.K, bias=d.bias, residual=self.x, out=self.x)
            first = plan.block_norm
        self._lm_logits(self.x.reshape(-1) if self.R == 1 else self.x, self.logits)
        self._tail(sampled)

    # ------------------------------------------------- the staged plan (OWQ layers)
    def _build_staged(self):
        """The staged plan of a model with OWQ layers, built once: per block the four sibling sets (q/k/v behind ln1, o_proj, gate/up behind ln2,
        down_proj behind SiLU*mul) as (x, activation, gamma, x2, the ops.owq_stage_parts array or None, [(linear, its GEMV's x, K, y, residual)]).
        The stage launch of a set leaves every OWQ sibling's gathered rows in a buffer of its own and its outlier partial (+ the set's residual)
        in the sibling's output; the packed GEMV then reads the partial as its residual.  Plain siblings of a set read the staged activation
        itself (one shared part), with the set's residual.  A plain o_proj needs no stage: its activation is the attention output as it lies.
        The buffers are the runner's, allocated here."""
        R, dev = self.R, self.dev
        f16 = dict(dtype=torch.float16, device=dev)
        widths = {"self_attn.q_proj": self.H, "self_attn.k_proj": self.H, "self_attn.v_proj": self.H, "self_attn.o_proj": self.qd,
                  "mlp.gate_proj": self.H, "mlp.up_proj": self.H, "mlp.down_proj": self.I}
        self.xg = {n: torch.zeros(R * k, **f16) for n, k in widths.items()}       # per linear: [R, Kp] of the block at hand
        self.act = torch.zeros(R, self.I, **f16)                                    # SiLU*mul rows for a plain down_proj
        sets = []
        for blk in self.blocks:
            per = []
            for x, act, gamma, x2, plain_buf, names, outs, residual in (
                    (self.x, ops.OWQ_ACT_RMSNORM, blk["ln1"], None, self.xn, ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"),
                     (self.q, self.k, self.v), None),
                    (self.att, ops.OWQ_ACT_NONE, None, None, self.att, ("self_attn.o_proj",), (self.x,), self.x),
                    (self.x, ops.OWQ_ACT_RMSNORM, blk["ln2"], None, self.xn, ("mlp.gate_proj", "mlp.up_proj"), (self.gate, self.up), None),
                    (self.gate, ops.OWQ_ACT_SILU_MUL, None, self.up, self.act, ("mlp.down_proj",), (self.x,), self.x)):
                K = x.shape[1]
                parts, gemvs, shared = [], [], False
                for n, y in zip(names, outs):
                    l = blk[n]
                    if l.owq:
                        xg = self.xg[n][:R * l.Kp].view(R, l.Kp)
                        parts.append(dict(perm=l.perm, out_ids=l.out_ids, W_out=l.W_out, xg=xg, y=y, residual=residual))
                        gemvs.append((l, xg, l.Kp, y, y))
                    else:
                        if not shared and plain_buf is not x:
                            parts.append(dict(xg=plain_buf))
                        shared = True
                        gemvs.append((l, plain_buf, K, y, residual))
                per.append((x, act, gamma, x2, ops.owq_stage_parts(parts, R, K) if parts else None, gemvs))
            sets.append(per)
        return sets

    def _step_staged(self, sampled):
        """the token step of a model with OWQ layers: per sibling set one stage launch and one plain GEMV per sibling (12 launches a block where
        every linear has outliers); attention, lm_head and tail as in every step"""
        for blk, per in zip(self.blocks, self._staged):
            for i, (x, act, gamma, x2, arr, gemvs) in enumerate(per):
                if arr is not None:
                    ops.owq_stage_launch(x, self.R, x.shape[1], act, gamma, self.eps, x2, arr)
                for l, xin, K, y, residual in gemvs:
                    if self.R <= ops.gemv_max_rows(K, plain=True, norm=False):
                        ops.gemv_grouped(xin, [l.seg(y, residual=residual)], K)
                    else:
                        ops.gemm(xin, l.qn, l.mn, l.bits, l.mode, l.N, K, bias=l.bias, residual=residual, out=y)
                if i == 0:
                    self._step_attention(blk)
        self._lm_logits(self.x.reshape(-1) if self.R == 1 else self.x, self.logits)
        self._tail(sampled)

    def _step_attention(self, blk):
        """rotation, cache append and attention of a token step's rows: self.q / self.k / self.v -> self.att"""
        if self.lookup:                         # the R rows are consecutive positions of the one sequence: causal among them, one cache slice
            ops.attn_decode_rows(self.q, self.k, self.v, blk["kc"], blk["vc"], self.att, self.rope_cur, self.pos, self.nh, self.nkv,
                                 grouped=self.rows_attention_grouped(self.nh, self.nkv, self.max_seq), **self._qkn(blk))
        elif self.kv_bits == 8:
            ops.attn_decode_kv8(self.q, self.k, self.v, blk["kc8"], blk["ks"], blk["vc8"], blk["vs"], self.att, self.pos, self.nh, self.nkv,
                                cur=self.rope_cur)
        else:
            ops.attn_decode(self.q, self.k, self.v, blk["kc"], blk["vc"], self.att, self.pos, self.nh, self.nkv, self.theta,
                            cur=self.rope_cur, **self._qkn(blk))

    def _behind_norm(self, how, gamma, segments):
        """one grouped launch (q/k/v, gate/up) over self.x behind the RMSNorm ``gamma``, which runs as the plan says"""
        if how == NORM_FROM_SUMS:
            ops.gemv_grouped_sums(self.x, segments, self.H, gamma=gamma, eps=self.eps, sums_in=self.ss)
        elif how == NORM_LAUNCH:
            ops.gemv_grouped(ops.rmsnorm(self.x, gamma, self.eps, out=self.xn), segments, self.H)
        else:
            ops.gemv_grouped(self.x, segments, self.H, prologue=ops.PRO_RMSNORM, gamma=gamma, eps=self.eps)

    def _tail(self, sampled):
        """the end of a token step: the next token (arg-max, or a draw with the device block's parameters + EOS bookkeeping), pos += 1,
        x = embed[token], rope_cur = cos/sin row of the new position (per sequence; the position is shared).  A lookup runner: the
        verify-and-propose tail over the R rows, greedy or -- ``lookup_sampling=True`` -- with every row's token drawn"""
        if self.lookup and sampled:
            if not self.lookup_sampling:
                raise ValueError("lookup: speculative decoding here is greedy (the sampled tail draws one token per row)")
            ops.decode_tail_lookup_sample(self.logits, self.embed, self.token, self.pos, self.x, self.lookup_state, self.history, self.rope_tab,
                                          self.rope_cur, self.sample_state, suppress=self.suppress)
        elif self.lookup:
            ops.decode_tail_lookup(self.logits, self.embed, self.token, self.pos, self.x, self.lookup_state, self.history, self.rope_tab, self.rope_cur,
                                   suppress=self.suppress)
        elif sampled:
            ops.decode_tail_sample(self.logits, self.embed, self.token, self.pos, self.x, self.sample_state, table=self.rope_tab, cur=self.rope_cur,
                                   suppress=self.suppress)
        else:
            ops.decode_tail(self.logits, self.embed, self.token, self.pos, self.x, table=self.rope_tab, cur=self.rope_cur, suppress=self.suppress)

    # ------------------------------------------------------------- sampling
    EOS_POLL_STEPS = 16         # generate(stop_at_eos=True) reads the unfinished count every this many steps: fewer = less work after the last EOS, more host syncs

    def _write_sampling_state(self):
        if self.sample_state is None:
            self.sample_state = ops.new_sampling_state(self.dev)
        if self.sampling is not None:
            ops.set_sampling_state(self.sample_state, eos_ids=self.eos, pad_id=self.pad_id, **self.sampling)
        else:                                   # greedy with EOS stop: top_k = 1 and the first kept token = the first maximum, as the greedy tail takes it
            ops.set_sampling_state(self.sample_state, top_k=1, eos_ids=self.eos, pad_id=self.pad_id, first_kept=True)

    def set_sampling(self, temperature=1.0, top_k=0, top_p=1.0, seed=0):
        """Sampled decoding from the next prompt pass on: temperature, then top-k (0 = off), then top-p (1 = off), HF's order; ``seed`` fixes the
        whole sequence (counter-based generator: draw i of sequence b is a function of (seed, i, b) -- not torch.multinomial's stream).
        ``set_sampling(None)``: back to greedy.  Writes the device block only: the greedy step (self.graph) and the sampled step (self.sample_graph)
        are two graphs, each captured once, and switching re-captures neither.  A lookup runner serves this only when built with
        ``lookup_sampling=True`` (its sampled step ends in the sampled verify-and-propose tail); a default one refuses."""
        if temperature is None:
            self.sampling = None
            return
        if self.lookup and not self.lookup_sampling:
            raise ValueError("lookup: speculative decoding here is greedy; sampled speculative decoding (rejection sampling) is not served")
        self.sampling = dict(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), seed=int(seed))
        self._write_sampling_state()

    def set_eos(self, ids=(), pad_id=0):
        """EOS ids (at most 8) and the pad id of the sampled tail's bookkeeping: a sequence that emits an EOS id is finished and emits ``pad_id``
        from then on (HF: next * unfinished + pad * (1 - unfinished))"""
        ids = tuple(int(i) for i in ids)
        if len(ids) > 8:
            raise ValueError("at most 8 EOS ids")
        self.eos, self.pad_id = ids, int(pad_id)
        if self.sample_state is not None:
            self._write_sampling_state()

    def _sampled_tail(self):
        """the token steps end in the sampled tail: sampling is on, or generate() runs greedy with EOS stop (the sampled tail taking the first maximum)"""
        return self.sampling is not None or self._greedy_eos

    def _first_token(self):
        """the first token after a prompt pass when the sampled tail is in use: draw 0 of every sequence from the last rows' logits"""
        if self.lookup:                         # (the prompt graph ended in the greedy lookup tail: the same again with the token drawn)
            return self._lookup_first_token(self._prompt_len, sampled=True)
        tok = ops.sample(self.logits, self.sample_state, suppress=self.suppress, flags=ops.SAMPLE_ADVANCE | ops.SAMPLE_EOS)
        self.set_token(tok)

    def unfinished(self):
        """number of sequences that have not emitted an EOS id yet (one 4-byte read; synchronises)"""
        return int(self.sample_state[24].item())

    def set_suppressed(self, ids=()):
        """token ids greedy decoding must not pick (at most 8; () = none): HF's generate(min_new_tokens = max_new_tokens) never emits an EOS id.
        Takes effect from the next step / prompt pass, captured or not."""
        ids = tuple(int(i) for i in ids)
        if len(ids) > 8:
            raise ValueError("at most 8 suppressed token ids")
        if ids == self.suppressed:              # (no host-to-device copy for what is already there)
            return
        self.suppress.copy_(torch.tensor(ids + (-1,) * (8 - len(ids)), dtype=torch.int32))
        self.suppressed = ids

    def _argmax(self, logits):
        """arg-max over the vocabulary (the last dimension) of a prompt pass with the suppressed ids left out, as the captured step's tail kernel
        does; no host synchronisation (unused slots are pointed at a spare element behind the vocabulary)"""
        m = torch.zeros(self.vocab + 1, dtype=torch.float32, device=logits.device)
        m.index_fill_(0, torch.where(self.suppress >= 0, self.suppress, self.vocab).to(torch.int64), float("-inf"))
        return torch.argmax(logits.float() + m[:self.vocab], dim=-1)

    def set_pos(self, pos):
        """set the position of the next decode step (device state + its host mirror); follow with set_token().  A ragged runner also takes one
        position per sequence (a list or tensor of B)."""
        if self.ragged and not isinstance(pos, int) and (not isinstance(pos, torch.Tensor) or pos.numel() > 1 or self.B == 1):
            each = _ints(pos, self.B, 0, self.max_seq, f"expected {self.B} positions inside the KV cache (max_seq={self.max_seq}), got {{got}}")
            self.pos.copy_(torch.tensor(each, dtype=torch.int32))
            self.host_pos = max(each)
            return
        pos = int(pos)
        if not 0 <= pos <= self.max_seq:
            raise ValueError(f"position {pos} outside the KV cache (max_seq={self.max_seq})")
        if self.lookup:                         # block j = row j of the step: position pos + j (saturating, as the tail leaves them)
            self.pos.copy_((self._row_offsets + pos).clamp_(max=self.max_seq))
        else:
            self.pos.fill_(pos)
        self.host_pos = pos

    def check(self):
        """raise if any decode step ran with its device-side position outside the cache (synchronises)"""
        try:
            ops.check_step_state(self.step_err)
        except Exception:
            self._tickets.zero_()               # (the fused q/k/v + attention launch leaves a timed-out ticket as it is: include/amq_hip.h)
            raise
        if self.engine is not None:
            try:
                self.engine.check()
            except Exception:
                self.graph = None               # the engine re-zeroed its barrier words: the next decode_step re-captures
                raise

    def set_token(self, token):
        """make ``token`` (int or 1-element tensor) the input of the next decode step; also re-derives what the step
        reads besides the token (embedding row, cos/sin row of the current position) -- set_pos() first"""
        if self.lookup:
            return self._lookup_set_token(token)
        if isinstance(token, torch.Tensor) and token.is_cuda and token.dtype is torch.int64 and token.numel() in (1, self.B) and token.is_contiguous():
            # one launch instead of five framework ops (a caller that feeds every token itself pays this per token: hf_fast's forward)
            return ops.set_token(token, self.embed, self.token, self.pos, self.x, table=self.rope_tab, cur=self.rope_cur)
        if isinstance(token, torch.Tensor):
            self.token.copy_(token.reshape(-1).expand(self.B) if token.numel() == 1 else token.reshape(self.B))
        else:
            self.token.fill_(int(token))
        torch.index_select(self.embed, 0, self.token, out=self.x)
        rows = torch.index_select(self.rope_tab.view(self.max_seq, 128), 0, self.pos.to(torch.int64).clamp_(0, self.max_seq - 1))
        self.rope_cur.copy_(rows if self.ragged else rows[0])

    def _graph(self, sampled):
        """the captured token step: the one ending in the sampled tail, or the greedy one"""
        return self.sample_graph if sampled else self.graph

    def capture(self, sampled=False):
        """capture one token step into a hipGraph (replayed by decode_step); ``sampled``: the step that ends in the sampled tail, kept beside the greedy one"""
        if self._graph(sampled) is not None:
            return
        if self.host_pos >= self.max_seq:
            raise ValueError(f"cannot capture a decode step at position {self.host_pos}: the KV cache holds {self.max_seq} rows")
        if sampled and self.sample_state is None:
            self._write_sampling_state()
        # (the warm-up and the recorded step advance positions and tokens -- lookup: the counters and the drafts too --: put back)
        saved = (self.token.clone(), self.pos.clone(), self.lookup_state.clone() if self.lookup else None)
        saved_state = self.sample_state.clone() if sampled else None       # (the warm-up and the capture's own launch-free recording must not consume a draw)
        g = capture_graph(self.dev, lambda: self._step(sampled), lambda: self._restore_step_inputs(saved, saved_state))
        torch.cuda.synchronize(self.dev)
        self._restore_step_inputs(saved)
        if sampled:
            self.sample_state.copy_(saved_state)
            self.sample_graph = g
        else:
            self.graph = g

    def _restore_step_inputs(self, saved, saved_state=None):
        """put back what a step consumed (capture's warm-up): positions, tokens and what derives from them (lookup: the state block and the draft rows
        too; ``saved_state``: the sampling block -- a sampled lookup step advances its draw counter by what it accepted)"""
        self.pos.copy_(saved[1])
        if saved_state is not None:
            self.sample_state.copy_(saved_state)
        if self.lookup:
            self.lookup_state.copy_(saved[2])
            ops.set_token(saved[0], self.embed, self.token, self.pos, self.x, table=self.rope_tab, cur=self.rope_cur)
        else:
            self.set_token(saved[0])

    def decode_step(self, use_graph=True, sampled=None):
        # the step appends cache row host_pos: refuse on the host (the kernels also guard the device-side position:
        # a step past the cache is skipped there and raises the sticky error word, see check())
        if self.host_pos >= self.max_seq:
            raise ValueError(f"decode step at position {self.host_pos} does not fit the KV cache (max_seq={self.max_seq})")
        if sampled is None:
            sampled = self._sampled_tail()
        if self.lookup and self.host_pos + self.lookup >= self.max_seq:
            raise ValueError(f"a verify step at position {self.host_pos} with {self.lookup} drafts does not fit the KV cache (max_seq={self.max_seq})")
        if use_graph and self._graph(sampled) is None:
            self.capture(sampled)
        self.host_pos += self.R if self.lookup else 1       # (lookup: an upper bound -- a step advances by 1 + accepted drafts; lookup_sync() reads the exact value)
        if use_graph:
            self._graph(sampled).replay()
        else:
            self._step(sampled)

    # ---------------------------------------------------------------- prefill
    def _rope(self, t, positions):
        # HF apply_rotary_pos_emb: cos/sin in fp32 -> fp16; rotate_half
        inv = 1.0 / (self.theta ** (torch.arange(0, 128, 2, device=self.dev, dtype=torch.float32) / 128.0)) if self.inv_freq is None \
            else self.inv_freq.to(self.dev, torch.float32)
        fr = positions.to(torch.float32)[:, None] * inv[None, :]
        emb = torch.cat([fr, fr], dim=-1)
        cos, sin = (emb.cos() * self.rope_scale).to(torch.float16)[:, None, :], (emb.sin() * self.rope_scale).to(torch.float16)[:, None, :]
        t1, t2 = t[..., :64], t[..., 64:]
        rot = torch.cat([-t2, t1], dim=-1)
        return t * cos + rot * sin

    def prefill(self, ids, use_graph=True, start_pos=0, lengths=None):
        """ids: int64 [S] prompt.  Fills the KV caches, leaves the next token in self.token and pos = start_pos + S.
        The ~25 framework launches per block make an eager prefill host-bound for short prompts (13 ms at S = 64,
        of which ~1 ms is GPU work); with ``use_graph`` the whole prefill of a given prompt LENGTH is captured once
        into a hipGraph and replayed for later prompts of that length.
        ``start_pos`` > 0 (the reference's patched forward takes the same argument, ftllama_modeling.py:76,98-104): the rows
        are appended behind ``start_pos`` cached positions -- a prompt fed in chunks, or the next turn of a conversation --
        and attend the whole cache; the graph cache is keyed by (length, start_pos).
        ``lengths`` (ragged runners): int [B], 1 <= L_b <= S -- ids [B, S] holds prompt b in its first L_b columns (RIGHT-padded with any valid id).
        Still one pass over B * S rows: under causal attention the pad rows behind a prompt cannot reach its rows, and what they leave in cache
        rows L_b .. S - 1 is overwritten by the decode steps before any step reads it (the step at position p writes row p, then reads 0 .. p).
        Afterwards pos[b] = L_b and the first token comes from row L_b - 1.  The lengths live in a device tensor: the captured pass of (S, 0) serves any."""
        ids = self._ids_rows(ids)
        S = ids.shape[1]
        start_pos = int(start_pos)
        if start_pos < 0 or start_pos + S > self.max_seq:
            raise ValueError("prompt longer than the KV cache")
        if self.lookup and start_pos != 0:
            raise ValueError("lookup: the history holds the whole sequence -- a prompt pass starts at position 0")
        self._kv8_prompt_check(start_pos)
        if self.lookup:
            self._prompt_len = S
        if lengths is not None and not self.ragged:
            raise ValueError("lengths needs a runner built with ragged=True (this one keeps one position for the whole batch)")
        longest = S
        if self.ragged:
            if start_pos != 0:
                raise ValueError("a ragged prompt pass starts at position 0 (chunked ragged prompts are not served)")
            each = _ints(S if lengths is None else lengths, self.B, 1, S, f"lengths: expected {self.B} values in 1..{S}, got {{got}}")
            self.lengths.copy_(torch.tensor(each, dtype=torch.int64))
            longest = max(each)
        if use_graph:
            ent = self._prefill_graphs.get((S, start_pos))
            if ent is None:
                static_ids = ids.to(self.dev).clone()
                g = capture_graph(self.dev, lambda: self._prefill_rows(static_ids, start_pos))
                ent = self._prefill_graphs[(S, start_pos)] = (g, static_ids, self.logits_rows if self.all_logits else None)
            g, static_ids, rows = ent
            static_ids.copy_(ids)
            g.replay()
            if rows is not None:
                self.logits_rows = rows         # (this graph's own output buffer: valid until its next replay)
        else:
            self._prefill_rows(ids, start_pos)
        self.host_pos = start_pos + longest     # (a replay sets the device-side position; the host mirror is not part of it)
        if self._sampled_tail():
            self._first_token()                 # (outside the prompt graph, which ends in the arg-max: one graph per prompt length serves both)
        return self.logits

    # ------------------------------------------------- prompt-lookup speculative decoding
    def _lookup_first_token(self, S, sampled):
        """the first token of a lookup run, with the prompt's S tokens in the history: the lookup block is armed -- S tokens, no steps, no drafts, row
        j at position S - 1 + j -- and the verify-and-propose tail runs on the last prompt row's logits as row 0 of a step without drafts: it
        emits the first token, proposes the first drafts and leaves the step inputs of position S.  ``sampled``: outside the prompt graph (which
        ends in the greedy tail: one graph per length serves both), the sampled tail -- it draws with counter 0 and leaves the counter at 1."""
        st = self.lookup_state
        st[ops.LOOKUP_COUNT:ops.LOOKUP_TICKET + 1].zero_()                      # count, steps, accepted, ticket
        st[ops.LOOKUP_COUNT].fill_(S)
        st[ops.LOOKUP_DRAFT:ops.LOOKUP_DRAFT + 8].fill_(-1)
        self.set_pos(S - 1)
        self._tail(sampled)
        st[ops.LOOKUP_STEPS].zero_()                                            # (the prompt pass is not a verify step)
        self.host_pos = S

    def _lookup_set_token(self, token):
        """row 0 = ``token``, no drafts (-1: rows 1 .. D run a placeholder and are never accepted); the counters are left alone"""
        if isinstance(token, torch.Tensor):
            self._tok_in.zero_()
            self._tok_in[:1].copy_(token.reshape(-1)[:1])
        else:
            self._tok_in.zero_()
            self._tok_in[0] = int(token)
        self.lookup_state[ops.LOOKUP_DRAFT:ops.LOOKUP_DRAFT + 8].fill_(-1)
        ops.set_token(self._tok_in, self.embed, self.token, self.pos, self.x, table=self.rope_tab, cur=self.rope_cur)

    def set_lookup_mode(self, external):
        """who proposes the drafts: False = the tail looks them up in the history; True = the caller (``verify_step``) -- the tail then leaves -1 drafts.
        One word of the device block: nothing is re-captured."""
        self.lookup_state[ops.LOOKUP_MODE].fill_(1 if external else 0)

    def set_ngram_max(self, ngram_max):
        """the longest suffix the tail looks up (1 .. 4): one word of the device block, read on every launch -- nothing is re-captured"""
        if not self.lookup:
            raise ValueError("set_ngram_max needs a runner built with lookup=D")
        if not 1 <= int(ngram_max) <= 4:
            raise ValueError(f"ngram_max must be 1..4, got {ngram_max}")
        if int(ngram_max) != self.ngram_max:
            self.ngram_max = int(ngram_max)
            self.lookup_state[ops.LOOKUP_NGRAM].fill_(self.ngram_max)

    def verify_step(self, drafts, use_graph=True):
        """one verify step with the caller's drafts: a tensor (or list) of D token ids for rows 1 .. D, -1 = none.  The runner must be in external mode
        (``set_lookup_mode(True)``) before the step that precedes this one, or the tail's own proposals are overwritten here all the same."""
        if not self.lookup:
            raise ValueError("verify_step needs a runner built with lookup=D")
        d = torch.as_tensor(drafts, dtype=torch.int64).reshape(-1).to(self.dev)
        if d.numel() != self.lookup:
            raise ValueError(f"expected {self.lookup} draft ids (-1 = none), got {d.numel()}")
        self._tok_in[:1].copy_(self.token[:1])
        self._tok_in[1:].copy_(d.clamp(0, self.vocab - 1))
        ops.set_token(self._tok_in, self.embed, self.token, self.pos, self.x, table=self.rope_tab, cur=self.rope_cur)
        self.lookup_state[ops.LOOKUP_DRAFT + 1:ops.LOOKUP_DRAFT + 1 + self.lookup].copy_(d.to(torch.int32))     # unclamped: what the comparison sees
        self.decode_step(use_graph)

    def lookup_sync(self):
        """(tokens in the history, steps taken) read from the device block (synchronises); makes the host's position mirror exact again"""
        c = self.lookup_state[ops.LOOKUP_COUNT:ops.LOOKUP_STEPS + 1].tolist()
        self.host_pos = max(0, c[0] - 1)
        return c[0], c[1]

    def lookup_stats(self):
        """dict(steps, tokens, mean_accepted): verify steps since the last prompt pass, tokens they emitted, accepted drafts per step"""
        count, steps = self.lookup_sync()
        tokens = count - self._prompt_len - 1 if steps else 0
        return dict(steps=steps, tokens=tokens, mean_accepted=(tokens / steps - 1.0) if steps else 0.0)

    def lookup_tokens(self):
        """everything emitted since the last prompt pass (its first token included), int64 device tensor"""
        count, _ = self.lookup_sync()
        return self.history[self._prompt_len:count].to(torch.int64)

    def _lookup_generate(self, ids, gen_len, use_graph, stop_at_eos, min_new_tokens):
        S, D = ids.shape[-1], self.lookup
        if S + gen_len + D > self.max_seq:
            raise ValueError(f"prompt ({S}) + {gen_len} tokens + {D} draft rows do not fit the KV cache (max_seq={self.max_seq})")
        if self.sampling is not None and not self.lookup_sampling:
            raise ValueError("lookup: speculative decoding here is greedy; call set_sampling(None)")
        if self.sampling is not None:
            self._write_sampling_state()        # draw counter 0: one seed fixes the whole sequence
        eos = tuple(self.eos) if stop_at_eos else ()
        with _held_back(self, eos, bool(eos) and min_new_tokens > 0) as hold:
            self.set_lookup_mode(False)
            self.prefill(ids, use_graph=use_graph)
            count, emitted = S + 1, 1
            while emitted < gen_len:
                if emitted >= min_new_tokens:
                    hold.release()
                if hold.held and min_new_tokens - emitted < self.R:
                    # the EOS ids are held back for exactly the first min_new_tokens tokens: a step that could cross that line runs without drafts
                    # (one token)
                    self._lookup_set_token(self.token[:1])
                    self.decode_step(use_graph)
                else:
                    # a burst: at most what is still wanted (a step emits at least one token), while the EOS ids are held back only steps that stay
                    # inside the first min_new_tokens however much is accepted, and never so far that the rows of a fully accepted step would
                    # leave the cache
                    k = min(self.EOS_POLL_STEPS, gen_len - emitted, max(1, (self.max_seq - D - self.host_pos) // self.R))
                    if hold.held:
                        k = min(k, (min_new_tokens - emitted) // self.R)
                    for _ in range(k):
                        self.decode_step(use_graph)
                count, _ = self.lookup_sync()
                emitted = count - S
                if eos and self._first_eos(self.history[S:count], min_new_tokens) is not None:
                    break
            out = self.history[S:min(count, S + gen_len)].to(torch.int64)
            if eos:
                cut = self._first_eos(out, min_new_tokens)
                if cut is not None:
                    out = out[:cut + 1]
            return out

    def _first_eos(self, toks, skip=0):
        """index of the first EOS id in ``toks`` at or behind index ``skip`` (None: none)"""
        if not self.eos or toks.numel() <= skip:
            return None
        hit = torch.isin(toks[skip:], torch.tensor(self.eos, dtype=toks.dtype, device=toks.device)).nonzero()
        return None if hit.numel() == 0 else int(hit[0].item()) + skip

    def _ids_rows(self, ids):
        """prompt ids as [batch, S] on the device (a 1-D prompt is the batch-1 form)"""
        ids = ids.to(self.dev)
        if ids.dim() == 1:
            ids = ids[None, :]
        if ids.dim() != 2 or ids.shape[0] != self.B:
            raise ValueError(f"expected {self.B} prompt(s) of equal length, got ids of shape {tuple(ids.shape)}")
        return ids

    def _kv8_prompt_check(self, start_pos):
        """an 8-bit cache is written by the prompt pass and read by the token step only: a prompt pass behind cached rows would have to attend them"""
        if self.kv_bits == 8 and start_pos != 0:
            raise ValueError("kv_bits=8: a prompt pass starts at position 0 (the prompt kernels read no 8-bit cache: chunked prompts are not served)")

    def _rows_kv(self, blk, q, k, v, S, start_pos, cache):
        """the rotation and the cache write of a prompt pass -> (k, v, kv_cache) as ops.attn_prefill is to read them.  fp16 cache: one launch
        rotates q / k and writes rows start_pos .. of the cache, which the attention reads.  No cache: q / k are rotated in place and the attention
        reads the projection outputs.  8-bit cache (position 0): the same -- exact fp16, the prompt's own attention is the no-cache pass bit for
        bit -- and ONE ops.kv8_store quantizes the rows into the cache."""
        if cache and self.kv_bits == 16:
            ops.rope_cache(q, k, v, blk["kc"], blk["vc"], self.rope_tab, start_pos, self.nh, self.nkv, **self._qkn(blk))
            return blk["kc"], blk["vc"], True
        ops.rope_rows(q, k, self.rope_tab, S, self.nh, self.nkv, **self._qkn(blk))
        if cache:
            ops.kv8_store(k, v, blk["kc8"], blk["ks"], blk["vc8"], blk["vs"], 0, self.nkv)
        return k, v, False

    def _prefill_rows(self, ids, start_pos):
        """the prompt pass of every sequence (each into its own slice of the caches), then position(s) and first token(s); all device work: what
        the prompt graph captures"""
        B, S = ids.shape
        return self._prompt_finish(self._rows_pass(ids, start_pos, cache=True), B, S, start_pos, self.lengths, prompt_ids=ids)

    def _prompt_finish(self, x, B, S, start_pos=0, lengths=None, prompt_ids=None):
        """the end of a prompt pass over B prompts of S rows, x [B * S, H] its final hidden rows: the logits of every sequence's last row (all_logits:
        of every row, in self.logits_rows), the position, the first token.  ``lengths`` (a ragged runner's, device int64 [B]): sequence b ends in
        row lengths[b] - 1 and goes on at position lengths[b].  ``prompt_ids``: what a lookup runner copies into its history."""
        out = self.logits.view(self.R, self.vocab)[:B]      # (lookup: row 0 of the step's R rows)
        each = None if lengths is None else torch.arange(B, device=x.device)
        if self.all_logits:
            self.logits_rows = self._logits_of_rows(x, B, S, out)
            if lengths is not None:
                out.copy_(self.logits_rows[each, lengths - 1])
        else:
            last = (x.view(B, S, self.H)[:, S - 1] if lengths is None else x.view(B, S, self.H)[each, lengths - 1]).contiguous()
            self._lm_logits(last[0] if B == 1 else last, out[0] if B == 1 else out)
        if self.lookup:
            # the prompt goes into the history with a device copy, and the verify-and-propose tail itself -- run on the last prompt row's logits as
            # row 0 of a step at position S - 1 without drafts -- emits the first token, proposes the first drafts and leaves the step inputs of
            # position S
            self.history[:S].copy_(prompt_ids.reshape(-1))
            self._lookup_first_token(S, sampled=False)
        elif lengths is not None:
            self.pos.copy_(lengths)             # (the host mirror: prefill())
            self.set_token(self._argmax(out))
        else:
            self.set_pos(start_pos + S)
            self.set_token(self._argmax(out))
        return self.logits

    def _rows_pass(self, ids, start_pos, cache):
        """ONE many-row pass over B prompts of S rows (ids [B, S]): the linears see all B * S rows at once (one pass over
        the weights), RoPE and the causal attention run as ONE launch each over all sequences.  ``cache``: the rotated keys /
        values are written into the runner's KV caches (rows start_pos .. start_pos + S - 1 of every sequence) and the
        attention reads them there (a batched decode runner's prompt); otherwise q / k are rotated in place and the
        attention reads the projection outputs (the harness' GeMM mode, no cache).  Returns the final hidden rows [B * S, H].
        The ONE walk over the blocks of a prompt pass, for every runner; which kernels it takes: _rows_route."""
        B, S = ids.shape
        nh, nkv = self.nh, self.nkv
        if cache:
            self._kv8_prompt_check(start_pos)
        route = self._rows_route(B, S, cache)
        frag = route == "frag"
        lin, up_gated = (self._few_linear, self._few_up_gated) if route == "few" else (self._rows_linear, self._rows_up_gated)
        x = self.embed.index_select(0, ids.reshape(-1).to(self.dev))        # the residual stream, updated in place
        h = None                                # frag: the normed input of this block, where the block in front left it behind
        for bi, blk in enumerate(self.blocks):
            if frag:
                if h is None:
                    h = ops.rmsnorm_xfrag(x, blk["ln1"], self.eps)
                q, k, v = self._frag_group([blk["self_attn.q_proj"], blk["self_attn.k_proj"], blk["self_attn.v_proj"]], h, S)     # one launch
            else:
                h = ops.rmsnorm(x, blk["ln1"], self.eps)
                q, k, v = lin(blk["self_attn.q_proj"], h), lin(blk["self_attn.k_proj"], h), lin(blk["self_attn.v_proj"], h)
            kk, vv, cached = self._rows_kv(blk, q, k, v, S, start_pos, cache)
            a = ops.attn_prefill(q, kk, vv, None if frag else torch.empty_like(q), S, nh, nkv, batch=B, pos0=start_pos if cached else 0,
                                 kv_cache=cached, out_xfrag=frag)
            if not frag:
                x = lin(blk["self_attn.o_proj"], a, residual=x)
                h2 = ops.rmsnorm(x, blk["ln2"], self.eps)
                act = up_gated(blk["mlp.up_proj"], h2, lin(blk["mlp.gate_proj"], h2))
                x = lin(blk["mlp.down_proj"], act, residual=x)
                continue
            # the projections that read a normed / attention activation take it in fragment order (written that way by the producing launch):
            # 1.2-1.6x faster few-row GEMMs; down_proj (K = 11008: the per-workgroup x stream is what bounds that kernel) stays on
            # the tiled kernel, whose split-K reduce also writes the next block's normed input (FUSE_DOWN_NORM)
            l = blk["self_attn.o_proj"]
            x = ops.gemm_xfrag(a, S, l.qn, l.mn, l.bits, l.mode, l.N, l.K, bias=l.bias, residual=x, out=x)
            g, u = self._frag_group([blk["mlp.gate_proj"], blk["mlp.up_proj"]], ops.rmsnorm_xfrag(x, blk["ln2"], self.eps), S)    # one launch
            act, l, h = ops.silu_mul(g, u, out=g), blk["mlp.down_proj"], None
            if self.FUSE_DOWN_NORM and bi + 1 < len(self.blocks):
                x, h = ops.gemm_res_norm_xfrag(act, l.qn, l.mn, l.bits, l.mode, l.N, l.K, self.blocks[bi + 1]["ln1"], self.eps,
                                               bias=l.bias, residual=x, out=x)
            else:
                x = lin(l, act, residual=x)
        return x

    def _frag_group(self, ls, xf, S):
        """the linears ``ls`` over the same S rows in fragment order ``xf``, as one launch -> their outputs [S, N] each"""
        ys = [torch.empty(S, l.N, dtype=torch.float16, device=self.dev) for l in ls]
        ops.gemm_xfrag_grouped(xf, S, [l.seg(y) for l, y in zip(ls, ys)], ls[0].K)
        return ys

    def _logits_of_rows(self, x, B, S, last_logits):
        """logits of every prompt row, [B, S, vocab] fp16: final RMSNorm + ONE pass over the lm_head for all rows (fp16 MFMA GEMM); each sequence's
        last row is copied into ``last_logits`` (the runner's token choice), instead of a second pass over the lm_head for it"""
        rows = self._lm_logits_many(x).view(B, S, self.vocab)
        last_logits.view(B, self.vocab).copy_(rows[:, S - 1])
        return rows

    def _lm_head_streamed(self, x, out):
        """out [n, vocab] = lm_head(final RMSNorm(x [n, H])) through the weight-streaming kernel, 8 rows a launch (any vocabulary)"""
        n = x.shape[0]
        for r0 in range(0, n, 8):
            r1 = min(n, r0 + 8)
            if r1 - r0 == 1:
                self._lm_logits(x[r0], out[r0])
            else:
                self._lm_logits(x[r0:r1], out[r0:r1])
        return out

    # rows of logits formed at a time by score_rows: the fp16 scratch is [SCORE_ROWS, vocab] (156 MB at 512 x 152064, against the 1.87 GB of a
    # 2048-token window's fp16 + fp32 logits)
    SCORE_ROWS = 512

    @staticmethod
    def score_chunks(S, rows):
        """the scored rows 0 .. S - 2 of a window of S tokens (its last row has no label) as [(first, end)] pieces of at most ``rows`` rows"""
        if S < 2 or rows < 1:
            raise ValueError(f"a scored window needs at least 2 tokens and a chunk at least 1 row (got S={S}, rows={rows})")
        return [(t0, min(S - 1, t0 + rows)) for t0 in range(0, S - 1, rows)]

    def score_rows(self, ids, dense_logits=None):
        """The evaluation metrics of this model on token windows ``ids`` [B, S] (or [S]): per-row negative log-likelihood, row t scored against
        ids[:, t + 1] -> float32 [B, S - 1] on the device; with ``dense_logits`` ([B, S, vocab] or [S, vocab], fp16 or fp32, device or host: the
        dense model's logits on the same windows) also the per-row Jensen-Shannon divergence (ops.logit_jsd: the reference's JSD) -> (nll, jsd).

        One prompt pass over all B * S rows without a KV cache (any B; S <= max_seq, the RoPE table): caches, positions and tokens of the runner
        are untouched.  The logits of a window never exist: the final hidden rows are walked in pieces of SCORE_ROWS rows -- final RMSNorm, lm_head
        into one reused fp16 scratch, one metric launch (two with JSD) on it; host-side dense logits are moved a piece at a time.  Nothing
        synchronises."""
        ids = ids.to(self.dev)
        if ids.dim() == 1:
            ids = ids[None, :]
        if ids.dim() != 2 or ids.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"expected integer ids [B, S] or [S], got {ids.dtype} of shape {tuple(ids.shape)}")
        B, S = ids.shape
        if B < 1 or S < 2:
            raise ValueError(f"a scored window needs at least 2 tokens (got ids of shape {tuple(ids.shape)})")
        if S > self.max_seq:
            raise ValueError(f"window of {S} tokens longer than the RoPE table (max_seq={self.max_seq})")
        if dense_logits is not None:
            if dense_logits.dim() == 2:
                dense_logits = dense_logits[None]
            if tuple(dense_logits.shape) != (B, S, self.vocab) or dense_logits.dtype not in (torch.float16, torch.float32):
                raise ValueError(f"dense_logits: expected fp16 / fp32 [{B}, {S}, {self.vocab}], got {dense_logits.dtype} {tuple(dense_logits.shape)}")
            if dense_logits.stride(2) != 1 or dense_logits.stride(1) < self.vocab:
                dense_logits = dense_logits.contiguous()
        R = int(self.SCORE_ROWS)
        chunks = self.score_chunks(S, R)
        x = self._rows_pass(ids, 0, cache=False).view(B, S, self.H)
        labels = ids[:, 1:].to(torch.int64).contiguous()
        buf = getattr(self, "_score_buf", None)
        if buf is None or buf[0].shape[0] != R:
            dev = self.dev
            buf = self._score_buf = (torch.empty(R, self.vocab, dtype=torch.float16, device=dev), torch.empty(R, dtype=torch.float32, device=dev),
                                     torch.empty(R, dtype=torch.int32, device=dev))
        scratch, lse, amax = buf
        nll = torch.empty(B, S - 1, dtype=torch.float32, device=self.dev)
        jsd = None if dense_logits is None else torch.empty(B, S - 1, dtype=torch.float32, device=self.dev)
        for b in range(B):
            for t0, t1 in chunks:
                n = t1 - t0
                rows, lg = x[b, t0:t1], scratch[:n]
                self._lm_logits_many(rows, lg)
                ops.logit_nll(lg, labels[b, t0:t1], out=(nll[b, t0:t1], lse[:n], amax[:n]))
                if jsd is not None:
                    ops.logit_jsd(lg, dense_logits[b, t0:t1].to(self.dev, non_blocking=True), out=jsd[b, t0:t1])
        return nll if jsd is None else (nll, jsd)

    # prompt rows (exclusive, inclusive) served by the fragment-ordered few-row kernels with q/k/v and gate/up as grouped
    # launches.  7B avg-3, ms per prompt pass, this path | the row-major / tiled kernels: 16 rows 2.91 | 2.55, 24 3.03 | 3.13,
    # 32 3.06 | 3.28, 64 3.19 | 3.72, 256 6.74 | 7.32, 384 10.86 | 11.30, 512 12.58 | 11.26
    FRAG_ROWS = (16, 384)
    FUSE_DOWN_NORM = True       # down_proj's split-K reduce also writes the next block's normed input (A/B: tools/prompt64_time.py)

    def _rows_route(self, B, S, cache):
        """which kernels the walk of a prompt pass takes (_rows_pass).  Only the one prompt of a batch-1 runner into its cache
        leaves the tiled kernels:
          "frag"   FRAG_ROWS[0] < S <= FRAG_ROWS[1], groups of 128, no OWQ layer: the fragment-ordered few-row kernels -- rmsnorm_xfrag, q/k/v and
                   gate/up as grouped launches, attention and o_proj handing over in fragment order, down_proj's reduce carrying the next norm;
          "few"    S <= 8: ops.linear (the GEMV) per linear, residual and SiLU*mul as launches of their own (_few_linear / _few_up_gated);
          "tiled"  everything else -- any batch, ragged runners, passes without a cache (score_rows, prefill_batch) at ANY row count: the tiled
                   MFMA GEMM with residual / SiLU*mul epilogues (_rows_linear / _rows_up_gated)."""
        if B != 1 or not cache or self.ragged:
            return "tiled"
        if self.FRAG_ROWS[0] < S <= self.FRAG_ROWS[1] and not self.fine and not self.owq:     # (an OWQ model: the plain, unfused form)
            return "frag"
        return "few" if S <= 8 else "tiled"

    def _few_linear(self, l, inp, residual=None):
        # _rows_linear for up to 8 rows of one prompt
        if l.owq:
            return self._rows_owq(l, inp, residual)
        y = ops.linear(inp, l.qn, l.mn, l.bits, l.mode, l.N, l.K, bias=l.bias)
        return y if residual is None else residual.add_(y)

    def _few_up_gated(self, l, inp, gate):
        return ops.silu_mul(gate, self._few_linear(l, inp), out=gate)

    def _rows_linear(self, l, inp, residual=None):
        # y = inp . W^T (+ residual, in place) for many rows
        if l.owq:
            return self._rows_owq(l, inp, residual)
        return ops.gemm(inp, l.qn, l.mn, l.bits, l.mode, l.N, l.K, bias=l.bias, residual=residual, out=residual)

    def _rows_up_gated(self, l, inp, gate):
        # silu(gate) * (inp . W^T), in place on gate: the LlamaMLP product formed in up_proj's epilogue
        if l.owq:                               # (the outlier columns come after the packed product: no gate epilogue; plain, then silu_mul)
            return ops.silu_mul(gate, self._rows_owq(l, inp), out=gate)
        return ops.gemm(inp, l.qn, l.mn, l.bits, l.mode, l.N, l.K, bias=l.bias, gate=gate, out=gate)

    @staticmethod
    def _rows_owq(l, inp, residual=None):
        """an OWQ linear over any number of rows, HIPOWQLinear.forward's three steps: gather, the packed matmul over the gathered rows (the
        residual in its epilogue, in place, where the caller passes one), outlier add"""
        y = ops.gemm(ops.owq_gather(inp, l.perm), l.qn, l.mn, l.bits, l.mode, l.N, l.Kp, bias=l.bias, residual=residual, out=residual)
        return ops.owq_outlier_add(inp, l.out_ids, l.W_out, y)

    def prefill_batch(self, ids):
        """ids: int64 [B, S].  The many-row pass over B prompts at once (B*S rows through every linear): what the reference
        harness times in GeMM mode with batch_size > 1 (amq/utils/speed.py:61-71; BASELINE.json configs[3] = 16 x 2048 on
        13B).  Returns the last-token logits [B, vocab].  The runner's KV cache is batch-1 (like the reference's FT path),
        so this pass does not write it and cannot be followed by decode steps."""
        if self.ragged:
            raise ValueError("prefill_batch writes no cache and keeps no positions: not offered with ragged=True")
        B, S = ids.shape
        if S > self.max_seq:
            raise ValueError("prompt longer than the RoPE table")
        last = self._rows_pass(ids, 0, cache=False).view(B, S, self.H)[:, S - 1].contiguous()
        return self._lm_head_streamed(last, torch.empty(B, self.vocab, dtype=torch.float16, device=self.dev))   # the lm_head once per 8 sequences

    def _prefill_attention_sdpa(self, q, blk, S):
        """causal attention of a batch-1 prompt at position 0 through the framework's SDPA: q [S, nh*128] rotated, K / V = cache rows 0 .. S - 1 ->
        [S, nh*128] (comparison point for tests / tools; not on the product path)"""
        nh, nkv = self.nh, self.nkv
        qh = q.view(S, nh, 128).transpose(0, 1)
        kh, vh = blk["kc"][0, :, :S], blk["vc"][0, :, :S]
        if nkv != nh:
            kh = kh.repeat_interleave(nh // nkv, dim=0)
            vh = vh.repeat_interleave(nh // nkv, dim=0)
        a = torch.nn.functional.scaled_dot_product_attention(qh[None], kh[None], vh[None], is_causal=True)[0]
        return a.transpose(0, 1).reshape(S, self.qd).contiguous()

    def _prefill_unfused(self, ids):
        """The same pass with framework ops for everything but the linears and RMSNorm (HF-style RoPE in fp32 -> fp16,
        separate cache copies, residual adds, SiLU and product): kept as the comparison point of the fused pass
        (tests/test_gpu_decode.py)."""
        S = ids.numel()
        if S > self.max_seq:
            raise ValueError("prompt longer than the KV cache")
        if self.qk_norm:
            raise ValueError("the framework-op comparison pass has no per-head q / k norm: not offered for a qk_norm model")
        if self.kv_bits == 8:
            raise ValueError("kv_bits=8: the framework-op comparison pass (SDPA over the fp16 cache) is not offered")
        H, nh, nkv = self.H, self.nh, self.nkv
        ids = ids.to(self.dev)
        x = self.embed.index_select(0, ids)
        positions = torch.arange(S, device=self.dev)

        def lin(l, inp):
            if l.owq:
                return self._rows_owq(l, inp)
            return ops.linear(inp, l.qn, l.mn, l.bits, l.mode, l.N, l.K, bias=l.bias)

        for blk in self.blocks:
            h = ops.rmsnorm(x, blk["ln1"], self.eps)
            q = lin(blk["self_attn.q_proj"], h).view(S, nh, 128)
            k = lin(blk["self_attn.k_proj"], h).view(S, nkv, 128)
            v = lin(blk["self_attn.v_proj"], h).view(S, nkv, 128)
            q, k = self._rope(q, positions), self._rope(k, positions)
            blk["kc"][0, :, :S] = k.transpose(0, 1)
            blk["vc"][0, :, :S] = v.transpose(0, 1)
            x = x + lin(blk["self_attn.o_proj"], self._prefill_attention_sdpa(q.reshape(S, nh * 128).contiguous(), blk, S))
            h2 = ops.rmsnorm(x, blk["ln2"], self.eps)
            g, u = lin(blk["mlp.gate_proj"], h2), lin(blk["mlp.up_proj"], h2)
            x = x + lin(blk["mlp.down_proj"], torch.nn.functional.silu(g) * u)
        return self._prompt_finish(x, 1, S, prompt_ids=ids)

    def reset(self):
        self.set_pos(0)
        self.set_token(0)
        if self.lookup:                         # an empty history; the counters start over
            self.lookup_state[ops.LOOKUP_COUNT:ops.LOOKUP_TICKET + 1].zero_()
            self._prompt_len = 0

    def generate(self, ids, gen_len, use_graph=True, stop_at_eos=False, min_new_tokens=0, lengths=None):
        """prefill + gen_len tokens (min_new_tokens = max_new_tokens = gen_len, amq/utils/speed.py:34-39): greedy, or sampled after
        ``set_sampling``.  Returns the generated ids (device tensor).  ``stop_at_eos`` (ids from ``set_eos``): a sequence that emits an EOS id is
        padded with the pad id from there on, and the loop ends once every sequence has (polled every EOS_POLL_STEPS steps): returns [B, n] with
        n = the longest sequence's length, as HF does; the EOS ids stay suppressed for the first ``min_new_tokens`` tokens.
        ``lengths`` (ragged runners): see :meth:`prefill`; the longest prompt + gen_len must fit the cache."""
        if self.lookup:
            return self._lookup_generate(ids, gen_len, use_graph, stop_at_eos, min_new_tokens)
        S = ids.shape[-1]
        if lengths is not None:
            if not self.ragged:
                raise ValueError("lengths needs a runner built with ragged=True (this one keeps one position for the whole batch)")
            lengths = _ints(lengths, self.B, 1, S, f"lengths: expected {self.B} values in 1..{S}, got {{got}}")
            S = max(lengths)
        if S + gen_len > self.max_seq:
            raise ValueError("sequence does not fit the KV cache")
        if not stop_at_eos and self.sampling is None:   # greedy, fixed length
            out = torch.empty(self.B, gen_len, dtype=torch.int64, device=self.dev)
            self.prefill(ids, lengths=lengths)
            out[:, 0] = self.token
            for i in range(1, gen_len):
                self.decode_step(use_graph)
                out[:, i] = self.token
            if self.engine is not None:
                self.check()                    # a barrier time-out of the one-launch-per-token engine must not pass as tokens
            return out[0] if self.B == 1 else out
        self._greedy_eos = self.sampling is None
        try:
            with _held_back(self, self.eos, stop_at_eos and min_new_tokens > 0) as hold:
                self._write_sampling_state()    # draw counter 0, nobody finished: one seed fixes the whole sequence
                if not stop_at_eos:
                    self.sample_state[8:16].fill_(-1)       # fixed length: no EOS bookkeeping
                out = torch.full((self.B, gen_len), self.pad_id, dtype=torch.int64, device=self.dev)
                self.prefill(ids, lengths=lengths)      # (draws the first token: draw 0)
                out[:, 0] = self.token
                for i in range(1, gen_len):
                    if i == min_new_tokens:
                        hold.release()
                    if stop_at_eos and i % self.EOS_POLL_STEPS == 0 and self.unfinished() == 0:
                        break
                    self.decode_step(use_graph, sampled=True)
                    out[:, i] = self.token
                if self.engine is not None:
                    self.check()
                if stop_at_eos:
                    out = self._trim_after_eos(out)
        finally:
            self._greedy_eos = False
        return out[0] if self.B == 1 else out

    def _trim_after_eos(self, out):
        """cut the columns behind the last sequence's EOS (they hold the pad id only)"""
        if not self.eos or out.shape[1] == 0:
            return out
        hit = torch.isin(out, torch.tensor(self.eos, dtype=out.dtype, device=out.device))
        cols = torch.arange(1, out.shape[1] + 1, device=out.device)
        length = torch.where(hit.any(dim=1), (hit.int().argmax(dim=1) + 1), cols[-1]).max()
        return out[:, :int(length.item())]


class DenseLlama(QuantLlama):
    """fp16 baseline with the same runner interface (the reference's ``result['fp16']`` row,
    amq_speed_benchmark.py:171-197): plain library GEMMs (torch / hipBLASLt) for the seven
    linears, the same RMSNorm / attention / lm_head kernels around them."""

    def __init__(self, config, device="cuda:0", max_seq=256, seed=0, batch=1, ragged=False, lookup=0):
        if lookup:
            raise ValueError("the fp16 baseline runs one row per sequence: lookup= is served by QuantLlama")
        if ragged:
            raise ValueError("the fp16 baseline keeps one position for the whole batch: ragged=True is served by QuantLlama")
        config = MODEL_CONFIGS[config] if isinstance(config, str) else config
        # (one position for the whole batch, one row per sequence and step; fp16 cache and lm_head)
        self._frame(config, device, max_seq, runner_options(batch, ngram_max=0))
        gen = torch.Generator(device=self.dev).manual_seed(seed)
        lin = lambda n, k: (torch.randn(n, k, device=self.dev, generator=gen) * (0.5 / math.sqrt(k))).to(torch.float16)
        self.blocks = [{**{name: lin(*config["linear_shape"][name]) for name in config["linear"]}, **self._block_norms(b, gen), **self._alloc_cache()}
                       for b in range(self.nb)]
        self._dense_tensors(gen)
        self._alloc_step_buffers()
        self._init_step_state((None, 1.0))      # (plain rope_theta frequencies)

    def linear_bytes_per_token(self):
        return sum(blk[name].numel() * 2 for blk in self.blocks for name in self.cfg["linear"])

    def set_sampling(self, *args, **kwargs):
        raise NotImplementedError("sampled decoding is served by QuantLlama; the fp16 baseline decodes greedily")

    def _step(self, sampled=False):
        if sampled:
            raise NotImplementedError("sampled decoding is served by QuantLlama; the fp16 baseline decodes greedily")
        F = torch.nn.functional
        x = self.x
        for blk in self.blocks:
            h = ops.rmsnorm(x, blk["ln1"], self.eps)
            q = F.linear(h, blk["self_attn.q_proj"])
            k = F.linear(h, blk["self_attn.k_proj"])
            v = F.linear(h, blk["self_attn.v_proj"])
            ops.attn_decode(q, k, v, blk["kc"], blk["vc"], self.att, self.pos, self.nh, self.nkv, self.theta, cur=self.rope_cur, **self._qkn(blk))
            x = x + F.linear(self.att, blk["self_attn.o_proj"])
            h2 = ops.rmsnorm(x, blk["ln2"], self.eps)
            x = x + F.linear(F.silu(F.linear(h2, blk["mlp.gate_proj"])) * F.linear(h2, blk["mlp.up_proj"]),
                             blk["mlp.down_proj"])
        ops.gemv_f16w(x.reshape(-1).contiguous() if self.B == 1 else x.contiguous(), self.lm_head, gamma=self.norm, eps=self.eps,
                      out=self.logits)
        ops.decode_tail(self.logits, self.embed, self.token, self.pos, self.x, table=self.rope_tab, cur=self.rope_cur, suppress=self.suppress)

    def _rows_linear(self, w, inp, residual=None):
        if residual is None:
            return torch.nn.functional.linear(inp, w)
        return torch.addmm(residual, inp, w.t(), out=residual)

    def _rows_up_gated(self, w, inp, gate):
        return ops.silu_mul(gate, torch.nn.functional.linear(inp, w), out=gate)

    def _rows_route(self, B, S, cache):
        return "tiled"                          # (library GEMMs at every row count: the two methods above)


def get_memory_footprint(model, return_buffers=True):
    """bytes of weights + buffers (amq_speed_benchmark.py:88-95 counts parameters and buffers); takes a runner or, as the reference
    does, a ``torch.nn.Module`` (e.g. the swapped HF model: HIPQuantLinear keeps its weights in buffers)"""
    if isinstance(model, torch.nn.Module):
        mem = sum(p.nelement() * p.element_size() for p in model.parameters())
        return mem + (sum(b.nelement() * b.element_size() for b in model.buffers()) if return_buffers else 0)
    tot = model.embed.numel() * 2 + model.lm_head_bytes() + model.norm.numel() * 2
    for blk in model.blocks:
        for k, v in blk.items():
            if isinstance(v, torch.Tensor):
                tot += v.numel() * v.element_size()
            elif hasattr(v, "nbytes"):
                tot += v.nbytes()
    return tot
