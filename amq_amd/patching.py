"""prepare_for_inference / patch_linearlayers -- the reference's plug-in API
(hqq/utils/patching.py:39-49, 143-223) for the HIP backend.

    prepare_for_inference(model, backend="hip", load_path=None)

walks ``named_children`` and replaces every HQQLinear by a HIPQuantLinear, with
the reference's cache-file behaviour (patching.py:178-208): if ``load_path`` is
given and missing, the patched ``model.state_dict()`` is saved there; if it
exists, empty modules are created and the state dict is loaded instead of
re-packing.  ``backend="gptq"`` and ``backend="ft"`` are accepted as aliases so
that ``amq_speed_benchmark.py:137-139`` runs unchanged: both produce
HIPQuantLinear modules (one class serves 2/3/4 bit).

Reference caches written by the CUDA build (``*_GPTQLinear.pt`` / ``*_FTLinear.pt``,
keys ``<module>.qweight|scales|zeros`` and ``<module>.qweight|scales|scaled_zeros``)
are imported with ``load_reference_cache``.
"""
import contextlib
import os

import torch

from . import ops
from .hqq_format import HQQWeights, from_hqq_layer
from .quant_linear import HIPLlamaMLP, HIPOWQLinear, HIPQuantLinear, HIPRMSNorm, LinearGroup

# sibling linears of one parent module that read the same input (HF LlamaAttention / LlamaMLP attribute names)
SIBLING_GROUPS = (("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj"))

HIP_BACKENDS = ("hip", "gptq", "ft")


def is_hqq_layer(layer):
    """HQQLinear / HQQLinearLoRA of the reference (quantize.py:387, peft.py) by
    duck typing -- this package never imports the reference."""
    if isinstance(layer, HQQWeightsModule):
        return True
    cls = type(layer).__name__
    if cls == "HQQLinear":
        return hasattr(layer, "W_q") and hasattr(layer, "meta")
    if cls == "HQQLinearLoRA":
        return hasattr(layer, "linear_layer")
    return False


class HQQWeightsModule(torch.nn.Module):
    """Minimal stand-in for HQQLinear holding an HQQWeights (used by the
    synthetic-model builders and tests; real HQQLinear objects work as well)."""

    def __init__(self, weights: HQQWeights):
        super().__init__()
        self.weights = weights
        self.W_q = weights.W_q
        self.meta = weights.meta
        self.bias = weights.bias
        self.name = weights.name
        self.device = weights.W_q.device


def patch_linearlayers(model, fct, patch_params=None, verbose=False):
    """The reference's walk (patching.py:39-49): depth first over ``named_children``; every HQQ layer gets its attribute name as
    ``layer.name`` and is replaced by ``fct(layer, patch_param)``; anything else is descended into."""
    stack = [model]
    while stack:
        parent = stack.pop()
        for attr, child in list(parent.named_children()):
            if not is_hqq_layer(child):
                stack.append(child)
                continue
            child.name = attr
            setattr(parent, attr, fct(child, patch_params))


def _inner(layer):
    return layer.linear_layer if type(layer).__name__ == "HQQLinearLoRA" else layer


def patch_hqq_to_hip(layer, patch_params=None, load=False):
    """Counterpart of patch_hqq_to_gptq / patch_hqq_to_ft (autogptq.py:291-341,
    ft.py:148-197): HQQLinear -> HIPQuantLinear on the layer's device."""
    if not is_hqq_layer(layer):
        return layer
    hqq_layer = _inner(layer)
    h = hqq_layer.weights if isinstance(hqq_layer, HQQWeightsModule) else from_hqq_layer(hqq_layer)
    h.name = getattr(hqq_layer, "name", None) or getattr(layer, "name", None)
    n, k = h.shape
    device = (patch_params or {}).get("device", None) or h.W_q.device
    # bfloat16 layers (compute_dtype = bfloat16) become fp16 modules like every module the reference's patchers build (ft.py:62) -- grouped, fused,
    # served by the decode runner -- unless the caller asks to keep HQQ's bf16 arithmetic (keep_bf16) and the bf16 kernels serve the layer's groups
    bf16 = bool((patch_params or {}).get("keep_bf16", False)) and h.scale.dtype == torch.bfloat16 and HIPQuantLinear.bf16_serves(h.group_size)
    if load:
        new = HIPQuantLinear(h.nbits, h.group_size, k, n, bias=h.bias, name=h.name,
                             weight_dtype=torch.bfloat16 if bf16 else torch.float16).to(device)
    else:
        new = HIPQuantLinear.from_hqq(h, device=device, keep_bf16=bf16)
    if type(layer).__name__ == "HQQLinearLoRA":
        layer.linear_layer = new
        return layer
    return new


def patch_hqq_to_hip_load(layer, patch_params=None):
    return patch_hqq_to_hip(layer, patch_params, load=True)


def patch_add_weight_param(layer, patch_param):
    """patching.py:76-91: dummy ``.weight`` so HF code can query dtype/device."""
    if isinstance(layer, (HIPQuantLinear, HIPOWQLinear)) and not hasattr(layer, "weight"):
        device = layer.W_out.device if isinstance(layer, HIPOWQLinear) else layer.qweight.device
        layer.weight = torch.nn.Parameter(torch.zeros((1,), device=device, dtype=torch.float16), requires_grad=False)
    return layer


def _walk_hip(model, fct):
    for name, layer in model.named_children():
        if isinstance(layer, (HIPQuantLinear, HIPOWQLinear)):      # (an OWQ layer is one module: its inner packed layer is not walked)
            setattr(model, name, fct(layer, None))
        else:
            _walk_hip(layer, fct)


def _fusable(m):
    """a HIPQuantLinear the grouped / fused launches take"""
    return isinstance(m, HIPQuantLinear) and not m.is_bf16        # (bfloat16 modules run unfused: ops.linear_bf16)


def _same_group(mods):
    """siblings of ONE launch share the granularity of their native meta (128, or 64 / 32: amq_gemv_grouped_f16 takes one `group`)"""
    return len({getattr(m, "native_group", ops.GROUP) for m in mods}) == 1


def group_sibling_linears(model):
    """Install a :class:`LinearGroup` wherever a module holds HIPQuantLinear children named like one of SIBLING_GROUPS with equal
    input sizes: their few-row forwards then run as ONE grouped launch.  Returns the number of groups made.  The modules
    themselves (buffers, state_dict keys) are not changed.  Siblings that already form exactly this group are left alone; siblings
    that carry groups from ELSEWHERE -- the reference's driver assembles a mixed-precision model by ``setattr``-ing linears taken
    from three separately prepared models (amq_speed_benchmark.py:231-251) -- are regrouped with their new neighbours."""
    made = 0
    for parent in model.modules():
        for names in SIBLING_GROUPS:
            mods = [getattr(parent, n, None) for n in names]
            if not all(_fusable(m) for m in mods) or len({m.infeatures for m in mods}) != 1 or not _same_group(mods):
                continue
            grps = [m.__dict__.get("_group") for m in mods]
            if all(g is not None and g[0] is grps[0][0] and g[1] == i for i, g in enumerate(grps)) and len(grps[0][0].members) == len(mods) \
                    and all(a is b for a, b in zip(grps[0][0].members, mods)):
                continue
            LinearGroup(mods)
            made += 1
    return made


def fuse_llama_mlps(model):
    """Replace every SiLU-gated MLP whose gate / up / down projections are (bias-free) HIPQuantLinear modules by
    :class:`HIPLlamaMLP` (two launches per few-row forward).  Recognised by structure: children ``gate_proj``, ``up_proj``,
    ``down_proj`` and an ``act_fn`` that is SiLU.  Returns the number of modules replaced."""
    n = 0
    for parent in list(model.modules()):
        for name, mod in list(parent.named_children()):
            if isinstance(mod, HIPLlamaMLP):
                continue
            kids = [getattr(mod, k, None) for k in ("gate_proj", "up_proj", "down_proj")]
            act = getattr(mod, "act_fn", None)
            is_silu = isinstance(act, torch.nn.SiLU) or type(act).__name__ in ("SiLUActivation", "SiLU")
            if all(_fusable(k) and k.bias is None for k in kids) and is_silu and _same_group(kids[:2]):      # (gate / up share a launch)
                setattr(parent, name, HIPLlamaMLP(*kids))
                n += 1
    return n


# RMSNorm classes whose forward is weight * x / sqrt(mean(x^2) + eps) with fp32 statistics (HF LlamaRMSNorm; module_walk's own)
# (transformers' Mistral / Qwen2 classes are generated from the Llama ones: the same forward, token for token)
RMSNORM_CLASSES = ("LlamaRMSNorm", "MistralRMSNorm", "Qwen2RMSNorm", "_RMSNorm")
# decoder layers whose ``forward`` is LlamaDecoderLayer's (checked by signature as well: fuse_llama_layers)
HF_LAYER_CLASSES = ("LlamaDecoderLayer", "MistralDecoderLayer", "Qwen2DecoderLayer")


def fuse_llama_norms(model):
    """In every Llama decoder layer -- a module with children ``input_layernorm``, ``self_attn``, ``post_attention_layernorm``,
    ``mlp`` -- whose q/k/v projections are one LinearGroup and whose MLP is a HIPLlamaMLP, wrap the two RMSNorms in
    :class:`HIPRMSNorm`: few-row forwards then form the norm in the prologue of the grouped launch that follows it (9 -> 7
    launches per block for a module swap).  Only the norm classes of RMSNORM_CLASSES are touched.  Returns the number wrapped."""
    n = 0
    for layer in list(model.modules()):
        attn, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
        if attn is None or mlp is None:
            continue
        qkv = [getattr(attn, k, None) for k in SIBLING_GROUPS[0]]
        grp = qkv[0].__dict__.get("_group") if all(_fusable(m) and m.bias is None for m in qkv) else None
        if grp is not None and not (len(grp[0].members) == 3 and all(a is b for a, b in zip(grp[0].members, qkv))):
            grp = None
        for name, consumer in (("input_layernorm", grp[0] if grp is not None else None),
                               ("post_attention_layernorm", mlp if isinstance(mlp, HIPLlamaMLP) else None)):
            norm = getattr(layer, name, None)
            slot = "qkv" if name == "input_layernorm" else "mlp"
            if isinstance(norm, HIPRMSNorm):
                # a second prepare_for_inference (or a sibling transplanted since): the wrapper exists but may point at a group that no
                # longer owns q/k/v -- re-target it, or un-fuse it when its launch is gone
                if consumer is None:
                    setattr(layer, name, norm.__dict__["_inner"])
                elif norm.__dict__.get("_consumer") is not consumer or norm.__dict__.get("_owner") is not layer:
                    norm.retarget(consumer, layer, slot)
                    n += 1
                continue
            if consumer is None or norm is None or type(norm).__name__ not in RMSNORM_CLASSES or getattr(norm, "weight", None) is None:
                continue
            setattr(layer, name, HIPRMSNorm(norm, consumer, layer, slot))
            n += 1
    return n


def _fused_attention(layer, h, residual, call):
    """``residual + self_attn(h)`` with the add formed in o_proj's epilogue when that call can take it (HIPQuantLinear._forward_residual):
    the residual is offered to o_proj through a one-shot holder for the duration of the attention call only."""
    o_proj = getattr(layer.self_attn, "o_proj", None)
    if not _fusable(o_proj) or not residual.is_cuda or residual.dtype is not torch.float16:
        return residual + call(h)
    hold = [residual]
    o_proj.__dict__["_residual"] = hold
    try:
        out = call(h)
    finally:
        o_proj.__dict__.pop("_residual", None)
    return out if hold[0] is None else residual + out


def _hf_llama_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                            position_embeddings=None, **kwargs):
    """transformers 5.x ``LlamaDecoderLayer.forward`` (modeling_llama.py) with the two ``residual + hidden_states`` adds folded into
    the o_proj / down_proj launches: same modules, same order, same values (the epilogue adds the residual to the fp16-rounded
    projection, i.e. the two roundings of the separate add)."""
    attn = lambda h: self.self_attn(hidden_states=h, attention_mask=attention_mask, position_ids=position_ids,
                                    past_key_values=past_key_values, use_cache=use_cache, position_embeddings=position_embeddings,
                                    **kwargs)[0]
    hidden_states = _fused_attention(self, self.input_layernorm(hidden_states), hidden_states, attn)
    h = self.post_attention_layernorm(hidden_states)
    if isinstance(self.mlp, HIPLlamaMLP):
        return self.mlp(h, residual=hidden_states)
    return hidden_states + self.mlp(h)


def _walk_block_forward(self, x):
    """module_walk._Block.forward (the HF layer's shape without HF's argument plumbing), fused the same way"""
    x = _fused_attention(self, self.input_layernorm(x), x, self.self_attn)
    h = self.post_attention_layernorm(x)
    if isinstance(self.mlp, HIPLlamaMLP):
        return self.mlp(h, residual=x)
    return x + self.mlp(h)


_HF_LAYER_PARAMS = ["self", "hidden_states", "attention_mask", "position_ids", "past_key_values", "use_cache", "position_embeddings", "kwargs"]


def fuse_llama_layers(model):
    """Fold the decoder layers' residual adds into the o_proj / down_proj launches: the layer instance's ``forward`` is replaced
    by a function that runs the SAME sub-modules in the same order and offers each residual to the projection that precedes its add
    (7 -> 5 launches per block for few rows; more rows, biases or other dtypes fall back to the plain add).  Only layers whose
    forward is known are touched: transformers' ``LlamaDecoderLayer`` with exactly the 5.x signature (its body is what
    ``_hf_llama_layer_forward`` restates) and module_walk's ``_Block``; the reference's FT path replaces Llama forwards the same
    way (kernel/monkeypatch/ftllama_modeling.py:39-46, 127-155).  Returns the number of layers patched."""
    import inspect
    import types
    n = 0
    for layer in model.modules():
        cls = type(layer)
        if "forward" in layer.__dict__ or not all(hasattr(layer, k) for k in ("input_layernorm", "self_attn", "post_attention_layernorm", "mlp")):
            continue
        if cls.__name__ == "_Block" and cls.__module__.endswith("module_walk"):
            layer.forward = types.MethodType(_walk_block_forward, layer)
        elif cls.__name__ in HF_LAYER_CLASSES and list(inspect.signature(cls.forward).parameters) == _HF_LAYER_PARAMS:
            layer.forward = types.MethodType(_hf_llama_layer_forward, layer)
        else:
            continue
        n += 1
    return n


def _decoder_linears(model):
    """[(block index, 'self_attn.q_proj' ..., parent module, attribute, nn.Linear)] of an HF llama / mistral / qwen2 / qwen3 causal LM: the seven
    projections of every decoder layer (arch.LINEARS).  lm_head, the embeddings and the norms are not listed: they stay dense, as in the
    reference's AutoHQQHFModel.quantize_model."""
    from .arch import LINEARS
    layers = getattr(getattr(model, "model", None), "layers", None)
    if layers is None:
        raise TypeError("expected an HF Llama-family causal LM (model.model.layers)")
    out = []
    for b, layer in enumerate(layers):
        for full in LINEARS:
            parent_name, attr = full.split(".")
            parent = getattr(layer, parent_name, None)
            lin = getattr(parent, attr, None)
            if lin is None:
                raise TypeError(f"layer {b}: no {full} (not a Llama-family decoder layer)")
            if not isinstance(lin, torch.nn.Linear):
                raise TypeError(f"layer {b}: {full} is a {type(lin).__name__}, not a dense nn.Linear (already quantized?)")
            out.append((b, full, parent, attr, lin))
    return out


def _bits_of(bits, name, block):
    """an int for every linear, or per-linear bit-widths {'self_attn.q_proj': [bits per block], ...} (an arch's 'linear' entry: arch.arch_bits)"""
    if isinstance(bits, dict):
        from .arch import arch_bits
        return arch_bits(bits.get("linear", bits), name, block)
    if int(bits) not in (2, 3, 4):
        raise ValueError(f"bits must be 2, 3 or 4 (got {bits})")
    return int(bits)


def _default_device(model, device):
    """``device``, or the model's own GPU, else cuda:0"""
    if device is None:
        p = next(model.parameters())
        device = p.device if p.is_cuda else torch.device("cuda:0")
    return torch.device(device)


def _block_linears(layer):
    """{'self_attn.q_proj': module, ...} over arch.LINEARS of one decoder layer"""
    from .arch import LINEARS
    return {name: getattr(getattr(layer, name.split(".")[0]), name.split(".")[1]) for name in LINEARS}


def _set_linear(layer, name, module):
    parent_name, attr = name.split(".")
    setattr(getattr(layer, parent_name), attr, module)


def _rtn_dequantized(W, nbits, group_size):
    """what hqq_format.quantize_rtn of W dequantizes to on the device: the round-to-nearest column of the calibrated quantizers' reports"""
    from .hqq_format import quantize_rtn
    r = quantize_rtn(W, nbits, group_size)
    return ops.dequantize_hqq(r.W_q.contiguous(), r.scale.reshape(-1).contiguous(), r.zero.reshape(-1).contiguous(), nbits, *W.shape, group_size)


class _BlockInputCaught(Exception):
    pass


@contextlib.contextmanager
def _calibrating(model, samples, device):
    """What a block-by-block calibration walk (GPTQ, AWQ) starts and ends with: the model is dense (TypeError) and moves to ``device``; ``samples``
    are token-id tensors [1, seqlen] of one length (ValueError); with ``use_cache`` off, a forward pre-hook catches the first block's inputs and
    keyword arguments over the samples.  Yields (device, inps, kwargs, run) with ``run(layer, x)`` a block's output for one input;
    ``config.use_cache`` is put back on the way out, also when the walk raises."""
    _decoder_linears(model)
    samples = list(samples)
    if not samples or any(s.dim() != 2 or s.shape != samples[0].shape for s in samples):
        raise ValueError("samples: expected token-id tensors [1, seqlen] of one length")
    device = _default_device(model, device)
    model.to(device)
    use_cache = getattr(model.config, "use_cache", None)
    model.config.use_cache = False
    inps, kwargs = [], {}

    def catch(_, args, kw):
        inps.append((args[0] if args else kw["hidden_states"]).detach())
        kwargs.update({k: v for k, v in kw.items() if k != "hidden_states"})
        raise _BlockInputCaught

    def run(layer, x):
        out = layer(x, **kwargs)
        return out[0] if isinstance(out, (tuple, list)) else out

    handle = model.model.layers[0].register_forward_pre_hook(catch, with_kwargs=True)
    try:
        try:
            for s in samples:
                try:
                    model(s.to(device))
                except _BlockInputCaught:
                    pass
        finally:
            handle.remove()
        yield device, inps, kwargs, run
    finally:
        if use_cache is not None:
            model.config.use_cache = use_cache


@torch.no_grad()
def quantize_model(model, bits, group_size=128, device=None):
    """The reference's ``AutoHQQHFModel.quantize_model(model, BaseQuantizeConfig(nbits, group_size))`` (amq_quantization_proxy.py:36-37) on the GPU:
    every decoder linear of a dense HF llama / mistral / qwen2 / qwen3 model is quantized with HQQ's solver (ops.hqq_quantize) and replaced by the
    HIPQuantLinear holding it; lm_head, embeddings and norms stay dense and the whole model ends on ``device`` (default: the model's own GPU, else
    cuda:0).  ``bits``: 2, 3 or 4, or per-linear bit-widths as an arch's ``'linear'`` dict holds them.  The model is then ready for
    ``prepare_for_inference(backend='hip')`` (grouping and fusion), ``QuantLlama.from_hf`` and ``evaluate.eval_ppl`` / ``eval_loss``."""
    todo = _decoder_linears(model)
    device = _default_device(model, device)
    for b, full, parent, attr, lin in todo:
        lin.name = attr
        setattr(parent, attr, HIPQuantLinear.from_linear(lin, _bits_of(bits, full, b), group_size, device=device))
    return model.to(device)


@torch.no_grad()
def quantize_bank(model, bits=(2, 3, 4), group_size=128, device=None):
    """Every decoder linear of a dense HF model at every bit-width of ``bits``: {nbits: {(block, 'self_attn.q_proj'): HQQWeights}} on the GPU, the
    model itself untouched -- what the reference's search holds as its per-bit model bank.  An arch picks one entry per (block, linear); the picks
    are ``QuantLlama(hqq_layers=...)``'s input."""
    device = _default_device(model, device)
    bank = {int(b): {} for b in bits}
    for b, full, _, attr, lin in _decoder_linears(model):
        w = lin.weight.detach().to(device)
        bias = None if lin.bias is None else lin.bias.detach().to(device, torch.float16)
        for nb in bank:
            bank[nb][(b, full)] = ops.hqq_quantize(w, nb, group_size, bias=bias, name=attr)
    return bank


TRUE_SEQUENTIAL = (("self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj"), ("self_attn.o_proj",), ("mlp.up_proj", "mlp.gate_proj"),
                   ("mlp.down_proj",))      # gptq.py:100-105


def _proxy_loss(W, W_hat, H):
    """tr(dW H dW^T) in fp32 torch ops on the device"""
    d = W.float() - W_hat.float()
    return float(((d @ H) * d).sum().item())


@torch.no_grad()
def quantize_model_gptq(model, bits, samples, group_size=128, percdamp=0.01, true_sequential=False, device=None, act_order=False,
                        static_groups=False):
    """The reference's ``GPTQ.run`` (amq/quantization/gptq.py:25-161: asymmetric, grouped; act_order and static_groups as below) for a dense HF
    llama / mistral / qwen2 / qwen3 model, ending in packed layers: block by block, one Hessian per linear is accumulated over ``samples`` with
    forward hooks (ops.GPTQHessian), every linear is quantized at ``_bits_of(bits, name, block)`` by the error-feedback solve (ops.gptq_hinv,
    ops.gptq_quantize: HIP kernels) and its dense weights are overwritten by what the packed layer dequantizes to, so that the block's second
    forward hands the next block the quantized model's activations; then the block's linears become HIPQuantLinear modules.  ``samples``: token-id
    tensors [1, seqlen] of one length, brought by the caller.  ``true_sequential``: the reference's four subsets per block (q/k/v, o, gate/up,
    down), each calibrated on the outputs of the quantized ones before it.  The whole model works on ``device`` (default: the model's own GPU,
    else cuda:0).  Returns (model, report) with ``report[(block, name)] = {"loss": tr(dW H dW^T), "rtn_loss": the same for
    hqq_format.quantize_rtn at the same bits and group, "solver_loss": the solve's own sum of row losses (the reference's printed error), "dead":
    the number of dead columns, "bits", "act_order", "static_groups"}``.  The model is then ready for ``prepare_for_inference(backend='hip')``.

    ``static_groups``: every group's (scale, zero) comes from the layer's original columns, not from the running ones.  ``act_order`` (with
    ``static_groups``): the solve walks the columns by descending ``diag(H)`` (ops.gptq_act_order) over the factor of the equally permuted Hessian;
    the packed layer stays in its own column order, an ordinary Format A layer on every fast path.  ``act_order`` without ``static_groups`` is
    refused (NotImplementedError): its groups run over the permuted columns and would need a gather at run time."""
    from .arch import LINEARS
    if act_order and not static_groups:
        raise NotImplementedError("quantize_model_gptq: act_order without static_groups forms its groups over the permuted columns, which is not "
                                  "a Format A layer (it would need a gather of x at run time); pass static_groups=True as well")
    report = {}
    with _calibrating(model, samples, device) as (device, inps, _, run):
        for b, layer in enumerate(model.model.layers):
            full = _block_linears(layer)
            packed = {}
            for names in (TRUE_SEQUENTIAL if true_sequential else (tuple(LINEARS),)):
                hess = {name: ops.GPTQHessian(full[name].in_features, device) for name in names}
                handles = [full[name].register_forward_hook(lambda _, inp, out, acc=hess[name]: acc.add_batch(inp[0].detach())) for name in names]
                try:
                    for x in inps:
                        run(layer, x)
                finally:
                    for h in handles:
                        h.remove()
                for name in names:
                    lin, nb = full[name], _bits_of(bits, name, b)
                    H = hess[name].H
                    perm = ops.gptq_act_order(H) if act_order else None
                    U, dead = ops.gptq_hinv(H if perm is None else H[perm][:, perm], percdamp, name=f"{b}.{name}")
                    if perm is not None:
                        dead = torch.diag(H) == 0              # (gptq_hinv's mask is in walk order)
                    W = lin.weight.detach().to(torch.float16).clone()
                    W[:, dead] = 0
                    bias = None if lin.bias is None else lin.bias.detach().to(device, torch.float16)
                    h, info = ops.gptq_quantize(W, U, nb, group_size, return_info=True, bias=bias, name=name.split(".")[1], perm=perm,
                                                static_groups=static_groups)
                    W_hat = ops.dequantize_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), nb, *W.shape, group_size)
                    report[(b, name)] = {"loss": _proxy_loss(W, W_hat, H), "rtn_loss": _proxy_loss(W, _rtn_dequantized(W, nb, group_size), H),
                                         "solver_loss": info.loss, "dead": int(dead.sum().item()), "bits": nb,
                                         "act_order": bool(act_order), "static_groups": bool(static_groups)}
                    lin.weight.data = W_hat.to(lin.weight.dtype)
                    packed[name] = h
            inps = [run(layer, x).detach() for x in inps]
            for name, h in packed.items():
                _set_linear(layer, name, HIPQuantLinear.from_hqq(h, device=device))
    return model, report


OWQ_RATIOS = {"self_attn.q_proj": 1, "self_attn.k_proj": 1, "self_attn.v_proj": 1, "self_attn.o_proj": 1, "mlp.up_proj": 0.375,
              "mlp.gate_proj": 0.375, "mlp.down_proj": 0.375}      # the reference's model_config.json "ratios" for the Llama family


def owq_n_out(K, avg_bits, name, group_size=128):
    """The reference's number of fp16 columns of a linear with K input columns (owq.py:69-70, 146-153): ``avg_bits`` is the arch's
    ``get_bits_usage`` (the group's 32 / group_size bits of scale and zero included, which the rule takes off again),
    r = 12 / (16 - (avg_bits - 32 / group_size)) * 0.1 / 7 over the seven linears, n_out = round(K * r * ratio), made even."""
    r = (12 / (16 - (avg_bits - (32 / group_size if group_size > 0 else 0)))) * 0.1
    r /= len(OWQ_RATIOS)
    n_out = round(K * r * OWQ_RATIOS[name])
    return n_out + n_out % 2


def _owq_avg_bits(model, bits, group_size):
    """arch.get_bits_usage over the model's own decoder linears: the mean of bits + 32 / group_size, weighted by the linears' sizes"""
    mem = numel = 0.0
    for b, full, _, _, lin in _decoder_linears(model):
        n = lin.weight.numel()
        mem += n * (_bits_of(bits, full, b) + 32 / group_size)
        numel += n
    return mem / numel


@torch.no_grad()
def quantize_model_owq(model, bits, samples, group_size=128, percdamp=0.01, true_sequential=True, frob_norm=True, n_out=None, device=None):
    """The reference's ``OWQ.run`` (amq/quantization/owq.py:50-237: asymmetric, grouped, act_order=False) for a dense HF llama / mistral / qwen2 /
    qwen3 model, ending in deployable layers (the reference only writes fake-quantized fp16 weights): block by block and subset by subset (the
    four ``TRUE_SEQUENTIAL`` subsets by default, as the reference's), one Hessian per linear is accumulated over ``samples`` with forward hooks
    (ops.GPTQHessian); per linear the outlier columns are chosen (ops.owq_select: the whole-row range pass, sens = diag(H) * the columns'
    round-off; ``frob_norm=False``: diag(H) alone), W and H are permuted, and the solve (ops.gptq_hinv, ops.owq_quantize: HIP kernels) leaves a
    packed layer over the kept columns and the fp16 outlier columns that absorbed the error feedback.  The dense weights are overwritten by what
    the new layer dequantizes to for the block's second forward; at the block's end the linears become HIPOWQLinear modules (HIPQuantLinear where
    n_out is 0).  ``n_out``: None = the reference's rule (``owq_n_out`` at the assignment's average bits), an int for every linear, or a dict
    name -> int (names as in arch.LINEARS; a missing name takes the rule).  Groups of 128 only.  Returns (model, report) with
    ``report[(block, name)] = {"loss", "rtn_loss", "solver_loss", "dead", "bits", "n_out", "out_ids"}`` -- loss = tr(dW H dW^T) over all K
    columns, the outliers' change included.  ``prepare_for_inference(backend='hip')`` leaves an OWQ model's layers as they are; the hipGraph
    runner takes them (``QuantLlama.from_hf``, ``hf_fast.convert_model_to_hip``, ``evaluate``: the staged token step)."""
    from .arch import LINEARS
    if int(group_size) != 128:
        raise ValueError(f"the OWQ kernels serve groups of 128 only (got {group_size})")
    report = {}
    avg_bits = _owq_avg_bits(model, bits, group_size)

    def outliers(name, K):
        want = n_out.get(name) if isinstance(n_out, dict) else n_out
        return owq_n_out(K, avg_bits, name, group_size) if want is None else int(want)

    with _calibrating(model, samples, device) as (device, inps, _, run):
        for b, layer in enumerate(model.model.layers):
            full = _block_linears(layer)
            made = {}
            for names in (TRUE_SEQUENTIAL if true_sequential else (tuple(LINEARS),)):
                hess = {name: ops.GPTQHessian(full[name].in_features, device) for name in names}
                handles = [full[name].register_forward_hook(lambda _, inp, out, acc=hess[name]: acc.add_batch(inp[0].detach())) for name in names]
                try:
                    for x in inps:
                        run(layer, x)
                finally:
                    for h in handles:
                        h.remove()
                for name in names:
                    lin, nb = full[name], _bits_of(bits, name, b)
                    H = hess[name].H
                    W = lin.weight.detach().to(torch.float16).clone()
                    K = W.shape[1]
                    no = outliers(name, K)
                    if frob_norm:
                        ids, out_ids = ops.owq_select(W, H, no, nb)
                    else:
                        ids, out_ids = ops.owq_select(W, H, 0, nb) if no == 0 else _owq_select_by_hessian(H, no)
                    Hp = H[ids][:, ids]
                    U, dead = ops.gptq_hinv(Hp, percdamp, name=f"{b}.{name}")
                    Wp = W[:, ids].contiguous()
                    Wp[:, dead] = 0
                    bias = None if lin.bias is None else lin.bias.detach().to(device, torch.float16)
                    h, W_out, info = ops.owq_quantize(Wp, U, no, nb, group_size, return_info=True, bias=bias, name=name.split(".")[1])
                    mod = HIPOWQLinear.from_owq(h, W_out, ids, device=device)
                    W_hat = mod.dequantize()
                    W0 = W.clone()
                    W0[:, ids[dead]] = 0
                    report[(b, name)] = {"loss": _proxy_loss(W0, W_hat, H), "rtn_loss": _proxy_loss(W0, _rtn_dequantized(W0, nb, group_size), H),
                                         "solver_loss": info.loss, "dead": int(dead.sum().item()), "bits": nb, "n_out": no,
                                         "out_ids": out_ids.cpu()}
                    lin.weight.data = W_hat.to(lin.weight.dtype)
                    made[name] = mod
            inps = [run(layer, x).detach() for x in inps]
            for name, mod in made.items():
                _set_linear(layer, name, mod)
    return model, report


def _owq_select_by_hessian(H, n_out):
    """owq.py hessian_sorting without frob_norm: the columns of largest diag(H)"""
    K = H.shape[0]
    desc = torch.argsort(torch.diag(H), descending=True, stable=True)
    keep = torch.ones(K, dtype=torch.bool, device=H.device)
    keep[desc[:n_out]] = False
    return torch.cat([torch.arange(K, device=H.device)[keep], desc[:n_out]]), torch.sort(desc[:n_out])[0].to(torch.int32)


AWQ_GRID = 20        # ratios r / 20 of the scale search (auto_scale.py:114)


def _awq_fake_quant(W, nbits, group_size, s):
    return ops.awq_quantize(W, nbits, group_size, col_scale=s, dense=True)


@torch.no_grad()
def awq_search_scale(inspect, linears, x, bits, group_size, kwargs=None, fake_quant=None):
    """The reference's ``_search_module_scale_per_linear`` (awq_utils/auto_scale.py:96-146): the per-input-channel scale of ``linears`` (name ->
    nn.Linear inside ``inspect``, all fed by ``x`` [windows, seqlen, K] or [rows, K]) that loses least at ``inspect``'s output.  ``x_mean`` is the
    mean of |x| per channel in fp32; for the ratios r / 20, r = 0 .. 19, ``s = clamp(x_mean ^ ratio, 1e-4)`` over ``sqrt(max(s) min(s))``; every
    linear's weight data is swapped for ``fake_quant(W, bits, group_size, s)`` -- by default ops.awq_quantize(..., col_scale=s, dense=True), the HIP
    kernel: fp16 W times s, rounded to nearest, divided by s again --; the loss is the mean of ``(org - out).float() ** 2`` over all rows, window by
    window, summed in fp64; the first strict minimum wins.  The original weight tensors are put back by reference.  ``bits``: an int or name -> int.
    Returns (s fp32 [K], ratio, the 20 losses)."""
    kwargs = {} if kwargs is None else {k: v for k, v in kwargs.items() if k != "use_cache"}
    fake_quant = _awq_fake_quant if fake_quant is None else fake_quant
    windows = x if x.dim() == 3 else x.unsqueeze(0)
    dtype = next(iter(linears.values())).weight.dtype

    def run(xw):
        out = inspect(xw.unsqueeze(0).to(dtype), **kwargs)
        return out[0] if isinstance(out, (tuple, list)) else out

    org = [run(xw) for xw in windows]
    count = sum(o.numel() for o in org)
    x_mean = x.reshape(-1, x.shape[-1]).abs().float().mean(0)
    keep = {name: lin.weight.data for name, lin in linears.items()}
    history, best = [], None
    try:
        for r in range(AWQ_GRID):
            ratio = r / AWQ_GRID
            s = x_mean.pow(ratio).clamp(min=1e-4)
            s = s / (s.max() * s.min()).sqrt()
            for name, lin in linears.items():
                nb = bits[name] if isinstance(bits, dict) else bits
                lin.weight.data = fake_quant(keep[name], int(nb), group_size, s).to(keep[name].dtype)
            loss = 0.0
            for xw, o in zip(windows, org):
                loss += float((o - run(xw)).float().pow(2).double().sum().item())
            loss /= count
            history.append(loss)
            if best is None or loss < best[0]:
                best = (loss, ratio, s)
    finally:
        for name, lin in linears.items():
            lin.weight.data = keep[name]
    if not all(v == v for v in history) or bool(torch.isnan(best[2]).any()):
        raise ValueError(f"awq_search_scale: a loss or a scale is NaN ({history})")
    return best[2].detach(), best[1], history


def _awq_searches(layer, feats, kwargs, bits, b, group_size, fake_quant=None):
    """the four searches of one Llama-family block (auto_scale.py:166-220), each against the unmodified block: [(prev op, its kind, names, s,
    ratio, losses)]"""
    attn, mlp, full = layer.self_attn, layer.mlp, _block_linears(layer)
    nb = {name: _bits_of(bits, name, b) for name in full}
    todo = [(layer.input_layernorm, "norm", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), attn, kwargs)]
    if attn.v_proj.weight.shape == attn.o_proj.weight.shape:        # auto_scale.py:185 (not under GQA: v's rows are not o's columns)
        todo.append((attn.v_proj, "linear", ("self_attn.o_proj",), attn.o_proj, None))
    todo.append((layer.post_attention_layernorm, "norm", ("mlp.gate_proj", "mlp.up_proj"), mlp, None))
    todo.append((mlp.up_proj, "linear", ("mlp.down_proj",), mlp.down_proj, None))
    found = []
    for prev, kind, names, inspect, kw in todo:
        linears = {name: full[name] for name in names}
        s, ratio, losses = awq_search_scale(inspect, linears, feats[names[0]], nb, group_size, kwargs=kw, fake_quant=fake_quant)
        found.append((prev, kind, names, s, ratio, losses))
    return found


def _awq_apply_scale(layer, found, feats=None):
    """auto_scale.py apply_scale: a norm's weight is divided by s, a linear prev-op's last len(s) rows (and bias) are; every scaled linear becomes
    fp16(w * s); the stored inputs are divided by s"""
    for prev, kind, names, s, _, _ in found:
        if kind == "norm":
            prev.weight.data = (prev.weight.data.float() / s).to(prev.weight.dtype)
        else:
            w = prev.weight.data
            w[-s.numel():] = (w[-s.numel():].float() / s.view(-1, 1)).to(w.dtype)
            if prev.bias is not None:
                prev.bias.data[-s.numel():] = (prev.bias.data[-s.numel():].float() / s).to(prev.bias.dtype)
        for name in names:
            lin = _block_linears(layer)[name]
            lin.weight.data = (lin.weight.data.float() * s.view(1, -1)).to(lin.weight.dtype)
        if feats is not None:
            feats[names[0]] = (feats[names[0]].float() / s).to(feats[names[0]].dtype)


_AWQ_INPUT_OF = {"self_attn.q_proj": "self_attn.q_proj", "self_attn.k_proj": "self_attn.q_proj", "self_attn.v_proj": "self_attn.q_proj",
                 "self_attn.o_proj": "self_attn.o_proj", "mlp.gate_proj": "mlp.gate_proj", "mlp.up_proj": "mlp.gate_proj",
                 "mlp.down_proj": "mlp.down_proj"}


@torch.no_grad()
def quantize_model_awq(model, bits, samples, group_size=128, clip=True, n_sample_token=512, device=None):
    """The reference's ``run_awq`` + ``apply_awq`` (amq/quantization/awq_utils/pre_quant.py:80-234: zero_point=True, clip_asym=True, per-linear bits)
    for a dense HF llama / mistral / qwen2 / qwen3 model, ending in packed layers -- which the reference, whose AWQ writes fake-quantized fp16
    weights back, cannot produce.  Block by block: one pass of the dense block over ``samples`` collects the inputs of q_proj (shared by k and v),
    o_proj, gate_proj (shared by up) and down_proj as fp16 rows on the device and hands the next block its inputs (AWQ calibrates on dense
    activations); the four scale searches run against the unmodified block (:func:`awq_search_scale`; o_proj's only when v_proj has its shape);
    the scales are folded into the norms / previous linears, the linears and the stored inputs; with ``clip`` every linear but q_proj and k_proj
    gets its per-group bounds from ``ops.awq_clip`` on the rows ``x[0 :: rows // n_sample_token]`` (the reference's stride: it can yield more than
    ``n_sample_token`` rows); ``ops.awq_quantize`` packs.  ``samples``: token-id tensors [1, seqlen] of one length, brought by the caller.
    Returns (model, report) with ``report[(block, name)] = {"bits", "ratio": the chosen r / 20 (None for o_proj where its search is skipped),
    "search_loss": the 20 losses of its search (None likewise), "clip_steps": the histogram of the chosen shrink steps (None without clip),
    "loss": the mean squared output error of the packed layer on its scaled sampled inputs against the dense layer on the unscaled ones,
    "rtn_loss": the same for hqq_format.quantize_rtn of the original weights}``.  The model is then ready for
    ``prepare_for_inference(backend='hip')``."""
    from .arch import LINEARS
    report = {}
    with _calibrating(model, samples, device) as (device, inps, kwargs, run):
        attn_kwargs = {k: v for k, v in kwargs.items() if k != "use_cache"}
        for b, layer in enumerate(model.model.layers):
            full = _block_linears(layer)
            caught = {name: [] for name in set(_AWQ_INPUT_OF.values())}
            handles = [full[name].register_forward_hook(lambda _, inp, out, acc=caught[name]: acc.append(inp[0].detach().to(torch.float16)))
                       for name in caught]
            try:
                inps = [run(layer, x).detach() for x in inps]
            finally:
                for h in handles:
                    h.remove()
            feats = {name: torch.cat(v, dim=0) for name, v in caught.items()}        # [windows, seqlen, K]
            found = _awq_searches(layer, feats, attn_kwargs, bits, b, group_size)
            searched = {name: (ratio, losses) for _, _, names, _, ratio, losses in found for name in names}
            # the sampled rows of every input, before and after the scales reach them
            sampled = {}
            for name in caught:
                rows = feats[name].reshape(-1, feats[name].shape[-1])
                sampled[name] = rows[0::max(1, rows.shape[0] // int(n_sample_token))].clone()
            dense_w = {name: full[name].weight.detach().to(torch.float16).clone() for name in LINEARS}
            _awq_apply_scale(layer, found, feats)
            for name in LINEARS:
                lin, nb = full[name], _bits_of(bits, name, b)
                attr = name.split(".")[1]
                W = lin.weight.detach().to(torch.float16).contiguous()
                N, K = W.shape
                rows = feats[_AWQ_INPUT_OF[name]].reshape(-1, K)
                xs = rows[0::max(1, rows.shape[0] // int(n_sample_token))].contiguous()
                hi = lo = steps = None
                if clip and attr not in ("q_proj", "k_proj"):       # auto_clip.py:16: hard to clip precisely in front of the q k product
                    hi, lo, info = ops.awq_clip(W, xs, nb, group_size, return_info=True)
                    steps = torch.bincount(info.best.reshape(-1).long(), minlength=10).tolist()
                bias = None if lin.bias is None else lin.bias.detach().to(device, torch.float16)
                h = ops.awq_quantize(W, nb, group_size, hi=hi, lo=lo, bias=bias, name=attr)
                W_hat = ops.dequantize_hqq(h.W_q, h.scale.reshape(-1), h.zero.reshape(-1), nb, N, K, group_size)
                W_rtn = _rtn_dequantized(dense_w[name], nb, group_size)
                x0 = sampled[_AWQ_INPUT_OF[name]]
                want = torch.nn.functional.linear(x0, dense_w[name]).float()
                ratio, losses = searched.get(name, (None, None))
                report[(b, name)] = {"bits": nb, "ratio": ratio, "search_loss": losses, "clip_steps": steps,
                                     "loss": float((torch.nn.functional.linear(xs, W_hat).float() - want).pow(2).mean().item()),
                                     "rtn_loss": float((torch.nn.functional.linear(x0, W_rtn).float() - want).pow(2).mean().item())}
                _set_linear(layer, name, HIPQuantLinear.from_hqq(h, device=device))
    return model, report


def _merge_zeros_with_lora(model):
    """``allow_merge=True`` (patching.py:210-216, patch_merge_zeros_with_lora :239-275): the reference folds the zero-point term
    of an HQQLinearLoRA into its LoRA factors -- only for layers quantized WITHOUT groups along axis 1 (":243-245: axis == 0 or a
    group_size -> 'Skipping zeros lora merging'").  Every AMQ layer has group_size 128, so on AMQ's path the reference skips every
    layer; this does the same walk, prints the same line for what the reference skips and refuses the one case it would merge
    (group-less symmetric kernels are not part of this package)."""
    for name, layer in model.named_modules():
        if type(layer).__name__ != "HQQLinearLoRA":
            continue
        meta = getattr(getattr(layer, "linear_layer", None), "meta", None) or {}
        if meta.get("axis") == 0 or meta.get("group_size") is not None:
            print("Skipping zeros lora merging for", getattr(layer, "name", name))
        else:
            raise NotImplementedError(f"allow_merge: {name} is quantized without groups; zero/LoRA merging for group-less layers "
                                      "is outside the AMQ path (group_size 128)")


def prepare_for_inference(model, allow_merge=False, backend="hip", verbose=False, load_path=None, group_siblings=True, fuse_mlp=True,
                          fuse_norms=True, fuse_layers=True, kernel_arithmetic=False, keep_bf16=False):
    """patching.py:143-223 for the HIP backend.  ``kernel_arithmetic`` (default off): the swapped linears dequantize like the reference's GPTQ /
    FT CUDA kernels -- w = fma(q, s, -fp16(z s)), one rounding, what its own ``backend='gptq'`` / ``'ft'`` paths compute -- instead of like HQQ's
    ``dequantize()`` (two roundings, the default here: bit-identical to ``W_deq``).  The two differ by the rounding of c = fp16(z s): |dw| <= ~ulp(z s),
    i.e. relative to |z s|, not to |w| (several ulps of a weight with |q - z| << z) -- exactly the reference's ``backend='gptq'`` numerics; 5-8 % faster decode
    (HIPQuantLinear.to_kernel_arithmetic).  The cache file always holds the HQQ form.  ``group_siblings`` (default on; not in the reference): q/k/v and gate/up
    siblings are additionally tied into grouped launches (group_sibling_linears); ``fuse_mlp`` / ``fuse_norms``: SiLU-gated MLPs
    and the decoder layers' RMSNorms are fused into those launches (fuse_llama_mlps, fuse_llama_norms); ``fuse_layers``: the decoder
    layers' residual adds move into the o_proj / down_proj epilogues (fuse_llama_layers).  ``keep_bf16`` (default off): layers quantized with
    compute_dtype = bfloat16 keep HQQ's bf16 arithmetic (bfloat16 modules: ungrouped, unfused, groups of 128 and multiples) instead of
    becoming fp16 modules as under the reference's patchers."""
    if backend not in HIP_BACKENDS:
        raise RuntimeError(f"backend '{backend}' is not available in amq_amd (use one of {HIP_BACKENDS})")
    if allow_merge:
        _merge_zeros_with_lora(model)
    # the cache-file contract of patching.py:178-208: no path -> convert in place; a path that does not exist yet -> convert and
    # write the patched state_dict there; an existing file -> build empty modules and load it instead of re-packing
    cached = load_path is not None and os.path.exists(load_path)
    patch_linearlayers(model, patch_hqq_to_hip_load if cached else patch_hqq_to_hip, {"keep_bf16": keep_bf16}, verbose=verbose)
    if cached:
        print("Loading the model from", load_path)
        model.load_state_dict(torch.load(load_path, weights_only=True))
    elif load_path is not None:
        print("Saving the model to", load_path)
        torch.save(model.state_dict(), load_path)
    else:
        print("No load_path provided, using the model as is")
    _walk_hip(model, patch_add_weight_param)
    if kernel_arithmetic:
        owq_inner = {id(m.inner) for m in model.modules() if isinstance(m, HIPOWQLinear)}      # OWQ layers keep the arithmetic their solve saw
        for mod in model.modules():
            if isinstance(mod, HIPQuantLinear) and id(mod) not in owq_inner:
                mod.to_kernel_arithmetic()
    if group_siblings:
        group_sibling_linears(model)
    if fuse_mlp:                      # (not in the reference's generic patcher; its FT path swaps whole Llama sub-modules too)
        fuse_llama_mlps(model)
    if fuse_norms and group_siblings:
        fuse_llama_norms(model)
    if fuse_layers:                   # the decoder layers' residual adds into the o_proj / down_proj epilogues
        fuse_llama_layers(model)
    _warn_unfused(model, group_siblings, fuse_mlp, fuse_norms and group_siblings, fuse_layers)
    return model


def _warn_unfused(model, group_siblings, fuse_mlp, fuse_norms, fuse_layers):
    """One warning per fusion step that was asked for and found NOTHING to fuse on a model that does hold HIPQuantLinear projections
    with the Llama names: the steps recognise HF's module structure by shape (child names, SiLU, LlamaRMSNorm, the 5.x decoder-layer
    signature), so a transformers refactor would otherwise fall back to 13 launches per block without a word.  Correctness is not
    affected either way."""
    import warnings
    owq = [n for n, m in model.named_modules() if isinstance(m, HIPOWQLinear)]
    if owq:
        warnings.warn(f"prepare_for_inference: {len(owq)} OWQ layers ({', '.join(owq[:3])}{', ...' if len(owq) > 3 else ''}) stay as they are: "
                      "a HIPOWQLinear is not grouped with its siblings and not fused (its gather has no place in those launches); the hipGraph "
                      "runner takes them as they are (QuantLlama.from_hf: one stage launch in front of each packed GEMV)",
                      RuntimeWarning, stacklevel=3)
    owq_inner = {id(m.inner) for m in model.modules() if isinstance(m, HIPOWQLinear)}
    lins = [(n.rsplit(".", 1)[-1], m) for n, m in model.named_modules() if isinstance(m, HIPQuantLinear) and id(m) not in owq_inner]
    names = {n for n, _ in lins}
    if not lins:
        return
    sib = {n for g in SIBLING_GROUPS for n in g}
    if group_siblings and names & sib and not any("_group" in m.__dict__ for n, m in lins if n in sib):
        warnings.warn("prepare_for_inference: q/k/v / gate/up siblings found but none could be grouped (group_sibling_linears matched "
                      "nothing): every projection runs as its own launch", RuntimeWarning, stacklevel=3)
    if fuse_mlp and {"gate_proj", "up_proj", "down_proj"} <= names and not any(isinstance(m, HIPLlamaMLP) for m in model.modules()):
        warnings.warn("prepare_for_inference: gate/up/down projections found but no MLP was fused (fuse_llama_mlps matched nothing: "
                      "no SiLU-gated, bias-free MLP of three HIPQuantLinear children)", RuntimeWarning, stacklevel=3)
    layers = [m for m in model.modules() if all(hasattr(m, k) for k in ("input_layernorm", "self_attn", "post_attention_layernorm", "mlp"))
              and any(isinstance(c, HIPQuantLinear) and id(c) not in owq_inner for c in m.modules())]
    if fuse_norms and layers and not any(isinstance(m, HIPRMSNorm) for m in model.modules()):
        warnings.warn("prepare_for_inference: decoder layers found but no RMSNorm was fused into its consumer (fuse_llama_norms matched "
                      "nothing: needs a grouped q/k/v, a fused MLP and a LlamaRMSNorm-class norm)", RuntimeWarning, stacklevel=3)
    if fuse_layers and layers and not any("forward" in m.__dict__ for m in layers):
        warnings.warn("prepare_for_inference: decoder layers found but none took the fused forward (fuse_llama_layers matched nothing: "
                      "the layer class is not transformers' LlamaDecoderLayer with the known forward signature); residual adds stay "
                      "separate launches", RuntimeWarning, stacklevel=3)


def load_reference_cache(state_dict, device="cuda"):
    """Import a backend cache written by the reference's CUDA build
    (patching.py:182-189 / 198-205).  Returns {module_prefix: HIPQuantLinear}.

    GPTQLinear entries: ``<p>.qweight`` int32, ``<p>.scales``/``<p>.zeros`` fp32;
    FT_QuantLinear entries: ``<p>.qweight`` int16, ``<p>.scales``/``<p>.scaled_zeros`` fp16."""
    out = {}
    prefixes = sorted({k[: -len(".qweight")] for k in state_dict if k.endswith(".qweight")})
    for p in prefixes:
        qw = state_dict[p + ".qweight"].to(device)
        bias = state_dict.get(p + ".bias")
        bias = None if bias is None else bias.to(device)
        if qw.dtype == torch.int16:
            out[p] = HIPQuantLinear.from_ft_buffers(qw, state_dict[p + ".scales"].to(device),
                                                    state_dict[p + ".scaled_zeros"].to(device), bias=bias, name=p.split(".")[-1])
        elif qw.dtype == torch.int32:
            scales = state_dict[p + ".scales"].to(device)
            k_over_g, n = scales.shape
            bits = qw.shape[0] * 32 // (k_over_g * 128)
            out[p] = HIPQuantLinear.from_gptq_buffers(qw, scales, state_dict[p + ".zeros"].to(device), bits, bias=bias,
                                                      name=p.split(".")[-1])
        else:
            raise ValueError(f"{p}.qweight: unexpected dtype {qw.dtype}")
    return out
