"""convert_model_to_hip -- the reference's ``use_ft`` call surface on the prepared HF object itself.

With ``--use_ft`` the reference patches the model it hands to its harness: ``convert_model_to_ft(model)`` replaces the Llama forwards so that
``model(input_ids, start_pos=..., use_cache=False)`` runs the static-cache fast step (kernel/monkeypatch/ftllama_modeling.py:427-492, 569-580) and
``replace_generate_functions()`` patches ``GenerationMixin._sample`` so that the caller's own ``model.generate(...)`` drives it
(ftllama_generate.py:613-622); the harness then calls exactly those two things (amq/utils/speed.py:31-36, 65, 82).

Here the fast step is the hipGraph runner (llama.QuantLlama).  ``convert_model_to_hip(model)`` binds one lazily over the swapped model's own
buffers (QuantLlama.from_hf: no weight copies; Llama 2 / 3.x, Mistral, Qwen2.5 and Qwen3 dense) and gives THIS model instance

  * ``model(input_ids, start_pos=p, use_cache=False)`` -- batch 1..8, any prompt length that fits the cache: the runner's prompt pass (captured per
    (length, start_pos)) or, for one new token at the runner's current position, the captured token step.  Returns a ``CausalLMOutputWithPast``
    whose ``logits`` are fp32 ``[B, S, vocab]`` for every input row, as HF's forward does (``.start_pos`` = the next position, as the
    reference's output carries);
  * ``model.generate(ids, min_new_tokens=n, max_new_tokens=n, do_sample=False, num_beams=1, attention_mask=all ones)`` -- greedy, fixed length,
    batch 1..8: prefill + n - 1 graph replays without a host sync in between; returns ``[B, S + n]`` ids like HF.

With ``convert_model_to_hip(model, sampling=True)`` (opt-in; the default routing above is unchanged) ``generate`` additionally serves, on the runner,

  * ``do_sample=True`` with ``temperature`` / ``top_k`` / ``top_p`` (call arguments, else ``generation_config``, else HF's defaults: top_k = 50),
    one beam, batch 1..8: the sampled tail of the captured step (amq_decode_tail_sample_f16).  The seed of a call is one ``torch.randint`` from
    torch's global CPU generator, so ``torch.manual_seed(s)`` before ``generate`` reproduces a call; the tokens are NOT ``torch.multinomial``'s
    (a counter-based generator of (seed, draw, sequence); the kept set is HF's warpers' except that a tie class at the top-p boundary is kept whole);
  * ``max_new_tokens`` without an equal ``min_new_tokens``, greedy or sampled: a sequence stops at its first ``eos_token_id`` (int or list, at most
    8) and is padded with ``pad_token_id`` from there on, the call returns at the longest sequence's length as HF's does; ``min_new_tokens = m``
    keeps the EOS ids suppressed for the first m tokens.

With ``convert_model_to_hip(model, padded=True)`` (opt-in beside ``sampling``; the default routing is unchanged) ``generate`` also accepts the
standard way to batch prompts of unequal length -- ``tokenizer(prompts, padding=True, padding_side="left")`` then ``model.generate(**enc)``: an
``attention_mask`` whose every row is ``0...0 1...1`` with at least one 1.  HF gives such a row the position ids ``cumsum(mask) - 1`` and masks the
pad keys, so each row decodes as if it were alone; here each row is stored compactly from cache row 0 and decoded at a position of its own
(``left_padded_to_right`` -> ``QuantLlama(ragged=True).generate(ids, n, lengths=...)``; such runners are cached under ``("ragged", B)``).  The
call returns ``cat([input_ids, new], 1)`` with the caller's left-padded ids untouched, as HF does.  Greedy fixed-length calls always; sampled and
open-ended ones with ``sampling=True`` as well.

With ``convert_model_to_hip(model, lookup=True)`` (opt-in as well) ``generate(ids, prompt_lookup_num_tokens=k, max_matching_ngram_size=g,
do_sample=False, num_beams=1, ...)`` for ONE sequence, 1 <= k <= 7 and 1 <= g <= 4 (HF's default 2 when absent) runs prompt-lookup speculative decoding
on the runner (``QuantLlama(lookup=k, ngram_max=g)``, cached under ``("lookup", k)``; g is one word of its device block): every step verifies k continuations guessed from the
sequence's own history in one pass of the weights.  The tokens are the greedy decode's whatever is guessed; the guesses follow the MOST RECENT earlier
occurrence of the last g .. 1 tokens (HF takes the earliest: only the acceptance rate differs).  ``lookup_request`` is the routing predicate.
With BOTH ``lookup=True`` and ``sampling=True`` the same call with ``do_sample=True`` (and ``temperature`` / ``top_k`` / ``top_p``) is served as
well, fixed-length or up to the first EOS id: every row's token is drawn, a guess is accepted while it equals the draw of the row in front of it --
what transformers' own prompt-lookup loop does under ``do_sample`` -- and the token at index i is always drawn with draw counter i, so the output
is distributed as plain sampled decoding's whatever is guessed (one runner per k serves greedy and sampled calls; the seed comes from torch's
global CPU generator as for plain sampled calls).  With either flag off such a call goes to HF.

With ``convert_model_to_hip(model, scoring=True)`` (opt-in as well) ``model(input_ids, start_pos=0, labels=lab, use_cache=False)`` stays on the fast
path and returns ``loss`` as well: HF's causal-LM loss -- the mean cross-entropy of row t against ``lab[:, t + 1]``, labels of -100 ignored -- formed
by ops.logit_nll on the runner's rows of logits (one launch; no fp32 copy of the logits goes into it).  ``logits`` is returned as without labels.
(``amq_amd.evaluate`` scores whole windows without materialising their logits at all.)

Anything else -- sampling and open-ended calls without that flag, ``labels`` without ``scoring=True`` or with ``start_pos`` other than 0, a padded mask without ``padded=True``, right padding, an all-zero mask row, ``min_p`` / ``typical_p`` / ``epsilon_cutoff`` / ``eta_cutoff``, beams, an attention mask with holes, ``past_key_values``, ``labels``, ``inputs_embeds``, hidden-state / attention outputs,
stopping criteria, streamers, more than 8 sequences, a call without ``start_pos`` -- falls through to the model's original ``forward`` / ``generate``
(HF's own, over the fused modules).  ``state_dict`` / ``deepcopy`` / ``.to()`` are untouched: the runners live outside the module, keyed weakly by it.
"""
import types
import weakref

import torch

try:
    from transformers.modeling_outputs import CausalLMOutputWithPast
except Exception:                                   # (transformers is needed only once a model is converted)
    CausalLMOutputWithPast = None

_RUNNERS = weakref.WeakKeyDictionary()      # model -> {batch: QuantLlama, ("ragged", batch): QuantLlama(ragged=True)}
_BUCKETS = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
# generation_config fields that make HF add a logits processor / warper / constraint to a greedy run: any of them set -> HF's own generate
_GC_PROCESSORS = ("repetition_penalty", "encoder_repetition_penalty", "no_repeat_ngram_size", "encoder_no_repeat_ngram_size", "bad_words_ids",
                  "force_words_ids", "constraints", "forced_bos_token_id", "forced_eos_token_id", "exponential_decay_length_penalty", "suppress_tokens",
                  "begin_suppress_tokens", "sequence_bias", "guidance_scale", "watermarking_config", "renormalize_logits", "remove_invalid_values",
                  "penalty_alpha", "dola_layers", "prompt_lookup_num_tokens", "num_beam_groups", "diversity_penalty")
# ... and the warpers the runner's sampled tail does not apply (temperature, top_k and top_p it does)
_GC_WARPERS = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "top_h")
MAX_BATCH = 8
LOOKUP_MAX_DRAFTS, LOOKUP_MAX_NGRAM = 7, 4
# what a generate call routed to the lookup runner may carry besides the two lookup arguments
_LOOKUP_KWARGS = ("input_ids", "max_new_tokens", "min_new_tokens", "do_sample", "num_beams", "attention_mask", "eos_token_id", "pad_token_id", "use_cache",
                  "return_dict_in_generate", "output_scores", "output_logits", "output_attentions", "output_hidden_states")


def lookup_request(kwargs, batch, enabled=True, sampling=False):
    """The routing predicate of prompt-lookup calls, a pure host function of the call's keyword arguments: -> (k, g) = (drafts per step, longest
    suffix looked up) when ``generate(**kwargs)`` on ``batch`` sequences is a call the lookup runner serves, else None (HF's own generate).
    Served: ``convert_model_to_hip(model, lookup=True)`` (``enabled``), one sequence, ``prompt_lookup_num_tokens`` = 1 .. 7 (an int),
    ``max_matching_ngram_size`` = 1 .. 4 (HF's default 2 when absent or None), greedy (``do_sample`` false), one beam, and no argument the
    runner does not know.  ``sampling`` (``convert_model_to_hip(model, lookup=True, sampling=True)``): a ``do_sample=True`` call is served as
    well and may carry ``temperature`` / ``top_k`` / ``top_p``."""
    if not enabled or batch != 1:
        return None
    k = kwargs.get("prompt_lookup_num_tokens")
    g = kwargs.get("max_matching_ngram_size")
    g = 2 if g is None else g
    if isinstance(k, bool) or isinstance(g, bool) or not isinstance(k, int) or not isinstance(g, int):
        return None
    if not 1 <= k <= LOOKUP_MAX_DRAFTS or not 1 <= g <= LOOKUP_MAX_NGRAM:
        return None
    if (kwargs.get("do_sample") not in (False, None) and not sampling) or kwargs.get("num_beams") not in (1, None):
        return None
    known = _LOOKUP_KWARGS + ("prompt_lookup_num_tokens", "max_matching_ngram_size") + (("temperature", "top_k", "top_p") if sampling else ())
    if any(key not in known for key in kwargs):
        return None
    return k, g


def _bucket(n, limit):
    for b in _BUCKETS:
        if n <= b:
            return min(b, max(limit, n))
    return n


def _limit(model):
    return int(getattr(model.config, "max_position_embeddings", 1 << 30) or (1 << 30))


def _bound(model, key, need, **build):
    """the runner kept under ``key`` with room for ``need`` positions, built on first use (``build``: from_hf's arguments) and rebuilt when a sequence
    outgrows it or the model's weights are no longer the ones it reads (the attention launch is chosen by the cache's size, so the cache is not
    made larger than asked for) -> (runner, the one it replaced or None)"""
    from .llama import QuantLlama
    per = _RUNNERS.setdefault(model, {})
    old = per.get(key)
    if old is not None and old.max_seq >= need and _same_weights(old, model):
        return old, None
    per[key] = QuantLlama.from_hf(model, max_seq=_bucket(need, _limit(model)), **build, **_lm_head_build(model))
    return per[key], old


def _lm_head_build(model):
    """from_hf's lm_head arguments: nothing for the fp16 lm_head; convert_model_to_hip(model, lm_head_bits=8 / 4): the bits and the ONE packed
    lm_head kept per converted model -- quantized on first use, shared by every runner built or rebuilt for it (growth, batch sizes, ragged,
    lookup), quantized again only when the module's weight is no longer the tensor it was made from"""
    from .llama import QuantLlama
    bits = model.__dict__.get("_amq_lm_head_bits", 16)
    if bits == 16:
        return {}
    w = model.lm_head.weight
    kept = model.__dict__.get("_amq_lm_head_packed")
    if kept is None or kept[0] != (bits, w.data_ptr(), w._version):
        kept = model.__dict__["_amq_lm_head_packed"] = ((bits, w.data_ptr(), w._version), QuantLlama.pack_lm_head(w.detach().to(torch.float16), bits))
    return dict(lm_head_bits=bits, lm_head_packed=kept[1])


def _lookup_runner(model, need, k, g):
    """the lookup runner for ``k`` drafts per step with room for ``need`` positions (every call starts with a prompt pass: a rebuilt one carries
    nothing over), looking up suffixes of up to ``g`` tokens -- one word of the runner's device block, so every g shares the runner of its k.
    None when ``need`` (prompt + new tokens + the k draft rows) passes the model's max_position_embeddings: the caller falls through to HF."""
    if need > _limit(model):
        return None
    r, _ = _bound(model, ("lookup", k), need, lookup=k, ngram_max=g, lookup_sampling=True)      # (one runner serves greedy and sampled calls)
    r.set_ngram_max(g)
    return r


def _runner(model, batch, need, ragged=False):
    """the runner for ``batch`` sequences with room for ``need`` positions; a rebuilt one carries the cache contents over.  ``ragged``: the runner
    with a position per sequence (left-padded generate calls), kept under a key of its own; every call on it starts with a prompt pass, so a rebuilt
    one carries nothing over."""
    if need > _limit(model):
        raise ValueError(f"{need} positions exceed the model's max_position_embeddings ({_limit(model)})")
    # (convert_model_to_hip(model, kv_bits=8): never together with padded / lookup)
    r, old = _bound(model, ("ragged", batch) if ragged else batch, need, batch=batch, ragged=ragged, kv_bits=model.__dict__.get("_amq_kv_bits", 16))
    if ragged:
        return r
    r.all_logits = True
    if old is not None and _same_weights(old, model) and old.host_pos > 0:
        for nb, ob in zip(r.blocks, old.blocks):
            for key in r.cache_keys:                # (an 8-bit cache: codes and scales)
                nb[key][:, :, :old.host_pos].copy_(ob[key][:, :, :old.host_pos])
        r.set_pos(old.host_pos)
        r.set_token(old.token)
    return r


def _same_weights(r, model):
    """the runner still reads the buffers the modules own (a linear replaced or moved since -- the reference's driver setattr's linears between
    models, amq_speed_benchmark.py:231-251 -- means a new runner)"""
    layer = model.model.layers[0]
    q = layer.self_attn.q_proj
    q = getattr(q, "inner", q)                  # (an OWQ layer: its packed inner layer owns the buffer the runner shares)
    same = r.blocks[0]["self_attn.q_proj"].qn.data_ptr() == q.qweight.data_ptr() and r.nb == len(model.model.layers)
    if same and r.qk_norm:                      # Qwen3: the per-head norm weights are the modules' own tensors too (fp16 ones: no copy was made)
        for key, m in (("qn", getattr(layer.self_attn, "q_norm", None)), ("kn", getattr(layer.self_attn, "k_norm", None))):
            w = getattr(m, "weight", None)
            same = same and w is not None and (w.dtype is not torch.float16 or r.blocks[0][key].data_ptr() == w.data_ptr())
    return same


def _plain_ids(input_ids):
    return (isinstance(input_ids, torch.Tensor) and input_ids.dim() == 2 and input_ids.dtype in (torch.int64, torch.int32)
            and 1 <= input_ids.shape[0] <= MAX_BATCH and input_ids.shape[1] >= 1)


def _mask_is_full(mask, ids):
    if mask is None:
        return True
    return isinstance(mask, torch.Tensor) and mask.shape == ids.shape and bool(mask.ne(0).all())


def left_padded_to_right(mask, ids, fill=0):
    """A LEFT-padded batch as the ragged runner takes it.  mask, ids: [B, S]; every row of ``mask`` must be ``0...0 1...1`` with at least one 1
    (integer or bool values 0 / 1).  -> (ids RIGHT-padded: row b holds its L_b real tokens in columns 0 .. L_b - 1, ``fill`` behind them;
    lengths int64 [B]), or None for anything else (holes, right padding, an all-zero row, other values, a floating / additive mask).  A full mask
    gives the ids back with every length S.  Pure torch, any device."""
    if not (isinstance(mask, torch.Tensor) and isinstance(ids, torch.Tensor) and ids.dim() == 2 and mask.shape == ids.shape):
        return None
    if mask.dtype.is_floating_point or mask.dtype.is_complex:
        return None
    B, S = ids.shape
    if B < 1 or S < 1:
        return None
    m = mask.to(torch.int64)
    if bool(((m != 0) & (m != 1)).any()):
        return None
    lengths = m.sum(dim=1)
    cols = torch.arange(S, device=ids.device)[None, :]
    shift = (S - lengths)[:, None]
    if bool((lengths < 1).any()) or not bool((m == (cols >= shift).to(torch.int64)).all()):
        return None
    src = (cols + shift).clamp_(max=S - 1)
    right = torch.where(cols < lengths[:, None], ids.gather(1, src), torch.full_like(ids, int(fill)))
    return right, lengths


def _fast_forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, start_pos=None, inputs_embeds=None,
                  labels=None, use_cache=None, **kwargs):
    """``LlamaForCausalLM.forward`` with the reference's extra ``start_pos`` argument (ftllama_modeling.py:428-441)"""
    orig = self.__dict__["_amq_orig_forward"]
    extras = {k: v for k, v in kwargs.items() if v is not None and v is not False and not (k == "return_dict" and v is True)
              and not (k == "logits_to_keep" and v == 0)}
    # convert_model_to_hip(model, scoring=True): integer labels of the ids' shape on a pass from position 0 are served (loss below)
    scored = (labels is not None and self.__dict__.get("_amq_scoring", False) and start_pos is not None and int(start_pos) == 0
              and _plain_ids(input_ids) and isinstance(labels, torch.Tensor) and labels.shape == input_ids.shape and not labels.dtype.is_floating_point)
    if (start_pos is None or not _plain_ids(input_ids) or past_key_values is not None or inputs_embeds is not None or (labels is not None and not scored)
            or position_ids is not None or use_cache or extras or not input_ids.is_cuda or not _mask_is_full(attention_mask, input_ids)):
        if start_pos is not None:
            raise ValueError("model(..., start_pos=) serves input_ids [1..8, S] on the GPU with use_cache=False and nothing else "
                             "(no mask with holes, past_key_values, labels, inputs_embeds or extra outputs); drop start_pos for HF's own forward")
        return orig(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, past_key_values=past_key_values,
                    inputs_embeds=inputs_embeds, labels=labels, use_cache=use_cache, **kwargs)
    B, S = input_ids.shape
    start_pos = int(start_pos)
    # room for the tokens that usually follow (a rebuilt runner re-captures its step): twice the context, at most 1024 more, never past the model's limit
    limit = _limit(self)
    end = start_pos + S
    r = _runner(self, B, max(end, min(limit, max(end + 1, 2 * end if end <= 1024 else end + 1024))))
    ids = input_ids if B > 1 else input_ids[0]
    if S == 1 and start_pos == r.host_pos and start_pos > 0:
        r.set_token(input_ids.reshape(-1))
        r.decode_step()
        logits = r.logits.view(B, 1, r.vocab).float()
    else:
        r.prefill(ids, start_pos=start_pos)
        logits = r.logits_rows.float()
    loss = _shifted_ce(r.logits_rows, labels) if scored else None       # (scored: start_pos = 0, so the pass above was a prompt pass)
    out = CausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=None, hidden_states=None, attentions=None)
    out["start_pos"] = start_pos + S          # (the reference's output carries it: ftllama_modeling.py:486)
    return out


def _shifted_ce(rows, labels):
    """HF's causal-LM loss from fp16 logits ``rows`` [B, S, vocab] and ``labels`` [B, S]: mean over the rows t < S - 1 whose label labels[:, t + 1] is not
    -100 of lse(rows[:, t]) - rows[:, t, label] (ops.logit_nll gives 0 for an ignored row); NaN when every label is ignored, as HF's is"""
    from . import ops
    B, S, V = rows.shape
    lab = torch.full((B, S), -100, dtype=torch.int64, device=rows.device)
    lab[:, :S - 1] = labels[:, 1:].to(rows.device)
    nll, _, _ = ops.logit_nll(rows.reshape(B * S, V), lab.view(-1))
    return nll.double().sum().div(lab.ne(-100).sum()).float()


def _fast_generate(self, inputs=None, generation_config=None, logits_processor=None, stopping_criteria=None, prefix_allowed_tokens_fn=None,
                   synced_gpus=None, assistant_model=None, streamer=None, negative_prompt_ids=None, negative_prompt_attention_mask=None,
                   custom_generate=None, **kwargs):
    orig = self.__dict__["_amq_orig_generate"]

    def fall():
        return orig(inputs, generation_config=generation_config, logits_processor=logits_processor, stopping_criteria=stopping_criteria,
                    prefix_allowed_tokens_fn=prefix_allowed_tokens_fn, synced_gpus=synced_gpus, assistant_model=assistant_model, streamer=streamer,
                    negative_prompt_ids=negative_prompt_ids, negative_prompt_attention_mask=negative_prompt_attention_mask,
                    custom_generate=custom_generate, **kwargs)

    kw = dict(kwargs)
    ids = inputs if inputs is not None else kw.pop("input_ids", None)
    if inputs is not None and "input_ids" in kw:
        return fall()
    look = None
    if "prompt_lookup_num_tokens" in kw or "max_matching_ngram_size" in kw:
        if kw.get("prompt_lookup_num_tokens") is None:
            return fall()
        look = lookup_request(kwargs, ids.shape[0] if _plain_ids(ids) else 0, self.__dict__.get("_amq_lookup", False),
                              self.__dict__.get("_amq_sampling", False))
        if look is None:
            return fall()
        kw.pop("prompt_lookup_num_tokens", None)
        kw.pop("max_matching_ngram_size", None)
    gc = getattr(self, "generation_config", None)
    sampling = self.__dict__.get("_amq_sampling", False)       # convert_model_to_hip(model, sampling=True): sampled and open-ended calls served too
    padded = self.__dict__.get("_amq_padded", False)           # convert_model_to_hip(model, padded=True): left-padded batches served too
    n = kw.pop("max_new_tokens", None)
    nmin = kw.pop("min_new_tokens", None)
    do_sample = kw.pop("do_sample", getattr(gc, "do_sample", False)) not in (False, None)
    one_beam = kw.pop("num_beams", getattr(gc, "num_beams", 1)) in (1, None)
    mask = kw.pop("attention_mask", None)
    eos = kw.pop("eos_token_id", getattr(gc, "eos_token_id", None))
    pad = kw.pop("pad_token_id", None)                         # (fixed-length decoding never pads)
    warp = {}
    if sampling:                                                # call arguments, else generation_config, else HF's defaults (top_k = 50)
        for k, default in (("temperature", 1.0), ("top_k", 50), ("top_p", 1.0)):
            v = kw.pop(k, None)
            v = getattr(gc, k, None) if v is None else v
            warp[k] = default if v is None else v
        if pad is None:
            pad = getattr(gc, "pad_token_id", None)
    for k in ("return_dict_in_generate", "output_scores", "output_logits", "output_attentions", "output_hidden_states", "use_cache"):
        if kw.get(k) in (None, False) or (k == "use_cache" and kw.get(k) is True):
            kw.pop(k, None)
    others = [generation_config, logits_processor, stopping_criteria, prefix_allowed_tokens_fn, assistant_model, streamer, negative_prompt_ids,
              negative_prompt_attention_mask, custom_generate]
    eos = [] if eos is None else ([int(e) for e in eos] if isinstance(eos, (list, tuple)) else [int(eos)])
    fixed = nmin == n
    if (kw or any(o is not None and (not hasattr(o, "__len__") or len(o)) for o in others) or synced_gpus or not one_beam or n is None
            or ((do_sample or not fixed) and not sampling and look is None)
            or not _plain_ids(ids) or not ids.is_cuda or int(n) < 1 or len(eos) > 8):
        return fall()
    compact = None                                              # (right-padded ids, lengths) of a left-padded batch
    if not _mask_is_full(mask, ids):
        compact = left_padded_to_right(mask, ids) if padded and isinstance(mask, torch.Tensor) and mask.device == ids.device else None
        if compact is None:
            return fall()
    # the model's own generation defaults must ask for nothing else (any other logits processor / warper HF would add changes the tokens)
    if gc is not None and any(getattr(gc, k, None) not in (None, False, 0, 1, 1.0, [], ()) for k in _GC_PROCESSORS + (_GC_WARPERS if do_sample else ())):
        return fall()
    B, S = ids.shape
    n = int(n)
    nmin = 0 if nmin is None else int(nmin)
    if do_sample and warp and not (float(warp["temperature"]) > 0.0 and int(warp["top_k"]) >= 0 and 0.0 < float(warp["top_p"]) <= 1.0):
        return fall()                                           # (HF raises its own error for these)
    if nmin > n or (not fixed and pad is not None and not 0 <= int(pad) < int(self.config.vocab_size)):
        return fall()
    if look is not None and do_sample and not sampling:         # (the model's generation_config samples, sampling=True was not asked for: HF's own generate)
        return fall()
    if look is not None:
        # prompt-lookup speculative decoding: one sequence; fixed length (the EOS ids never chosen, as above) or up to the first EOS id; greedy, or
        # -- sampling=True -- every row's token drawn and a draft accepted while it equals the draw in front of it, as HF's own loop does
        if compact is not None:
            return fall()
        r = _lookup_runner(self, S + n + look[0], *look)
        if r is None:                                           # (the draft rows would pass max_position_embeddings: HF serves the call)
            return fall()
        try:
            if do_sample:                                       # (the seed: as for plain sampled calls below)
                r.set_sampling(float(warp["temperature"]), int(warp["top_k"]), float(warp["top_p"]), seed=int(torch.randint(0, 2 ** 62, (1,)).item()))
            r.set_suppressed(eos if fixed else ())
            r.set_eos(() if fixed else eos)
            new = r.generate(ids[0], n, stop_at_eos=not fixed, min_new_tokens=nmin)
        finally:
            r.set_sampling(None)
        return torch.cat([ids, new.view(1, -1).to(ids.dtype)], dim=1)
    r = _runner(self, B, S + n, ragged=compact is not None)
    if compact is not None:                                     # each row from cache row 0 at a position of its own; the caller's ids come back untouched
        prompt, gkw = compact[0], dict(lengths=compact[1].tolist())
    else:
        prompt, gkw = (ids if B > 1 else ids[0]), {}
    if not do_sample and fixed:
        # min_new_tokens = max_new_tokens: HF never lets an EOS id through (MinNewTokensLengthLogitsProcessor sets their logits to -inf on every step)
        r.set_suppressed(eos)
        new = r.generate(prompt, n, **gkw)
        return torch.cat([ids, new.view(B, n).to(ids.dtype)], dim=1)
    try:
        if do_sample:
            # one number from torch's global CPU generator per call: torch.manual_seed(s) before generate() makes the call reproducible, as under HF
            # (the tokens are not torch.multinomial's: the runner draws with its own counter-based generator)
            r.set_sampling(float(warp["temperature"]), int(warp["top_k"]), float(warp["top_p"]), seed=int(torch.randint(0, 2 ** 62, (1,)).item()))
        if fixed:
            r.set_suppressed(eos)
            new = r.generate(prompt, n, **gkw)
        else:
            # open-ended: a sequence stops at its first EOS id and is padded from there on (HF pads with eos[0] when no pad id is set)
            r.set_suppressed(())
            r.set_eos(eos, pad_id=int(pad) if pad is not None else (eos[0] if eos else 0))
            new = r.generate(prompt, n, stop_at_eos=True, min_new_tokens=nmin, **gkw)
    finally:
        r.set_sampling(None)                                    # (model(ids, start_pos=) steps of this runner stay greedy)
    return torch.cat([ids, new.view(B, -1).to(ids.dtype)], dim=1)


def convert_model_to_hip(model, sampling=False, padded=False, lookup=False, scoring=False, kv_bits=16, lm_head_bits=16):
    """convert_model_to_ft(model) + replace_generate_functions() (ftllama_modeling.py:569-580, ftllama_generate.py:613-622) for the HIP backend:
    call it on the model ``prepare_for_inference(model, backend='hip')`` returned (a Llama-family ``*ForCausalLM`` whose decoder linears are
    HIPQuantLinear modules on one GPU).  Patches THIS instance's ``forward`` and ``generate`` (see the module docstring); idempotent; returns the
    model.  ``sampling=True`` also routes ``generate(do_sample=True, temperature / top_k / top_p)`` and open-ended calls (EOS stop) to the runner;
    ``padded=True`` also routes ``generate`` calls whose ``attention_mask`` is LEFT padding (``padding_side="left"``) to a runner that decodes every
    row at a position of its own; ``lookup=True`` also routes ``generate(prompt_lookup_num_tokens=k, ...)`` calls for one sequence to a
    prompt-lookup speculative runner (``lookup_request``), greedy ones -- and with ``sampling=True`` as well ``do_sample=True`` ones; ``scoring=True`` keeps ``model(ids, start_pos=0, labels=..., use_cache=False)`` on the runner and
    returns HF's shifted cross-entropy as ``loss``; ``kv_bits=8``: the runners keep an 8-bit KV cache (int8 rows with a scale per row, DESIGN.md 3.13:
    ``generate`` greedy and sampled, one-row ``model(ids, start_pos=p)`` steps; a many-row call at ``start_pos`` > 0 raises; refused together with
    ``lookup=True`` / ``padded=True``); ``lm_head_bits=8`` / ``4``: the runners read a packed lm_head (QuantLlama(lm_head_bits=)),
    quantized once from ``model.lm_head.weight`` and shared by every runner of the model; the module itself keeps its fp16 weight, so HF's own
    forward and a reverted model are untouched.  Calling it again on a converted model only updates the flags.  ``revert_model_to_hf(model)`` undoes it."""
    if not (hasattr(model, "lm_head") and hasattr(getattr(model, "model", None), "layers")):
        raise TypeError("convert_model_to_hip expects a Llama-family causal LM (model.model.layers, model.lm_head)")
    from .llama import check_kv_bits, check_lm_head_bits
    check_kv_bits(kv_bits)
    if kv_bits == 8 and (lookup or padded):
        raise ValueError("kv_bits=8 is not offered together with " + ("lookup=True" if lookup else "padded=True") + ": the 8-bit attention kernel "
                         "runs one row per sequence at one position for the batch (QuantLlama(kv_bits=8))")
    check_lm_head_bits(lm_head_bits)
    if model.__dict__.get("_amq_kv_bits", kv_bits) != kv_bits or model.__dict__.get("_amq_lm_head_bits", 16) != lm_head_bits:
        _RUNNERS.pop(model, None)                               # runners hold a cache of the other format / another lm_head
        model.__dict__.pop("_amq_lm_head_packed", None)
    model.__dict__["_amq_kv_bits"] = int(kv_bits)
    if lm_head_bits == 16:
        model.__dict__.pop("_amq_lm_head_bits", None)
    else:
        model.__dict__["_amq_lm_head_bits"] = int(lm_head_bits)
    if "_amq_orig_forward" in model.__dict__:
        model.__dict__["_amq_sampling"] = bool(sampling)
        model.__dict__["_amq_padded"] = bool(padded)
        model.__dict__["_amq_lookup"] = bool(lookup)
        model.__dict__["_amq_scoring"] = bool(scoring)
        return model
    from .llama import QuantLlama
    QuantLlama.check_hf(model)                               # refuse now, with the reason, what the runner cannot serve
    model.__dict__["_amq_orig_forward"] = model.forward
    model.__dict__["_amq_orig_generate"] = model.generate
    model.__dict__["_amq_sampling"] = bool(sampling)
    model.__dict__["_amq_padded"] = bool(padded)
    model.__dict__["_amq_lookup"] = bool(lookup)
    model.__dict__["_amq_scoring"] = bool(scoring)
    model.forward = types.MethodType(_fast_forward, model)
    model.generate = types.MethodType(_fast_generate, model)
    return model


def revert_model_to_hf(model):
    for name in ("forward", "generate"):
        if "_amq_orig_" + name in model.__dict__:
            model.__dict__.pop(name, None)
            model.__dict__.pop("_amq_orig_" + name)
    model.__dict__.pop("_amq_sampling", None)
    model.__dict__.pop("_amq_padded", None)
    model.__dict__.pop("_amq_lookup", None)
    model.__dict__.pop("_amq_scoring", None)
    model.__dict__.pop("_amq_kv_bits", None)
    model.__dict__.pop("_amq_lm_head_bits", None)
    model.__dict__.pop("_amq_lm_head_packed", None)
    _RUNNERS.pop(model, None)
    return model


def replace_generate_functions():
    """The reference patches ``GenerationMixin`` globally (ftllama_generate.py:613-622) and its driver calls this right after
    ``convert_model_to_ft`` (amq_speed_benchmark.py:79-80).  Here ``convert_model_to_hip`` patches the one instance, so this is a no-op kept for
    scripts that make both calls."""
    return None
