"""eval_ppl / eval_loss -- the two metrics the reference's search scores a candidate arch with (amq/utils/eval.py:22-75), on the deployed model.

``eval_loss`` is the search objective: the Jensen-Shannon divergence between the quantized model's logits and the dense model's (amq/utils/loss.py);
``eval_ppl`` is the reported quality.  Both have the reference's signatures and its arithmetic, window by window; what differs is where the work
happens: a window goes through ``QuantLlama.score_rows`` -- one prompt pass over the packed kernels, then per-row reductions on the device over
pieces of the logits (ops.logit_nll / ops.logit_jsd) -- so the ``[S, vocab]`` logits of a window are never materialised, in fp16 or fp32.  The per-row
values stay on the device, are summed there in fp64, and one number is read back per call.

The caller brings the token windows (the reference's ``loader``: an iterable of integer tensors ``[B, S]``) and, for ``eval_loss``, the dense model's
logits (the reference's ``get_logits``: indexable by window, entry i = ``[S, vocab]`` or ``[B, S, vocab]``, fp16 or fp32, device or host).  Dataset
loaders, the search and its proxies are not part of this package.
"""
import torch

from . import hf_fast
from .llama import QuantLlama


def _runner(model, need):
    """the runner that scores for ``model``: a QuantLlama / DenseLlama itself, or -- for an HF object prepared with
    ``prepare_for_inference(backend='hip')`` -- one bound over its buffers by QuantLlama.from_hf, kept beside hf_fast's runners (rebuilt when a
    window outgrows it or the model's linears were replaced)"""
    if isinstance(model, QuantLlama):
        return model
    if not (hasattr(model, "lm_head") and hasattr(getattr(model, "model", None), "layers")):
        raise TypeError("expected a QuantLlama / DenseLlama runner or a Llama-family causal LM prepared with prepare_for_inference(backend='hip')")
    if need > hf_fast._limit(model):
        raise ValueError(f"windows of {need} tokens exceed the model's max_position_embeddings ({hf_fast._limit(model)})")
    return hf_fast._bound(model, "score", need)[0]


def _gathered(accelerator, values):
    """the reference hands its per-window values to ``accelerator.gather_for_metrics``; an accelerator without that method (or None) is ignored"""
    gather = getattr(accelerator, "gather_for_metrics", None)
    if gather is not None:
        values = gather(values)
    return torch.stack(list(values)).flatten()


def window_value(rows, seqlen):
    """what the reference appends per window: the mean of the window's B * (S - 1) row values times ``seqlen * B`` (fp64, on the rows' device)"""
    return rows.double().mean() * float(seqlen * rows.shape[0])


@torch.inference_mode()
def eval_ppl(model, accelerator=None, loader=(), seqlen=2048):
    """Perplexity as the reference computes it (eval.py:50-75): per window the MEAN next-token NLL over its B * (S - 1) scored rows, times
    ``seqlen * B``; then exp(sum / (n_windows * seqlen)).  The mean over S - 1 rows is scaled by ``seqlen``, not by S - 1: that is the reference's
    arithmetic (its published numbers carry it), and it is kept.  Returns a Python float; one read-back."""
    values = []
    for inputs in loader:
        values.append(window_value(_runner(model, inputs.shape[-1]).score_rows(inputs), seqlen))
    if not values:
        raise ValueError("eval_ppl: the loader gave no window")
    values = _gathered(accelerator, values)
    return float(torch.exp(values.sum() / (values.numel() * seqlen)).item())


@torch.inference_mode()
def eval_loss(model, accelerator=None, loader=(), dense_logits_list=None, seqlen=2048):
    """The search objective as the reference computes it (eval.py:22-46): per window the JSD between this model's logits and
    ``dense_logits_list[i]`` averaged over the window's B * (S - 1) rows ('batchmean'; the last row is dropped on both sides), times
    ``seqlen * B``; then sum / (n_windows * seqlen).  Returns a Python float; one read-back."""
    if dense_logits_list is None:
        raise ValueError("eval_loss: dense_logits_list (the dense model's logits per window) is required")
    values = []
    for i, inputs in enumerate(loader):
        _, jsd = _runner(model, inputs.shape[-1]).score_rows(inputs, dense_logits=dense_logits_list[i])
        values.append(window_value(jsd, seqlen))
    if not values:
        raise ValueError("eval_loss: the loader gave no window")
    values = _gathered(accelerator, values)
    return float((values.sum() / (values.numel() * seqlen)).item())
