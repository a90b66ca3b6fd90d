#!/usr/bin/env python3
"""Golden vectors for the AWQ quantizer, produced by the REAL reference (amq/quantization/awq_utils: auto_clip_layer_asym, auto_scale_block,
pseudo_quantize_tensor; zero_point=True) on the CPU, over fp32 tensors holding fp16 values -- data only; no reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_awq.py

``awqclip_64x256_g{128,64,32}.npz``, ``awqclip_stride.npz``, ``awqclip_edge.npz``, each holding
  W         fp16 [N, K]     the layer's weights
  X         fp16 [rows, K]  the activation rows (the GPTQ generator's ``calibration``: a 1/16 grid with hot channels)
  n_sample_token int32      what the reference was called with: it samples X[0 :: rows // n_sample_token]
  bits      int32 [3]       2, 3, 4
  group     int32
  max_b{bits}, min_b{bits}  fp32 [N, K / group]  the reference's best_max / best_min
  Q_b{bits} fp32 [N, K]     the reference's pseudo_quantize_tensor of W (no scale, no bounds)
The stride file has 200 rows at n_sample_token = 64: stride 3, 67 sampled rows (not a multiple of 16).  The edge file (T = 1; group 128) holds in
group 0 a constant group (row 0: the 1e-5 floor), an all-positive group (row 1: z clamps to 0), an all-negative group (row 2), a group whose
range makes fp16(s) subnormal at every bit-width (row 3), and an all-zero X over group 1 (every error is 0: step 0 must win).

``awqscale_block.npz``: a one-layer Llama block (hidden 128, intermediate 256, 2 heads, MHA), its weights fp16, x fp16 [4, 32, 128] with hot
channels planted through the input norm's weight, group 64, mixed bits per linear; the reference's four scale vectors (``scale_{0..3}``) and
each search's 20 losses (``loss_{0..3}``), recomputed here from the outputs its loop produced (forward hooks on the inspected modules: the same
``(org - out).float().pow(2).mean().item()`` over the same tensors).  ``auto_clip_layer_asym`` calls torch.cuda.empty_cache(): stubbed here.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import REF, HERE      # noqa: E402
from gen_golden_gptq import calibration      # noqa: E402

REF_AMQ = os.path.dirname(os.path.dirname(REF))
BITS = (2, 3, 4)
SCALE_BITS = {"self_attn.q_proj": 4, "self_attn.k_proj": 3, "self_attn.v_proj": 2, "self_attn.o_proj": 3, "mlp.gate_proj": 2, "mlp.up_proj": 4,
              "mlp.down_proj": 3}
SCALE_GROUP = 64


def clip_case(torch, auto_clip_layer_asym, pseudo_quantize_tensor, W, X, G, n_sample_token, path):
    out = {"W": W.numpy(), "X": X.numpy(), "n_sample_token": np.int32(n_sample_token), "bits": np.array(BITS, np.int32), "group": np.int32(G)}
    cfg = {"zero_point": True, "q_group_size": G}
    for bits in BITS:
        mx, mn = auto_clip_layer_asym(W.float(), X.float(), n_bit=bits, q_config=cfg, n_sample_token=n_sample_token)
        out[f"max_b{bits}"], out[f"min_b{bits}"] = mx.squeeze(-1).numpy(), mn.squeeze(-1).numpy()
        out[f"Q_b{bits}"] = pseudo_quantize_tensor(W.float(), n_bit=bits, **cfg).numpy()
    np.savez_compressed(path, **out)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")


def scale_case(torch, auto_scale_block, path):
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaDecoderLayer, LlamaRotaryEmbedding
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, vocab_size=64,
                      max_position_embeddings=64, rms_norm_eps=1e-5, attn_implementation="eager")
    torch.manual_seed(21)
    layer = LlamaDecoderLayer(cfg, 0).eval()
    g = torch.Generator().manual_seed(22)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(p.half().float())
        gamma = 1.0 + 0.1 * torch.randn(128, generator=g)
        gamma[torch.randperm(128, generator=g)[:4]] *= 10.0              # hot channels in front of q / k / v
        layer.input_layernorm.weight.copy_(gamma.half().float())
        x = torch.randn(4, 32, 128, generator=g).half().float()
        S = x.shape[1]
        cos, sin = LlamaRotaryEmbedding(cfg)(x, torch.arange(S).unsqueeze(0))
        mask = torch.full((S, S), torch.finfo(torch.float32).min).triu(1).reshape(1, 1, S, S)
        kwargs = {"position_embeddings": (cos, sin), "attention_mask": mask}
        weights = {k: v.clone() for k, v in layer.state_dict().items()}
        names = ("self_attn.q_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.down_proj")
        mods = {n: getattr(getattr(layer, n.split(".")[0]), n.split(".")[1]) for n in names}
        feat = {}
        hs = [mods[n].register_forward_hook(lambda m, i, o, n=n: feat.__setitem__(n, i[0].detach().clone())) for n in names]
        layer(x, **kwargs)
        for h in hs:
            h.remove()
        feat["self_attn.k_proj"] = feat["self_attn.v_proj"] = feat["self_attn.q_proj"]
        feat["mlp.up_proj"] = feat["mlp.gate_proj"]
        # the outputs of the four inspected modules, in call order (o_proj also runs inside self_attn, down_proj inside mlp: each search is the
        # module's last 21 calls at the time it ends -- the searches run one after the other)
        seen = {k: [] for k in ("self_attn", "o_proj", "mlp", "down_proj")}
        insp = {"self_attn": layer.self_attn, "o_proj": layer.self_attn.o_proj, "mlp": layer.mlp, "down_proj": layer.mlp.down_proj}
        hs = [m.register_forward_hook(lambda m, i, o, k=k: seen[k].append((o[0] if isinstance(o, tuple) else o).detach().clone()))
              for k, m in insp.items()]
        scales = auto_scale_block(layer, dict(kwargs), {"zero_point": True, "q_group_size": SCALE_GROUP}, feat, module_bit=dict(SCALE_BITS))
        for h in hs:
            h.remove()
    assert len(scales) == 4 and all(len(seen[k]) == n for k, n in (("self_attn", 21), ("o_proj", 42), ("mlp", 21), ("down_proj", 42)))
    out = {"x": x.half().numpy(), "group": np.int32(SCALE_GROUP), "cos": cos.numpy(), "sin": sin.numpy(),
           "linears": np.array(list(SCALE_BITS)), "linear_bits": np.array(list(SCALE_BITS.values()), np.int32)}
    for k, v in weights.items():
        out["w." + k] = v.half().numpy()
    for i, (k, (_, lnames, s)) in enumerate(zip(("self_attn", "o_proj", "mlp", "down_proj"), scales)):
        outs = seen[k][-21:]
        out[f"scale_{i}"] = s.numpy()
        out[f"loss_{i}"] = np.array([(outs[0] - o).float().pow(2).mean().item() for o in outs[1:]], np.float64)
        out[f"names_{i}"] = np.array(list(lnames))
    np.savez_compressed(path, **out)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF_AMQ)
    import torch
    torch.cuda.empty_cache = lambda *a, **k: None
    from quantization.awq_utils.auto_clip import auto_clip_layer_asym
    from quantization.awq_utils.auto_scale import auto_scale_block
    from quantization.awq_utils.quantizer import pseudo_quantize_tensor

    N, K = 64, 256
    for G, seed in ((128, 31), (64, 32), (32, 33)):
        g = torch.Generator().manual_seed(seed)
        W = (torch.randn(N, K, generator=g) * 0.02).half()
        X = calibration(torch, g, 256, K)
        clip_case(torch, auto_clip_layer_asym, pseudo_quantize_tensor, W, X, G, 256, f"{HERE}/awqclip_{N}x{K}_g{G}.npz")

    g = torch.Generator().manual_seed(34)
    W = (torch.randn(N, K, generator=g) * 0.02).half()
    X = calibration(torch, g, 200, K)
    clip_case(torch, auto_clip_layer_asym, pseudo_quantize_tensor, W, X, 128, 64, f"{HERE}/awqclip_stride.npz")

    g = torch.Generator().manual_seed(35)
    W = (torch.randn(N, K, generator=g) * 0.02).half()
    W[0, 0:128] = 0.0123
    W[1, 0:128] = W[1, 0:128].abs() + 0.004
    W[2, 0:128] = -W[2, 0:128].abs() - 0.004
    W[3, 0:128] = torch.tensor([0.0010, 0.0011]).half().repeat(64)
    X = calibration(torch, g, 1, K)
    X[:, 128:] = 0.0
    clip_case(torch, auto_clip_layer_asym, pseudo_quantize_tensor, W, X, 128, 1, f"{HERE}/awqclip_edge.npz")

    scale_case(torch, auto_scale_block, f"{HERE}/awqscale_block.npz")


if __name__ == "__main__":
    main()
