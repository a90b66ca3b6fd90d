"""Qwen3's per-head q / k RMSNorm, CPU side: the reference restatement pinned to transformers' own modules, the one summation tree in the three
thread layouts of the rotating kernels, the config mapping (head_dim a field of its own, q / o widths of heads * 128) and check_hf's decisions."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qknorm_ref as ref  # noqa: E402


def _tiny_qwen3(**over):
    transformers = pytest.importorskip("transformers")
    kw = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
              vocab_size=1000, max_position_embeddings=256, rms_norm_eps=1e-6, attn_implementation="eager", tie_word_embeddings=False)
    kw.update(over)
    torch.manual_seed(0)
    return transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**kw)).eval()


def test_reference_restates_hf_qwen3_attention():
    """the fp16 restatement == transformers' Qwen3Attention pieces on the CPU: q_norm(q_proj(x).view(.., 128)) then apply_rotary_pos_emb, within 1
    fp16 ulp (runs HF's modules and the helper only)"""
    from transformers.models.qwen3.modeling_qwen3 import apply_rotary_pos_emb
    model = _tiny_qwen3().to(torch.float16)
    attn = model.model.layers[0].self_attn
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        attn.q_norm.weight.copy_((1 + 0.2 * torch.randn(128, generator=g)).half())
        attn.k_norm.weight.copy_((1 + 0.2 * torch.randn(128, generator=g)).half())
        S = 7
        x = torch.randn(1, S, 256, generator=g).half()
        pos = torch.arange(3, 3 + S)[None]
        cos, sin = model.model.rotary_emb(x, pos)                     # [1, S, 128] fp16
        q_raw = attn.q_proj(x).view(1, S, -1, 128)
        k_raw = attn.k_proj(x).view(1, S, -1, 128)
        q, k = apply_rotary_pos_emb(attn.q_norm(q_raw).transpose(1, 2), attn.k_norm(k_raw).transpose(1, 2), cos, sin)
    assert q.dtype is torch.float16 and q.shape == (1, 4, S, 128) and k.shape == (1, 2, S, 128)
    for got, raw, gamma in ((q, q_raw, attn.q_norm.weight), (k, k_raw, attn.k_norm.weight)):
        for s in range(S):
            mine = ref.norm_rope_f16(raw[0, s], gamma, 1e-6, cos[0, s], sin[0, s])          # [heads, 128]
            hf = got[0, :, s]
            ulp = torch.maximum(hf.abs(), mine.abs()).float().clamp_min(2.0 ** -14)
            ulp = 2.0 ** (torch.floor(torch.log2(ulp)) - 10)
            assert bool(((hf.float() - mine.float()).abs() <= ulp).all())
            # and the fp64 form is the same function: within fp16 rounding of the chain (three roundings of O(1) values)
            f64 = ref.norm_rope_f64(raw[0, s], gamma, 1e-6, cos[0, s], sin[0, s])
            assert float((f64 - mine.double()).abs().max()) <= 4 * 2.0 ** -10 * float(f64.abs().max())


def test_one_summation_tree_in_every_thread_layout():
    """64 lanes x 1 pair, 8 threads x 8 pairs and 4 lanes x 16 pairs in fragment order add the same operands at every one of the 6 levels -- so
    the fp32 statistic has the same bits in every kernel (fp32 addition is commutative, not associative)"""
    want = ref.tree_statement()
    assert [len(l) for l in want.levels] == [32, 16, 8, 4, 2, 1]
    for name, t in (("wave64", ref.tree_wave64()), ("threads8", ref.tree_threads8()), ("fragments", ref.tree_fragments())):
        for level in range(6):
            assert t.levels[level] == want.levels[level], (name, level)
    # a different association (a running sum) is a different tree: the property is not vacuous
    seq = ref.Tree()
    acc = ref.leaves()[0]
    for i in range(1, 64):
        acc = seq.add(min(5, i.bit_length() - 1), acc, ref.leaves()[i])
    assert seq.levels[1] != want.levels[1]


def test_config_mapping_for_qwen3_shapes():
    from amq_amd import arch
    from amq_amd.checkpoint import runner_config
    # Qwen3-0.6B / 4B / 32B: hidden_size is not heads * 128 (1024 vs 16 * 128, 2560 vs 32 * 128, 5120 vs 64 * 128)
    for hidden, heads, kv, inter in ((1024, 16, 8, 3072), (2560, 32, 8, 9728), (5120, 64, 8, 25600), (4096, 32, 8, 12288)):
        hf = dict(model_type="qwen3", hidden_size=hidden, intermediate_size=inter, num_hidden_layers=3, num_attention_heads=heads,
                  num_key_value_heads=kv, head_dim=128, vocab_size=151936, rms_norm_eps=1e-6, rope_theta=1000000.0)
        c = runner_config(hf)
        assert c["head_dim"] == 128 and c["qk_norm"] is True and c["hidden_size"] == hidden
        ls = c["linear_shape"]
        assert ls["self_attn.q_proj"] == [heads * 128, hidden] and ls["self_attn.o_proj"] == [hidden, heads * 128]
        assert ls["self_attn.k_proj"] == [kv * 128, hidden] == ls["self_attn.v_proj"]
        assert ls["mlp.gate_proj"] == [inter, hidden] and ls["mlp.down_proj"] == [hidden, inter]
        assert c["model_numel"] == 3 * sum(n * k for n, k in ls.values())
        assert c["rms_norm_eps"] == 1e-6 and c["rope_theta"] == 1000000.0
    # head_dim other than 128 stays refused
    with pytest.raises(ValueError, match="head_dim"):
        runner_config(dict(hf, head_dim=64))
    q8 = arch.MODEL_CONFIGS["Qwen3-8B"]
    assert (q8["n_block"], q8["hidden_size"], q8["intermediate_size"], q8["num_heads"], q8["num_kv_heads"], q8["vocab_size"]) == \
        (36, 4096, 12288, 32, 8, 151936)
    assert q8["qk_norm"] is True and q8["head_dim"] == 128 and not q8.get("qkv_bias")
    # every dense size: blocks, hidden, intermediate, heads (8 kv heads, head_dim 128, vocab 151936 throughout) as in the published configs
    sizes = {"0.6B": (28, 1024, 3072, 16), "1.7B": (28, 2048, 6144, 16), "4B": (36, 2560, 9728, 32), "8B": (36, 4096, 12288, 32),
             "14B": (40, 5120, 17408, 40), "32B": (64, 5120, 25600, 64)}
    assert sorted(n for n in arch.MODEL_CONFIGS if n.startswith("Qwen3-")) == sorted("Qwen3-" + s for s in sizes)
    for size, (blocks, hidden, inter, heads) in sizes.items():
        c = arch.MODEL_CONFIGS["Qwen3-" + size]
        hf = dict(model_type="qwen3", hidden_size=hidden, intermediate_size=inter, num_hidden_layers=blocks, num_attention_heads=heads,
                  num_key_value_heads=8, head_dim=128, vocab_size=151936, rms_norm_eps=1e-6, rope_theta=1000000.0)
        assert c == runner_config(hf)
        assert c["linear_shape"]["self_attn.q_proj"] == [heads * 128, hidden] and c["n_block"] == blocks
    tiny = arch.MODEL_CONFIGS["tiny-qwen3-test"]
    assert tiny["linear_shape"]["self_attn.q_proj"] == [512, 256] and tiny["linear_shape"]["self_attn.o_proj"] == [256, 512] and tiny["qk_norm"]
    # the existing families: no flag, square q / o, and what runner_config gives a llama config is what it gave before
    for name, c in arch.MODEL_CONFIGS.items():
        if "wen3" in name:
            continue
        H = c["hidden_size"]
        assert not c.get("qk_norm") and c["linear_shape"]["self_attn.q_proj"] == [H, H] == c["linear_shape"]["self_attn.o_proj"]
        assert c["head_dim"] == H // c["num_heads"]
    c = runner_config(dict(model_type="llama", hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
                           vocab_size=32000))
    want = dict(arch.MODEL_CONFIGS["Llama-2-7b-hf"], rms_norm_eps=1e-5, rope_theta=10000.0)
    assert c == want


def test_step_plan_unchanged_without_a_q_width():
    """the defaulted ``rows_q`` changes nothing for a model whose q / o widths are hidden_size (every existing family), and bounds the sums form by
    o_proj's own row limit where they are not"""
    from amq_amd.llama import NORM_FROM_SUMS, step_plan
    for H, I in ((4096, 11008), (5120, 13824), (8192, 28672), (3584, 18944), (256, 512)):
        for R in range(1, 9):
            for rows_h in (4, 8):
                base = step_plan(R, H, I, False, rows_h, 8, 8)
                assert step_plan(R, H, I, False, rows_h, 8, 8, rows_q=None) == base == step_plan(R, H, I, False, rows_h, 8, 8, rows_q=rows_h)
    assert step_plan(6, 5120, 25600, False, 8, 8, 8, rows_q=8).norm == NORM_FROM_SUMS
    assert step_plan(6, 5120, 25600, False, 8, 8, 8, rows_q=4).norm != NORM_FROM_SUMS


def _faked(model):
    """the decoder's q_proj as the swapped model has it, without a GPU: check_hf looks at the module's type only"""
    from amq_amd.quant_linear import HIPQuantLinear
    for layer in model.model.layers:
        lin = layer.self_attn.q_proj
        layer.self_attn.q_proj = HIPQuantLinear(4, 128, lin.in_features, lin.out_features, bias=None)
    return model


def _as_type(model, model_type):
    """the same object announcing another model_type (to_dict reads the class attribute)"""
    d = dict(model.config.to_dict(), model_type=model_type)
    model.config.to_dict = lambda: dict(d)


def test_check_hf_accepts_qwen3_and_keeps_refusing_the_rest():
    from amq_amd.llama import QuantLlama
    assert "qwen3" in QuantLlama.HF_MODEL_TYPES and "qwen3_moe" not in QuantLlama.HF_MODEL_TYPES
    model = _faked(_tiny_qwen3())
    cfg, rope = QuantLlama.check_hf(model, max_seq=128)              # (the parent commit: ValueError "per-head q / k norms are not part ...")
    assert cfg["qk_norm"] is True and cfg["head_dim"] == 128 and rope is None
    assert cfg["linear_shape"]["self_attn.q_proj"] == [512, 256] and cfg["linear_shape"]["self_attn.o_proj"] == [256, 512]
    # a norm on only one of q / k
    one = _faked(_tiny_qwen3())
    del one.model.layers[1].self_attn.k_norm
    with pytest.raises(ValueError, match="only one of q / k"):
        QuantLlama.check_hf(one)
    # not an RMSNorm over a head / another eps
    ln = _faked(_tiny_qwen3())
    ln.model.layers[0].self_attn.q_norm = torch.nn.LayerNorm(128)
    with pytest.raises(ValueError, match="RMSNorm"):
        QuantLlama.check_hf(ln)
    wide = _faked(_tiny_qwen3())
    wide.model.layers[0].self_attn.k_norm.weight = torch.nn.Parameter(torch.ones(256))
    with pytest.raises(ValueError, match="width 256"):
        QuantLlama.check_hf(wide)
    eps = _faked(_tiny_qwen3())
    eps.model.layers[0].self_attn.q_norm.variance_epsilon = 1e-5
    with pytest.raises(ValueError, match="rms_norm_eps"):
        QuantLlama.check_hf(eps)
    # the mixture-of-experts family is another block
    moe = _faked(_tiny_qwen3())
    _as_type(moe, "qwen3_moe")
    with pytest.raises(ValueError, match="qwen3_moe"):
        QuantLlama.check_hf(moe)
    # q / k norms on a model of another family stay refused
    other = _faked(_tiny_qwen3())
    _as_type(other, "llama")
    with pytest.raises(ValueError, match="q / k norms"):
        QuantLlama.check_hf(other)
    # a live sliding window beyond max_seq
    sw = _faked(_tiny_qwen3(sliding_window=64, use_sliding_window=True, max_window_layers=0))
    with pytest.raises(ValueError, match="sliding window"):
        QuantLlama.check_hf(sw, max_seq=128)
    QuantLlama.check_hf(sw, max_seq=64)


def test_ops_refuse_a_bad_norm_argument():
    """one norm without the other and a wrong shape / dtype are refused by the wrapper before any launch (no GPU needed: the check comes first)"""
    from amq_amd import ops
    g = torch.ones(128, dtype=torch.float16)
    cpu = torch.device("cpu")
    assert ops._qk_norm(None, None, 1e-6, cpu) is None
    with pytest.raises(ValueError, match="go together"):
        ops._qk_norm(g, None, 1e-6, cpu)
    with pytest.raises(ValueError, match="go together"):
        ops._qk_norm(None, g, 1e-6, cpu)
    with pytest.raises(ValueError, match="128 elements"):
        ops._qk_norm(torch.ones(256, dtype=torch.float16), g, 1e-6, cpu)
    with pytest.raises(ValueError, match="128 elements"):
        ops._qk_norm(g.float(), g, 1e-6, cpu)
    with pytest.raises(ValueError, match="128 elements"):
        ops._qk_norm(torch.ones(256, dtype=torch.float16)[::2], g, 1e-6, cpu)
    with pytest.raises(ValueError, match=r"must be in GPU memory.*it is on cpu"):
        ops._qk_norm(g, g, 1e-6, cpu)                                 # (the kernels read device memory)
