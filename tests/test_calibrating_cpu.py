"""patching._calibrating -- what quantize_model_gptq and quantize_model_awq start and end their block-by-block walk with -- on a stub model, no GPU:
a walk that fails in the middle of the model leaves ``config.use_cache`` as it found it, and bad samples are refused before anything is touched."""
import types

import pytest
import torch


class _Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.self_attn = torch.nn.Module()
        for name in ("q_proj", "k_proj", "v_proj", "o_proj"):
            setattr(self.self_attn, name, torch.nn.Linear(128, 128, bias=False))
        self.mlp = torch.nn.Module()
        for name, (k, n) in (("gate_proj", (128, 256)), ("up_proj", (128, 256)), ("down_proj", (256, 128))):
            setattr(self.mlp, name, torch.nn.Linear(k, n, bias=False))

    def forward(self, hidden_states, **kwargs):
        raise RuntimeError("the first block fails")


class _Stub(torch.nn.Module):
    def __init__(self, use_cache):
        super().__init__()
        self.config = types.SimpleNamespace(use_cache=use_cache)
        self.model = torch.nn.Module()
        self.model.embed_tokens = torch.nn.Embedding(16, 128)
        self.model.layers = torch.nn.ModuleList([_Block()])

    def forward(self, ids):
        x = self.model.embed_tokens(ids)
        for layer in self.model.layers:
            x = layer(x, use_cache=self.config.use_cache)
        return x


SAMPLES = [torch.zeros(1, 8, dtype=torch.long), torch.ones(1, 8, dtype=torch.long)]


@pytest.mark.parametrize("walk", ["quantize_model_gptq", "quantize_model_awq"])
@pytest.mark.parametrize("use_cache", [True, False])
def test_use_cache_is_put_back_when_a_block_raises(walk, use_cache):
    from amq_amd import patching
    model = _Stub(use_cache)
    with pytest.raises(RuntimeError, match="first block fails"):
        getattr(patching, walk)(model, 4, SAMPLES, device="cpu")
    assert model.config.use_cache is use_cache
    assert not model.model.layers[0]._forward_pre_hooks          # the hook that caught the block's inputs is gone too


def test_calibrating_yields_the_first_blocks_inputs_with_use_cache_off():
    from amq_amd import patching
    model = _Stub(True)
    with patching._calibrating(model, SAMPLES, "cpu") as (device, inps, kwargs, run):
        assert device == torch.device("cpu") and model.config.use_cache is False
        assert len(inps) == 2 and tuple(inps[0].shape) == (1, 8, 128) and kwargs == {"use_cache": False}
        assert torch.equal(inps[1], model.model.embed_tokens(SAMPLES[1]))
    assert model.config.use_cache is True


@pytest.mark.parametrize("samples", [[], [torch.zeros(8, dtype=torch.long)], [torch.zeros(1, 8, dtype=torch.long), torch.zeros(1, 9, dtype=torch.long)]])
def test_bad_samples_are_refused_before_the_model_is_touched(samples):
    from amq_amd import patching
    model = _Stub(True)
    with pytest.raises(ValueError, match="samples: expected token-id tensors"):
        patching.quantize_model_gptq(model, 4, samples, device="cpu")
    assert model.config.use_cache is True
