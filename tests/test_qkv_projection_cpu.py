"""The `hip_proj` switch of the context layers without a GPU: on CPU tensors it changes nothing, bit for bit, and
ops.qkv_projection refuses what it does not serve."""
import pytest
import torch

from featurematching_amd import ops, synth, transformer

FINE = {'d_model': 64, 'nhead': 8, 'layer_names': ['self', 'cross']}


def _run(module, inputs, grads, **kw):
    inputs = [t.detach().clone().requires_grad_(True) for t in inputs]
    outs = module(*inputs, **kw)
    outs = outs if isinstance(outs, tuple) else (outs,)
    torch.autograd.backward(list(outs), grads)
    return [o.detach() for o in outs] + [t.grad for t in inputs] + [p.grad for _, p in sorted(module.named_parameters())]


def test_encoder_layer_on_cpu_is_unchanged():
    torch.manual_seed(5)
    off = transformer.EncoderLayer(64, 8).train()
    on = transformer.EncoderLayer(64, 8, hip_proj=True).train()
    on.load_state_dict(off.state_dict())
    assert on.hip_proj and not off.hip_proj and list(on.state_dict()) == list(off.state_dict())
    x, src = torch.as_tensor(synth.normal(11, 1, (3, 25, 64))), torch.as_tensor(synth.normal(11, 2, (3, 49, 64)))
    g = torch.as_tensor(synth.normal(11, 3, (3, 25, 64)))
    for a, b in zip(_run(on, (x, src), [g]), _run(off, (x, src), [g])):
        assert torch.equal(a, b)


@pytest.mark.parametrize("masked", [False, True])
def test_fine_transformer_on_cpu_is_unchanged(masked):
    weights = {k: torch.as_tensor(v) for k, v in synth.transformer_weights(7, 64, 2).items()}
    off = transformer.LocalFeatureTransformer(FINE).train()
    on = transformer.LocalFeatureTransformer(FINE, hip_proj=True).train()
    off.load_state_dict(weights)
    on.load_state_dict(weights)
    assert on.hip_proj and not off.hip_proj
    assert all(layer.hip_proj for layer in on.layers) and not any(layer.hip_proj for layer in off.layers)
    assert list(on.state_dict()) == list(off.state_dict()) == list(weights)
    x0, x1, g0, g1 = (torch.as_tensor(synth.normal(12, i, (4, 49, 64))) for i in (1, 2, 3, 4))
    kw = {}
    if masked:
        mask0 = torch.ones(4, 49, dtype=torch.bool)
        mask0[1, 30:] = False
        kw = {'mask0': mask0}
    for a, b in zip(_run(on, (x0, x1), [g0, g1], **kw), _run(off, (x0, x1), [g0, g1], **kw)):
        assert a is not None and torch.equal(a, b)


def test_all_three_switches_on_cpu_are_unchanged():
    weights = {k: torch.as_tensor(v) for k, v in synth.transformer_weights(7, 64, 2).items()}
    off = transformer.LocalFeatureTransformer(FINE).train()
    on = transformer.LocalFeatureTransformer(FINE, hip_attention=True, hip_tail=True, hip_proj=True).train()
    off.load_state_dict(weights)
    on.load_state_dict(weights)
    x0, x1, g0, g1 = (torch.as_tensor(synth.normal(13, i, (2, 25, 64))) for i in (1, 2, 3, 4))
    for a, b in zip(_run(on, (x0, x1), [g0, g1]), _run(off, (x0, x1), [g0, g1])):
        assert a is not None and torch.equal(a, b)


def test_supported_refuses_cpu_float64_and_256_channels():
    x = torch.zeros(3, 25, 64)
    assert not ops.qkv_projection_supported(x, x)
    assert not ops.qkv_projection_supported(x.double(), x.double())
    assert not ops.qkv_projection_supported(torch.zeros(3, 25, 256), torch.zeros(3, 25, 256))


def test_qkv_projection_raises_on_cpu_tensors():
    layer = transformer.EncoderLayer(64, 8)
    x = torch.zeros(3, 25, 64)
    with pytest.raises(RuntimeError):
        ops.qkv_projection(x, x, layer.q_proj.weight, layer.k_proj.weight, layer.v_proj.weight)
