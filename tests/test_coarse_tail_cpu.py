"""The `hip_coarse_tail` switch of the context layers and the Matcher's `hip_train_coarse` without a GPU: on CPU and
float64 tensors the switch changes nothing, bit for bit; ops.coarse_tail refuses what it does not serve; the Matcher's
training mode sets the switch and eval mode clears it."""
import pytest
import torch

from featurematching_amd import ops, synth, transformer
from featurematching_amd.matcher import Matcher

COARSE = {'d_model': 256, 'nhead': 8, 'layer_names': ['self', 'cross']}


def _run(module, inputs, grads, **kw):
    inputs = [t.detach().clone().requires_grad_(True) for t in inputs]
    outs = module(*inputs, **kw)
    outs = outs if isinstance(outs, tuple) else (outs,)
    torch.autograd.backward(list(outs), grads)
    return [o.detach() for o in outs] + [t.grad for t in inputs] + [p.grad for _, p in sorted(module.named_parameters())]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_encoder_layer_on_cpu_is_unchanged(dtype):
    torch.manual_seed(5)
    off = transformer.EncoderLayer(256, 8).to(dtype).train()
    on = transformer.EncoderLayer(256, 8, hip_coarse_tail=True).to(dtype).train()
    on.load_state_dict(off.state_dict())
    assert on.hip_coarse_tail and not off.hip_coarse_tail and list(on.state_dict()) == list(off.state_dict())
    x, src, g = (torch.as_tensor(synth.normal(11, i, s)).to(dtype) for i, s in ((1, (2, 25, 256)), (2, (2, 30, 256)),
                                                                                 (3, (2, 25, 256))))
    for a, b in zip(_run(on, (x, src), [g]), _run(off, (x, src), [g])):
        assert a is not None and torch.equal(a, b)


@pytest.mark.parametrize("masked", [False, True])
def test_coarse_transformer_on_cpu_is_unchanged(masked):
    weights = {k: torch.as_tensor(v) for k, v in synth.transformer_weights(7, 256, 2).items()}
    off = transformer.LocalFeatureTransformer(COARSE).train()
    on = transformer.LocalFeatureTransformer(COARSE, hip_coarse_tail=True).train()
    off.load_state_dict(weights)
    on.load_state_dict(weights)
    assert all(layer.hip_coarse_tail for layer in on.layers) and not any(layer.hip_coarse_tail for layer in off.layers)
    assert on.hip_coarse_tail and not off.hip_coarse_tail and not on.hip_tail
    x0, x1, g0, g1 = (torch.as_tensor(synth.normal(12, i, (2, 40, 256))) for i in (1, 2, 3, 4))
    kw = {}
    if masked:
        mask0 = torch.ones(2, 40, dtype=torch.bool)
        mask0[1, 30:] = False
        kw = {'mask0': mask0}
    for a, b in zip(_run(on, (x0, x1), [g0, g1], **kw), _run(off, (x0, x1), [g0, g1], **kw)):
        assert a is not None and torch.equal(a, b)


def test_switch_is_an_attribute_of_the_transformer():
    tf = transformer.LocalFeatureTransformer(COARSE)
    assert not tf.hip_coarse_tail
    tf.hip_coarse_tail = True
    assert all(layer.hip_coarse_tail for layer in tf.layers) and not tf.hip_tail
    tf.hip_coarse_tail = False
    assert not any(layer.hip_coarse_tail for layer in tf.layers)


def test_supported_refuses_cpu_float64_and_64_channels():
    x = torch.zeros(3, 25, 256)
    assert not ops.coarse_tail_supported(x, x)
    assert not ops.coarse_tail_supported(x.double(), x.double())
    assert not ops.coarse_tail_supported(torch.zeros(3, 25, 64), torch.zeros(3, 25, 64))


def test_coarse_tail_raises_on_cpu_tensors():
    layer = transformer.EncoderLayer(256, 8)
    x = torch.zeros(3, 25, 256)
    with pytest.raises(RuntimeError):
        ops.coarse_tail(x, x, layer.merge.weight, layer.norm1.weight, layer.norm1.bias, layer.mlp[0].weight,
                        layer.mlp[2].weight, layer.norm2.weight, layer.norm2.bias, 1e-5, 1e-5)


def test_matcher_switch_and_state_dict():
    torch.manual_seed(0)
    plain = Matcher()
    assert plain.hip_train_coarse is False
    plain.train()
    assert not plain.coarse.hip_coarse_tail and plain.coarse.hip_attention
    m = Matcher(hip_train_coarse=True)
    assert list(m.state_dict()) == list(plain.state_dict())
    assert m.training and m.coarse.hip_coarse_tail                   # (a fresh module is in training mode)
    m.eval()
    assert not m.coarse.hip_coarse_tail
    m.train()
    assert m.coarse.hip_coarse_tail and not m.fine.hip_coarse_tail and m.coarse.hip_attention
    m.eval()
    assert not m.coarse.hip_coarse_tail
    m.train(False)
    assert not m.coarse.hip_coarse_tail
    off = Matcher(hip_train=False, hip_train_coarse=True).train()    # hip_train=False overrides it
    assert not off.coarse.hip_coarse_tail and not off.coarse.hip_attention
