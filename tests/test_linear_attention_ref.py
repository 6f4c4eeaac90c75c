"""transformer.linear_attention - the yardstick of tests/test_gpu_linear_attention.py - against the reference's own
LinearAttention (tests/golden/linear_attention_small.npz, written by tests/golden/make_golden_linear_attention.py from
network/module/attentions.py in float64), gradients included; and the module-level fallback of hip_attention=True on CPU
tensors.  No GPU."""
import functools
import os

import numpy as np
import pytest
import torch

from featurematching_amd import ops, synth, transformer

import linear_attention_ref as lref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_attention_small.npz")


@functools.lru_cache(maxsize=1)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("index,name", list(enumerate(lref.GOLDEN_CASES)))
def test_yardstick_is_the_references_attention(index, name):
    """The two are the same expressions in float64: 2^-52 times a few thousand operations stays below 1e-12 max|value|
    (they agreed to the last bit when the fixture was written)."""
    dims, masked = lref.GOLDEN_CASES[name]
    gold = _golden()
    q, k, v, g = (torch.as_tensor(t, dtype=torch.float64) for t in lref.inputs(lref.GOLDEN_SEED + index, dims))
    qm = km = None
    if masked:
        qm, km = (torch.as_tensor(m, dtype=torch.float64) for m in lref.ragged_masks(dims))
    res = lref.autograd(transformer.linear_attention, q, k, v, g, qm, km)
    for key, got in zip(("out", "dq", "dk", "dv"), res):
        want = torch.as_tensor(gold[f"{name}_{key}"])
        assert want.dtype == torch.float64 and want.shape == got.shape
        top = want.abs().max().item()
        assert top > 0
        assert (got - want).abs().max().item() <= 1e-12 * top, (name, key)
    if masked:                                   # the masks did something: padded rows carry no value and no gradient
        qm_b, km_b = lref.ragged_masks(dims)
        assert not qm_b.all() and not km_b.all()
        assert not gold[f"{name}_out"][~qm_b].any() and not gold[f"{name}_dk"][~km_b].any() and not gold[f"{name}_dv"][~km_b].any()


def test_fixture_size():
    assert os.path.getsize(GOLDEN) < 1 << 20


CONFIGS = {"fine": ({'d_model': 64, 'nhead': 8, 'layer_names': ['self', 'cross']}, (5, 49), (5, 49)),
           "coarse": ({'d_model': 256, 'nhead': 8, 'layer_names': ['self', 'cross']}, (2, 30), (2, 20))}


def _module(cfg, **kw):
    m = transformer.LocalFeatureTransformer(cfg, **kw)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in
                       synth.transformer_weights(7, cfg['d_model'], len(cfg['layer_names'])).items()})
    return m.train()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_module_on_cpu_tensors_is_the_torch_function(name):
    """hip_attention=True on CPU tensors: ops.linear_attention_supported says no, so the layers run the torch function -
    the same bits and the same parameter gradients as hip_attention=False"""
    cfg, s0, s1 = CONFIGS[name]
    d = cfg['d_model']
    x0 = torch.as_tensor(synth.normal(11, 1, (*s0, d)))
    x1 = torch.as_tensor(synth.normal(11, 2, (*s1, d)))
    res = []
    for flag in (False, True):
        m = _module(cfg, hip_attention=flag)
        assert m.hip_attention is flag and all(layer.hip_attention is flag for layer in m.layers)
        a, b = x0.clone().requires_grad_(True), x1.clone().requires_grad_(True)
        o0, o1 = m(a, b)
        assert o0.grad_fn is not None and o1.grad_fn is not None
        (o0.square().sum() + o1.sum()).backward()
        res.append((o0.detach(), o1.detach(), a.grad, b.grad, {k: p.grad for k, p in m.named_parameters()}))
    for x, y in zip(res[0][:4], res[1][:4]):
        assert torch.equal(x, y)
    assert res[0][4].keys() == res[1][4].keys()
    for key in res[0][4]:
        assert res[0][4][key] is not None and torch.equal(res[0][4][key], res[1][4][key]), key


def test_default_is_off_and_state_dict_keys_are_unchanged():
    cfg = CONFIGS["fine"][0]
    plain = transformer.LocalFeatureTransformer(cfg)
    assert plain.hip_attention is False and not any(layer.hip_attention for layer in plain.layers)
    assert transformer.EncoderLayer(64, 8).hip_attention is False
    on = transformer.LocalFeatureTransformer(cfg, hip_attention=True)
    assert list(on.state_dict().keys()) == list(plain.state_dict().keys())
    assert set(plain.state_dict().keys()) == set(synth.transformer_weights(7, 64, 2).keys())     # the reference's names


def test_cpu_tensors_are_refused():
    q = torch.zeros(1, 25, 8, 8)
    assert not ops.linear_attention_supported(q, q)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.linear_attention(q, q, q)
