"""transformer.full_attention - the yardstick of tests/test_gpu_full_attention.py - against the reference's own FullAttention
(tests/golden/full_attention_small.npz, written by tests/golden/make_golden_full_attention.py from
network/module/attentions.py in float64), gradients included; the module-level fallback of hip_attention=True with
attention='full' on CPU and on float64 tensors; and what ops.full_attention_supported refuses.  No GPU."""
import functools
import os

import numpy as np
import pytest
import torch

from featurematching_amd import ops, synth, transformer

import full_attention_ref as fref
import train_layers_yardstick as yard

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full_attention_small.npz")


@functools.lru_cache(maxsize=1)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("index,name", list(enumerate(fref.GOLDEN_CASES)))
def test_yardstick_is_the_references_attention(index, name):
    """The two are the same expressions in float64 (they agreed to 4e-16 when the fixture was written): 1e-12 max|value|."""
    dims = fref.GOLDEN_CASES[name]
    gold = _golden()
    q, k, v, g = (torch.as_tensor(t, dtype=torch.float64) for t in fref.inputs(fref.GOLDEN_SEED + index, dims))
    res = fref.autograd(transformer.full_attention, q, k, v, g)
    for key, got in zip(("out", "dq", "dk", "dv"), res):
        want = torch.as_tensor(gold[f"{name}_{key}"])
        assert want.dtype == torch.float64 and want.shape == got.shape
        top = want.abs().max().item()
        assert top > 0
        assert (got - want).abs().max().item() <= 1e-12 * top, (name, key)


def test_fixture_size():
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("kind", fref.KINDS)
@pytest.mark.parametrize("d", [8, 32])
def test_hard_inputs_are_finite_in_float32(kind, d):
    """what the GPU tests rest on: float32 torch autograd through the yardstick stays finite on the three hard kinds"""
    q, k, v, g = (torch.as_tensor(t) for t in fref.hard_inputs(kind, 5, (2, 130, 97, 8, d)))
    for t in fref.autograd(transformer.full_attention, q, k, v, g):
        assert bool(torch.isfinite(t).all())
    if kind == "shifted":                        # without the maximum subtracted, exp of these scores is inf
        assert (q[0, 0, 0] @ k[0, 0, 0] / d ** .5).item() > 100


CONFIGS = {"fine": ({'d_model': 64, 'nhead': 8, 'layer_names': ['self', 'cross'], 'attention': 'full'}, (5, 49), (5, 49)),
           "coarse": ({'d_model': 256, 'nhead': 8, 'layer_names': ['self', 'cross'], 'attention': 'full'}, (2, 30), (2, 20))}


def _module(cfg, dtype, **kw):
    m = transformer.LocalFeatureTransformer(cfg, **kw)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in
                       synth.transformer_weights(7, cfg['d_model'], len(cfg['layer_names'])).items()})
    return m.to(dtype).train()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_module_on_cpu_tensors_is_the_torch_function(monkeypatch, name, dtype):
    """attention='full', hip_attention=True on CPU tensors, float32 and float64: ops.full_attention_supported says no, so
    the layers run the torch function - the same bits and the same parameter gradients as hip_attention=False, and
    ops.full_attention is never called"""
    cfg, s0, s1 = CONFIGS[name]
    d = cfg['d_model']
    x0 = torch.as_tensor(synth.normal(11, 1, (*s0, d))).to(dtype)
    x1 = torch.as_tensor(synth.normal(11, 2, (*s1, d))).to(dtype)
    calls = yard.count_calls(monkeypatch, "full_attention")
    res = []
    for flag in (False, True):
        m = _module(cfg, dtype, hip_attention=flag)
        assert m.attention == 'full' and m.hip_attention is flag
        a, b = x0.clone().requires_grad_(True), x1.clone().requires_grad_(True)
        o0, o1 = m(a, b)
        assert o0.grad_fn is not None and o1.grad_fn is not None
        (o0.square().sum() + o1.sum()).backward()
        res.append((o0.detach(), o1.detach(), a.grad, b.grad, {k: p.grad for k, p in m.named_parameters()}))
    assert calls == {"full_attention": 0}
    for x, y in zip(res[0][:4], res[1][:4]):
        assert torch.equal(x, y)
    assert res[0][4].keys() == res[1][4].keys()
    for key in res[0][4]:
        assert res[0][4][key] is not None and torch.equal(res[0][4][key], res[1][4][key]), key


def test_state_dict_keys_are_unchanged():
    cfg = CONFIGS["fine"][0]
    plain = transformer.LocalFeatureTransformer(cfg)
    on = transformer.LocalFeatureTransformer(cfg, hip_attention=True)
    assert list(on.state_dict().keys()) == list(plain.state_dict().keys())
    assert set(plain.state_dict().keys()) == set(synth.transformer_weights(7, 64, 2).keys())     # the reference's names


def test_supported_refuses():
    q = torch.zeros(2, 25, 8, 8)
    assert not ops.full_attention_supported(q, q)                                # CPU
    assert not ops.full_attention_supported(q.double(), q.double())              # float64
    assert not ops.full_attention_supported(torch.zeros(2, 25, 4, 8), torch.zeros(2, 25, 4, 8))      # H = 4
    assert not ops.full_attention_supported(torch.zeros(2, 25, 8, 16), torch.zeros(2, 25, 8, 16))    # D = 16
    assert not ops.full_attention_supported(q, torch.zeros(3, 25, 8, 8))                             # another N


def test_cpu_tensors_and_masks_are_refused():
    q = torch.zeros(1, 25, 8, 8)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.full_attention(q, q, q)
    with pytest.raises(ValueError, match="mask"):
        ops.full_attention(q, q, q, kv_mask=torch.ones(1, 25))
    with pytest.raises(ValueError, match="mask"):
        ops.full_attention(q, q, q, q_mask=torch.ones(1, 25))
