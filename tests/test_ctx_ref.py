"""The float64 yardstick of the context layers (tests/ctx_layers_ref.py) pinned without a GPU: against the fixtures the
reference itself wrote, at the edges of its formula, and on the inputs of tests/test_gpu_ctx_layers.py - each of them
is what that file says it is."""
import numpy as np
import pytest
import torch

from featurematching_amd import synth
from oracle import matcher_ref as orc

import ctx_layers_ref as cr
from helpers import load_golden


def _f32(t):
    return t.float().numpy()


# ------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name,layers,gain,atol", [("tf_masked_small", ['self', 'cross'], 1.0, 2e-5),
                                                    ("tf_masked_coarse", cr.FOUR_LAYERS, 2.0, 3e-5)])
def test_float64_reproduces_the_reference_s_masked_outputs(name, layers, gain, atol):
    """the bars of tests/test_modules_cpu.py for the same fixtures"""
    g = load_golden(name)
    seed, n, l, s, d = [int(v) for v in g['meta']]
    w = synth.transformer_weights(seed, d, len(layers))
    x0 = (gain * synth.normal(seed, 1, (n, l, d))).astype(np.float32)
    x1 = (gain * synth.normal(seed, 2, (n, s, d))).astype(np.float32)
    y0, y1 = cr.ctx_layers64(x0, x1, w, layers, g['mask0'], g['mask1'])
    np.testing.assert_allclose(_f32(y0), g['out0'], rtol=0, atol=atol)
    np.testing.assert_allclose(_f32(y1), g['out1'], rtol=0, atol=atol)
    # the float32 evaluation the bars are made of sees the same fixture, and the masks matter
    z0, z1 = cr.ctx_layers32(x0, x1, w, layers, g['mask0'], g['mask1'])
    np.testing.assert_allclose(z0.numpy(), g['out0'], rtol=0, atol=atol)
    np.testing.assert_allclose(z1.numpy(), g['out1'], rtol=0, atol=atol)
    u0, _ = cr.ctx_layers64(x0, x1, w, layers)
    assert (u0 - y0).abs().max().item() > 1e-2


def test_float64_without_masks_against_the_oracle():
    """the inputs of tf_full_small (whose outputs are the other attention's), unmasked, against the oracle's float32"""
    g = load_golden("tf_full_small")
    seed, n, l, s, d = [int(v) for v in g['meta']]
    w = synth.transformer_weights(seed, d, 2)
    x0, x1 = synth.normal(seed, 1, (n, l, d)), synth.normal(seed, 2, (n, s, d))
    y0, y1 = cr.ctx_layers64(x0, x1, w, ['self', 'cross'])
    r0, r1 = orc.local_feature_transformer(x0, x1, w, 8, ['self', 'cross'])
    np.testing.assert_allclose(_f32(y0), r0.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(_f32(y1), r1.numpy(), rtol=0, atol=2e-5)
    # all-ones masks change nothing, bit for bit
    a0, a1 = cr.ctx_layers64(x0, x1, w, ['self', 'cross'], np.ones((n, l), bool), np.ones((n, s), bool))
    assert torch.equal(a0, y0) and torch.equal(a1, y1)


# ------------------------------------------------------------------ the edges of the formula
def test_formula_edges_are_finite():
    d, layers = 64, ['cross']
    w = synth.transformer_weights(41, d, 1)
    x0, x1 = synth.normal(41, 1, (2, 9, d)), synth.normal(41, 2, (2, 7, d))
    x0[1, 4] = 0.0                                             # an all-zero token
    m0, m1 = np.ones((2, 9), bool), np.ones((2, 7), bool)
    m1[0, :] = False                                           # a fully padded source sample
    m0[1, :] = False                                           # a fully padded query sample
    y0, y1 = cr.ctx_layers64(x0, x1, w, layers, m0, m1)
    assert torch.isfinite(y0).all() and torch.isfinite(y1).all()
    # no source: the message is 0 / (0 + eps) = 0, the merge of 0 is 0 and LN1 of a constant row is its bias - so the
    # layer is x + LN2(MLP([x, beta1])); the same holds for a padded query (Q = 0)
    t = lambda k: torch.as_tensor(w["layers.0." + k]).double()
    x = torch.as_tensor(x0).double()
    cat = torch.cat([x, t("norm1.bias").expand(2, 9, d)], 2)
    want = x + torch.nn.functional.layer_norm(torch.relu(cat @ t("mlp.0.weight").T) @ t("mlp.2.weight").T, (d,),
                                              t("norm2.weight"), t("norm2.bias"), 1e-5)
    assert (y0 - want).abs().max().item() <= 1e-12
    z0, z1 = cr.ctx_layers32(x0, x1, w, layers, m0, m1)
    assert torch.isfinite(z0).all() and torch.isfinite(z1).all()


# ------------------------------------------------------------------ the GPU cases are what they claim to be
def _report(tag, yard):
    for img, (o64, e32, omax) in enumerate(yard):
        assert torch.isfinite(o64).all()
        # a row whose float32 evaluation were exact would leave the bar at its floor alone
        assert torch.isfinite(e32).all() and (e32 > 0).all(), f"{tag} image {img}"
        print(f"E32 {tag} image {img}: rows {e32.numel()}, e32 {e32.min().item():.2e} .. {e32.max().item():.2e}, "
              f"max|out64| {omax.min().item():.2e} .. {omax.max().item():.2e}")


@pytest.mark.parametrize("w", [5, 7])
def test_fine_regimes(w):
    """matches of gain <= 8 stay inside the first scale's range with every operand of the kernel (|x|, the projections
    and the hidden layer among them); matches of gain >= 120 leave it in |x|, the projections or the hidden layer; gain 40
    lies between (printed: its window values and projections fit, its KV operand may not); e32 per match and gain"""
    wts = cr.fine_weights()
    for calm in (False, True):
        gains = cr.fine_gains(calm=calm)
        x0, x1 = cr.fine_inputs(w, gains)
        listed, amax = cr.operand_max(x0, x1, wts, cr.FINE_LAYERS)
        calm_rows = torch.as_tensor(gains <= cr.FINE_IN_RANGE)
        low = torch.as_tensor(gains >= cr.FINE_MUST_LOWER)
        assert (amax[calm_rows] < cr.F16_RANGE).all(), amax[calm_rows].max().item()
        assert (listed[low] > cr.F16_RANGE).all() and (amax < 65504.0 * 16).all()     # ... and inside the smallest scale's
        assert bool(low.any()) != calm and bool(calm_rows.all()) == calm
        yard = cr.yardstick(x0, x1, wts, cr.FINE_LAYERS, rows="match")
        _report(f"fine W={w} calm={calm}", yard)
        for gain in sorted(set(gains.tolist())):
            sel = torch.as_tensor(gains == np.float32(gain))
            print(f"E32 fine W={w} calm={calm} gain {gain:g}: |x|, projections, hidden <= {listed[sel].max().item():.3g}, "
                  f"every operand <= {amax[sel].max().item():.3g}, "
                  f"e32 {max(y[1][sel].max().item() for y in yard):.2e}, "
                  f"max|out64| {max(y[2][sel].max().item() for y in yard):.3g}")
    # e32 of the high-gain matches is the cancellation of elu(x) + 1 = expm1(x) + 1 in float32, not the conditioning of
    # the layers: a float32 evaluation with exp(x) there is two orders of magnitude closer to float64
    x0, x1 = cr.fine_inputs(w)
    ex = cr.exp_form_error(x0, x1, wts, cr.FINE_LAYERS)
    e32 = [y[1] for y in cr.yardstick(x0, x1, wts, cr.FINE_LAYERS, rows="match")]
    sel = torch.as_tensor(cr.fine_gains() >= cr.FINE_MUST_LOWER)
    print(f"E32 fine W={w} gain >= 120: e32 {max(e[sel].max().item() for e in e32):.2e}, "
          f"with exp(x): {max(e[sel].max().item() for e in ex):.2e}")
    assert max(e[sel].max().item() for e in ex) < 0.1 * max(e[sel].max().item() for e in e32)
    # every workgroup of 8 matches of the mixed case holds both kinds of wave
    low = cr.fine_gains() >= cr.FINE_MUST_LOWER
    for b in range(0, cr.FINE_M, 8):
        assert low[b:b + 8].any() and not low[b:b + 8].all()


@pytest.mark.parametrize("n,l,s,layers", cr.COARSE_SHAPES)
def test_coarse_shape_cases(n, l, s, layers):
    x0, x1 = cr.coarse_inputs(n, l, s)
    _report(f"coarse ({n},{l},{s})", cr.yardstick(x0, x1, cr.coarse_weights(len(layers)), layers))


def test_coarse_token_gains_and_masks():
    x0, x1, c0, c1 = cr.token_gain_inputs()
    for k in range(3):                       # every tile of 32 tokens holds every magnitude
        assert all((c0[:, t:t + 32] == k).any() for t in range(0, 77, 32)) and (c1[:, :32] == k).any()
    assert not x1[0, 5].any() and np.abs(x0[1, 9]).max() == np.float32(1e4)
    wts = cr.coarse_weights(4)
    _report("coarse token gains", cr.yardstick(x0, x1, wts, cr.FOUR_LAYERS))
    x0, x1 = cr.coarse_inputs(2, 77, 45)
    for name, (m0, m1) in cr.mask_cases().items():
        _report(f"coarse masks {name}", cr.yardstick(x0, x1, wts, cr.FOUR_LAYERS, m0, m1))
    m0, m1 = cr.mask_cases()["both"]
    assert not m1[0].any() and m1[1, :33].all() and not m1[1, 33:].any()
    assert m0[0, :70].all() and not m0[0, 70:].any() and not m0[1, 3:40].any() and m0[1, :3].all() and m0[1, 40:].all()


def test_coarse_layernorm_cases():
    x0, x1 = cr.coarse_inputs(1, 70, 45)
    cases = cr.layernorm_cases(2)
    g = cases["wide"]["layers.1.norm1.weight"]
    assert (g == 0).sum() >= 80 and g.max() == 25.0 and np.abs(cases["wide"]["layers.1.norm1.bias"]).max() == np.float32(5.0)
    assert not cases["zero"]["layers.0.norm1.weight"].any() and not cases["zero"]["layers.0.norm1.bias"].any()
    for name, w in cases.items():
        _report(f"coarse layernorm {name}", cr.yardstick(x0, x1, w, ['self', 'cross']))
