"""The trainable Matcher on the GPU: Matcher.training_step - the reference's training step (lightning_new.py:216-230) - from
the images to Loss and back, with the HIP training ops on (hip_train=True) and off.

Images 1 x 3 x 96 x 128 (coarse grid 12 x 16, fine maps 48 x 64, W = 7) with 300 seeded correspondences
(supervision_ref.points).  profiles/matcher_train_accuracy.txt holds every ACC line these tests print."""
import pytest
import torch

from featurematching_amd import modules, supervision, synth
from featurematching_amd.matcher import Matcher
from featurematching_amd.transformer import LocalFeatureTransformer

import matcher_train_ref as mref
import supervision_ref as sref
from train_layers_yardstick import count_calls

pytestmark = pytest.mark.gpu
HC, WC, HF, WF, DEV = mref.HC, mref.WC, mref.HF, mref.WF, mref.DEV
OPS = ("window_merge", "linear_attention", "encoder_tail", "qkv_projection")
_data, _matcher, _loss, _step = mref.batch, mref.matcher, mref.loss_module, mref.step


@pytest.fixture
def deterministic_torch():
    """torch's own scatter-adds (the backward of feat_c[b_ids, ids]) in a fixed order while two runs are compared"""
    before = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(before[0], warn_only=before[1])


# ---- (a) -------------------------------------------------------------------------------------------------------------
def test_training_step_reaches_every_parameter():
    m = _matcher()
    with pytest.raises(RuntimeError, match="compute_supervision_coarse"):    # no supervision ids yet
        m(_data(61))
    data = _data(61, grad=True)
    loss, grads = _step(m, data)
    assert loss.dim() == 0 and torch.isfinite(loss) and loss.item() > 0
    assert data['loss'].grad_fn is not None and '_fm_coarse_loss' in data and 'conf_matrix' not in data
    assert torch.equal(data['i_ids'], data['spv_i_ids']) and data['mkpts0_f'].shape == (data['i_ids'].shape[0], 3)
    for sub in ("backbone", "coarse", "fine_preprocess", "fine", "fine_matching"):
        assert any(k.startswith(sub + ".") for k in grads), sub
    for name, g in grads.items():
        assert g is not None, name
        assert torch.isfinite(g).all(), name
        assert g.abs().max().item() > 0, name


# ---- (b) -------------------------------------------------------------------------------------------------------------
def _chain_inputs(seed=33):
    """the inputs of tests/test_gpu_loss_chain.py's chain, the descriptors as maps [1, 64, hc, wc]"""
    c0, c1 = synth.coarse_descriptors(seed, 1, HC * WC, 64, "borderline")
    f0, f1 = synth.fine_maps(seed, 1, 64, HF, WF)
    to_map = lambda c: torch.as_tensor(c, device=DEV).transpose(1, 2).reshape(1, 64, HC, WC).contiguous()
    img = torch.zeros(1, 1, HC * 8, WC * 8, device=DEV)
    data = {'image0': img, 'image1': img, 'bs': 1, 'hw0_i': (HC * 8, WC * 8), 'hw1_i': (HC * 8, WC * 8),
            'origin_kp0': torch.as_tensor(sref.points(seed, 300, (HC, WC), 0), device=DEV)[None],
            'origin_kp1': torch.as_tensor(sref.points(seed, 300, (HC, WC), 1), device=DEV)[None]}
    return [to_map(c0), to_map(c1), torch.as_tensor(f0, device=DEV), torch.as_tensor(f1, device=DEV)], data


def _by_hand(m, maps, data):
    """network/net.py:66-92 in training mode from separately built modules that hold the matcher's weights"""
    cfg = m.config
    tfc, tff = LocalFeatureTransformer(cfg['coarse']), LocalFeatureTransformer(cfg['fine'])
    cm = modules.CoarseMatching(cfg['match_coarse'], loss_stats=True)
    fp = modules.FinePreprocess(cfg)
    fm = modules.FineMatching(window=cfg['fine_window_size'])
    for mod, src in ((tfc, m.coarse), (tff, m.fine), (fp, m.fine_preprocess), (fm, m.fine_matching)):
        mod.load_state_dict(src.state_dict())
    for mod in (tfc, tff, cm, fp, fm):
        mod.to(DEV).train()
    supervision.data_preprocess(data)
    supervision.compute_supervision_coarse(data)
    data.update({'hw0_c': (HC, WC), 'hw1_c': (HC, WC), 'hw0_f': (HF, WF), 'hw1_f': (HF, WF)})
    c0, c1 = (t.flatten(2).transpose(1, 2).contiguous() for t in maps[:2])
    c0, c1 = tfc(c0, c1)
    cm(c0, c1, data)
    w0, w1 = fp(maps[2], maps[3], c0, c1, data)
    w0, w1 = tff(w0, w1)
    fm(w0, w1, data)
    supervision.compute_supervision_fine(data)
    _loss()(data)
    return data['loss'].detach()


def test_forward_features_is_the_hand_written_chain():
    """forward_features (hip_train=False, 'stats') against network/net.py:66-92 wired by hand from separately built modules:
    the same loss, bit for bit.  Shared with tests/test_gpu_loss_chain.py are the INPUTS only (its seed-33 descriptors, fine
    maps and correspondences).  A Matcher has a coarse level, so both sides here run a coarse LocalFeatureTransformer (d_model
    64, self + cross) that chain does not have; the weights are the Matcher's own seeded draw, handed to the modules of the
    hand-written side, and CoarseMatching takes DEFAULT_CONFIG's match_coarse (that chain's thr, border_rm and temperature)."""
    cfg = {'coarse': {'d_model': 64, 'nhead': 8, 'layer_names': ['self', 'cross'], 'attention': 'linear'}}
    m = _matcher(seed=33, config=cfg, hip_train=False, train_coarse='stats')
    maps, data = _chain_inputs()
    hand = [_by_hand(m, maps, dict(data)) for _ in range(2)]
    apart = (hand[0].double() - hand[1].double()).abs().item()
    supervision.data_preprocess(data)
    supervision.compute_supervision_coarse(data)
    assert 100 < data['spv_i_ids'].shape[0] < 192
    m.forward_features(*maps, data)
    supervision.compute_supervision_fine(data)
    _loss()(data)
    got = data['loss'].detach()
    print(f"ACC  matcher chain     loss {got.item():.9e}  by hand {hand[0].item():.9e}  hand-written chain run to run {apart:.3e}")
    assert torch.isfinite(got) and got.item() > 0 and data['loss'].grad_fn is not None
    if apart == 0:
        assert torch.equal(got, hand[0])
    else:                                                            # the chain itself is not bit-reproducible
        assert (got.double() - hand[0].double()).abs().item() <= 4 * apart


# ---- (c) -------------------------------------------------------------------------------------------------------------
def test_hip_train_on_against_off(monkeypatch, deterministic_torch):
    """every switch engages, and nothing is dropped or doubled: loss and every gradient within 1e-3 of max|g_off| - a wiring
    check (a missing or doubled term shows at 1e-1 or more; the ops' own bars are 1e-5 or less).  On the patch backbone
    and with torch's deterministic algorithms: what is left between the two runs is the HIP ops against the torch lines.

    g_off - float32 torch - is the reference here, so the weights are such that it is one: FinePreprocess holds the
    fixtures' weights (fixture_merge), which give windows of magnitude 3 whose tokens differ.  With the module's own kaiming
    fan-out draw the context row (magnitude 45) swamps the window, every token of a window is nearly the same, and the first
    self layer's q / k gradients are residuals of cancelling terms that float32 torch does not resolve: measured on the
    fine layers alone with the step's own windows and gradients, against float64, torch's q_proj / k_proj gradient of layer 0
    is 8.7e-3 / 9.1e-3 off (ops.linear_attention: 2.9e-5 / 8.6e-5) there, and 1.1e-5 / 1.5e-5 off (2.5e-5 / 5.8e-5) with
    the fixtures' weights (profiles/matcher_train_accuracy.txt)."""
    off = _matcher(hip_train=False, patches=True, fixture_merge=True)
    on = _matcher(hip_train=True, patches=True, fixture_merge=True)
    on.load_state_dict(off.state_dict())
    calls = count_calls(monkeypatch, *OPS)
    loss_off, g_off = _step(off, _data(62, grad=True))
    assert calls == {k: 0 for k in OPS}
    loss_on, g_on = _step(on, _data(62, grad=True))
    # one merge per image; every layer runs twice (coarse 8 + fine 2 layers); d_model 256 keeps the torch tail and projections
    assert calls == {"window_merge": 2, "linear_attention": 20, "encoder_tail": 4, "qkv_projection": 4}
    d_loss = abs(loss_on.item() - loss_off.item())
    print(f"ACC  matcher on/off    loss off {loss_off.item():.9e}  on {loss_on.item():.9e}  |diff| / |off| {d_loss / abs(loss_off.item()):.3e}")
    rows = []
    for name, g in g_off.items():
        top = g.abs().max().item()
        diff = (g_on[name].double() - g.double()).abs().max().item()
        print(f"ACC  matcher on/off    {name:44s} max|g_off| {top:.3e}  max|g_on - g_off| / max|g_off| {diff / top:.3e}")
        rows.append((name, diff, top))
    assert d_loss <= 1e-3 * abs(loss_off.item())
    for name, diff, top in rows:
        assert diff <= 1e-3 * top, (name, diff, top)


def test_default_init_hip_layers_against_float64(deterministic_torch):
    """The module's own initialisation, which test_hip_train_on_against_off leaves out because float32 torch is no
    reference there: the HIP side is held to float64 instead.  The fine layers alone, on the windows and upstream gradients
    of a training step of the default-initialised matcher (patch backbone), with all three HIP switches against a float64
    copy of the layers: every parameter's gradient, both window gradients and the output within the issue's wiring bar,
    1e-3 of max|ref64|.  The float32 torch layers are printed beside them and not asserted."""
    m = _matcher(hip_train=False, patches=True)
    names, tops, (e_torch, e_hip), top_x = mref.fine_layers_against_float64(
        m, _data(62, grad=True), switches=({}, dict(hip_attention=True, hip_tail=True, hip_proj=True)))
    assert top_x > 10                                                # the context row swamps the windows (magnitude 45)
    for name, top, et, eh in zip(names, tops, e_torch, e_hip):
        print(f"ACC  default init f64  {name:28s} max|ref64| {top:.3e}  e_torch32 {et:.3e}  e_hip {eh:.3e}")
    for name, top, eh in zip(names, tops, e_hip):
        assert top > 0 and eh <= 1e-3, (name, eh)


# ---- (d) -------------------------------------------------------------------------------------------------------------
def test_train_coarse_matrix_takes_the_dense_branch():
    m = _matcher(train_coarse='matrix')
    data = _data(63, grad=True)
    loss, grads = _step(m, data)
    assert data['conf_matrix'].shape == (1, HC * WC, HC * WC) and data['conf_matrix'].grad_fn is not None
    assert '_fm_coarse_loss' not in data and data['conf_matrix_gt'].shape == data['conf_matrix'].shape
    assert torch.isfinite(loss) and loss.item() > 0
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
    assert grads['coarse.layers.0.q_proj.weight'].abs().max().item() > 0      # the coarse loss reached the coarse layers
    stats_loss, _ = _step(_matcher(train_coarse='stats'), _data(63, grad=True))
    assert abs(stats_loss.item() - loss.item()) <= 1e-4 * abs(loss.item())    # the same loss, with and without the matrix


# ---- (e) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hip_train", [True, False])
def test_eval_after_training_mode_is_the_eval_matcher(hip_train):
    never = _matcher(seed=5, hip_train=False, patches=True).eval()
    m = _matcher(seed=5, hip_train=hip_train, patches=True)
    _step(m, _data(65, grad=True))                                   # a training step ...
    m.load_state_dict(never.state_dict())                            # ... and the weights and batch-norm statistics of before
    img0, img1 = (torch.as_tensor(synth.normal(64, k, (1, 3, HC * 8, WC * 8)), device=DEV) for k in (1, 2))
    m.eval()
    assert not m.coarse_matching.loss_stats and not m.coarse_matching.conf_matrix
    want, got = never.match(img0, img1), m.match(img0, img1)
    assert '_fm_coarse' in m.last and '_fm_coarse_loss' not in m.last and 'conf_matrix' not in m.last
    assert not any(t.requires_grad for t in got)
    for u, v in zip(got, want):
        assert u.shape == v.shape and torch.equal(u, v)
