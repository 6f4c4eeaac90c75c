"""The `hip_merge` switch of FinePreprocess and the trainable Matcher without a GPU: on CPU tensors the switch changes
nothing, bit for bit; the Matcher keeps its state-dict keys and leaves no training flag behind in eval mode."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from featurematching_amd import modules, ops, synth
from featurematching_amd.matcher import Matcher

import window_merge_ref as wref


class _NoBackbone(nn.Module):            # the feature extractor is out of scope: a parameter-free stand-in
    def forward(self, x):
        raise RuntimeError("not used")


def _reference_keys():
    """the key set of the reference's net(...).state_dict() without its backbone (tests/test_modules_cpu.py)"""
    keys = {}
    for name, d, n in (("coarse", 256, 8), ("fine", 64, 2)):
        for k in range(n):
            for lin, shape in (("q_proj", (d, d)), ("k_proj", (d, d)), ("v_proj", (d, d)), ("merge", (d, d)),
                               ("mlp.0", (2 * d, 2 * d)), ("mlp.2", (d, 2 * d))):
                keys[f"{name}.layers.{k}.{lin}.weight"] = shape
            for ln in ("norm1", "norm2"):
                keys[f"{name}.layers.{k}.{ln}.weight"] = (d,)
                keys[f"{name}.layers.{k}.{ln}.bias"] = (d,)
    keys.update({"fine_preprocess.down_proj.weight": (64, 256), "fine_preprocess.down_proj.bias": (64,),
                 "fine_preprocess.merge_feat.weight": (64, 128), "fine_preprocess.merge_feat.bias": (64,),
                 "fine_matching.mix_feat_0.weight": (1, 49), "fine_matching.mix_feat_0.bias": (1,),
                 "fine_matching.mix_feat_1.weight": (1, 49), "fine_matching.mix_feat_1.bias": (1,)})
    return keys


CFG = {'fine_concat_coarse_feat': True, 'fine_window_size': 7, 'coarse': {'d_model': 32}, 'fine': {'d_model': 64}}


def _unfold_crop(feat, b_ids, ids, w, stride, w_c, h_c, pad=2, cells=None):
    """fine_preprocess.py:43-50: F.unfold, then the listed cells (its backward, a fold, adds in a fixed order)"""
    n, c = feat.shape[:2]
    unf = F.unfold(feat, (w, w), stride=stride, padding=pad)
    assert unf.shape[2] == h_c * w_c
    return unf.view(n, c, w * w, -1).permute(0, 3, 2, 1)[b_ids, ids]


def _cpu_crop(monkeypatch):
    """the crop has no CPU path: the torch unfold stands in for ops.gather_windows_grad, for both modules alike"""
    monkeypatch.setattr(ops, "gather_windows_grad", _unfold_crop)
    calls = []
    monkeypatch.setattr(ops, "window_merge", lambda *a, **kw: calls.append(1))
    return calls


def _run(fp, maps, descs, data, grads):
    leaves = [t.detach().clone().requires_grad_(True) for t in maps + descs]
    w0, w1 = fp(leaves[0], leaves[1], leaves[2], leaves[3], dict(data))
    torch.autograd.backward([w0, w1], grads)
    return [w0.detach(), w1.detach()] + [t.grad for t in leaves] + [p.grad for _, p in sorted(fp.named_parameters())]


@pytest.mark.parametrize("w", [5, 7])
def test_fine_preprocess_on_cpu_is_unchanged(monkeypatch, w):
    calls = _cpu_crop(monkeypatch)
    cfg = dict(CFG, fine_window_size=w)
    torch.manual_seed(3)
    off = modules.FinePreprocess(cfg).train()
    on = modules.FinePreprocess(cfg, hip_merge=True).train()
    on.load_state_dict(off.state_dict())
    assert on.hip_merge and not off.hip_merge and list(on.state_dict()) == list(off.state_dict())
    m = 21
    cells = wref.HC * wref.WC                                        # distinct (sample, cell) pairs: no select adds twice
    pick = synth.permutation(40, 7, wref.N * cells)[:m]
    b_ids, i_ids, j_ids = pick // cells, pick % cells, (pick % cells + 5) % cells
    data = {'hw0_f': (wref.HF, wref.WF), 'hw0_c': (wref.HC, wref.WC), 'hw1_c': (wref.HC, wref.WC),
            'b_ids': torch.as_tensor(b_ids), 'i_ids': torch.as_tensor(i_ids), 'j_ids': torch.as_tensor(j_ids)}
    maps = [torch.as_tensor(wref.fine_map(s)) for s in (42, 43)]
    descs = [torch.as_tensor(synth.normal(44, i, (wref.N, wref.HC * wref.WC, 32))) for i in (1, 2)]
    grads = [torch.as_tensor(synth.normal(45, i, (m, w * w, 64))) for i in (1, 2)]
    got, want = _run(on, maps, descs, data, grads), _run(off, maps, descs, data, grads)
    assert len(got) == 2 + 4 + 4
    for a, b in zip(got, want):
        assert a is not None and torch.equal(a, b)
    assert not calls                                                 # CPU tensors never reach the HIP op


def test_supported_refuses_what_the_op_does_not_serve():
    x = torch.zeros(1, 64, 8, 8)
    assert not ops.window_merge_supported(x, 7)                      # a CPU map
    assert not ops.window_merge_supported(x, 9)
    with pytest.raises(RuntimeError):
        ops.window_merge(x, torch.zeros(64, 64), torch.zeros(1, 64), torch.zeros(1, dtype=torch.int64),
                         torch.zeros(1, dtype=torch.int64), 7, 4, 2, 2)


def test_matcher_keeps_its_state_dict_keys():
    for kw in ({}, {'hip_train': False}, {'train_coarse': 'matrix'}):
        m = Matcher(backbone=_NoBackbone(), **kw)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == _reference_keys()
    with pytest.raises(ValueError):
        Matcher(backbone=_NoBackbone(), train_coarse='dense')


def _switches(m):
    tf = [(t.hip_attention, t.hip_tail, t.hip_proj) for t in (m.coarse, m.fine)]
    layers = [(l.hip_attention, l.hip_tail, l.hip_proj) for t in (m.coarse, m.fine) for l in t.layers]
    return set(tf + layers + [(m.fine_preprocess.hip_merge,) * 3])


@pytest.mark.parametrize("train_coarse", ["stats", "matrix"])
@pytest.mark.parametrize("hip_train", [True, False])
def test_no_training_flag_survives_eval(hip_train, train_coarse):
    m = Matcher(backbone=_NoBackbone(), hip_train=hip_train, train_coarse=train_coarse)
    cm = m.coarse_matching
    for step in (m, m.train(), m.eval().train()):                    # a fresh module is in training mode
        assert step.training and (cm.loss_stats, cm.conf_matrix) == (train_coarse == 'stats', train_coarse == 'matrix')
        assert _switches(m) == {(hip_train,) * 3}
    m.eval()
    assert not m.training and not cm.training
    assert cm.loss_stats is False and cm.conf_matrix is False
    assert _switches(m) == {(False,) * 3}
    never = Matcher(backbone=_NoBackbone(), hip_train=False).eval()
    assert (never.coarse_matching.loss_stats, never.coarse_matching.conf_matrix) == (False, False)
    assert _switches(never) == {(False,) * 3}


def test_training_mode_names_the_missing_supervision():
    class _Maps(nn.Module):
        def forward(self, x):
            return torch.zeros(x.shape[0], 256, 2, 2), torch.zeros(x.shape[0], 64, 8, 8)
    m = Matcher(backbone=_Maps()).train()
    img = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="compute_supervision_coarse"):
        m({'image0': img, 'image1': img})
    with pytest.raises(RuntimeError, match="compute_supervision_coarse"):
        c, f = _Maps()(img)
        m.forward_features(c, c, f, f, {'bs': 1, 'hw0_i': (16, 16), 'hw1_i': (16, 16)})
    with pytest.raises(RuntimeError, match="training mode"):
        m.eval().training_step({'image0': img, 'image1': img}, None)
