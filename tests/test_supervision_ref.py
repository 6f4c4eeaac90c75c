"""The supervision and the fine loss without a GPU: the float64 / NumPy restatement the GPU tests are held to
(tests/supervision_ref.py), supervision.compute_supervision_coarse / compute_supervision_fine and the CPU branch of
modules.FineLoss / Loss against the fixture written by the reference's own code
(tests/golden/make_golden_supervision.py).

Ids and tables: exactly equal.  Loss values: |got - loss64| <= 4 e_ref + FLOOR |loss64| with e_ref = |loss_ref32 - loss64|,
both of the reference's own numbers in the fixture; FLOOR as in tests/test_gpu_fine_loss.py
(profiles/fine_loss_accuracy.txt)."""
import logging
import os

import numpy as np
import pytest
import torch

from featurematching_amd import modules, supervision, synth
from oracle import matcher_ref as orc

import supervision_ref as sref

FLOOR = 2 * 1.15e-7        # profiles/fine_loss_accuracy.txt: the largest e_ref / |loss64| over the inputs of tests/test_gpu_fine_loss.py
GRIDS = ((8, 12), (12, 16))
KS = (1, 5, 300)
CASES = [(hw, k) for hw in GRIDS for k in KS]
SEED = 47                 # make_golden_supervision.py
CONFIG = {'module': {'loss': {'fine_correct_thr': 1.0, 'pos_weight': 1.0, 'neg_weight': 1.0, 'pose_loss_cal_flag': False,
                              'coarse_type': 'focal', 'focal_alpha': 0.25, 'focal_gamma': 2.0, 'coarse_weight': 1.0,
                              'fine_weight': 0.25},
                     'match_coarse': {'sparse_spvs': False}}}
SCALARS = ("loss_c", "loss_f", "loss_pose", "loss")
PRE_KEYS = ('coarse_kp0', 'coarse_kp1', 'fine_kp0', 'fine_kp1', 'lists_f0', 'lists_f1', 'fine_mtx_0', 'fine_mtx_1')


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "supervision_small.npz"))


def _case(golden, hw, k):
    pre = f"g{hw[0]}x{hw[1]}_k{k}_"
    return {key[len(pre):]: golden[key] for key in golden.files if key.startswith(pre)}


def _data(g, hw):
    """what data_preprocess leaves in the data dict, from the fixture (the function itself runs on the GPU only)"""
    img = torch.zeros(1, 1, hw[0] * 8, hw[1] * 8)
    data = {'image0': img, 'image1': img, 'pair_names': 'fixture'}
    data.update({key: torch.as_tensor(g[key]) for key in PRE_KEYS})
    return data


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _close(got, want64, ref32):
    return abs(got - want64) <= 4 * abs(float(ref32) - want64) + FLOOR * abs(want64)


def test_fixture_has_the_cases_it_should(golden):
    left_out = np.zeros(2, np.int64)
    for hw, k in CASES:
        g = _case(golden, hw, k)
        assert g["kp0"].shape == (k, 2) and g["kp0"].dtype == np.float32
        n = g["spv_i_ids"].shape[0]
        assert 1 <= n <= k and g["fine_kp0"].shape == (1, n, 2) and g["fine_mtx_0"].shape == (1, hw[0] * hw[1], 2)
        assert g["i_ids"].shape[0] == n + 7
        assert int(g["coarse_raised"]) == (1 if n == 1 else 0)
        if k == 300:        # many correspondences per cell, many survivors per image-0 cell
            assert n < k // 2 and n - len(np.unique(g["spv_i_ids"])) > 20
        left_out += np.array([(g["expec_f_gt_0"][:, 0] == 0).sum(), (g["expec_f_gt_1"][:, 0] == 0).sum()])
    assert left_out.min() >= 6                       # rows the fine loss leaves out, in either image


@pytest.mark.parametrize("hw,k", CASES)
def test_restatement_is_the_references_data_preprocess(golden, hw, k):
    g = _case(golden, hw, k)
    out = sref.supervise(g["kp0"], g["kp1"], hw, hw)
    for key in PRE_KEYS:
        assert out[key].dtype == g[key].dtype == np.float32, key
        assert np.array_equal(_bits(out[key]), _bits(g[key][0])), key
    assert np.array_equal(out["i_ids"], g["spv_i_ids"]) and np.array_equal(out["j_ids"], g["spv_j_ids"])


@pytest.mark.parametrize("hw,k", CASES)
def test_supervision_functions_on_cpu_tensors(golden, hw, k):
    g = _case(golden, hw, k)
    data = _data(g, hw)
    supervision.compute_supervision_coarse(data, {'MODULE': {'RESOLUTION': (8, 2)}}, dense_gt=True)
    for key in ("spv_i_ids", "spv_j_ids"):
        assert data[key].dtype == torch.int64 and np.array_equal(data[key].numpy(), g[key]), key
    assert data['spv_b_ids'].dtype == torch.int64 and not data['spv_b_ids'].any()
    assert data['spv_fine_0'] is data['fine_kp0'] and data['spv_fine_1'] is data['fine_kp1']
    assert data['conf_matrix_gt'].dtype == torch.float32
    assert np.array_equal(torch.nonzero(data['conf_matrix_gt'][0]).numpy(), g["gt_pos"])
    plain = _data(g, hw)
    supervision.compute_supervision_coarse(plain)
    assert 'conf_matrix_gt' not in plain and torch.equal(plain['spv_i_ids'], data['spv_i_ids'])
    data.update({'b_ids': torch.as_tensor(g["b_ids"]), 'i_ids': torch.as_tensor(g["i_ids"]), 'j_ids': torch.as_tensor(g["j_ids"])})
    supervision.compute_supervision_fine(data)
    for key in ("expec_f_gt_0", "expec_f_gt_1"):
        assert np.array_equal(_bits(data[key].numpy()), _bits(g[key])), key


def test_compute_supervision_fine_any_batch():
    mtx0, mtx1 = torch.arange(2 * 6 * 2.).reshape(2, 6, 2), -torch.arange(2 * 5 * 2.).reshape(2, 5, 2)
    data = {'fine_mtx_0': mtx0, 'fine_mtx_1': mtx1, 'b_ids': torch.tensor([1, 0, 1]), 'i_ids': torch.tensor([5, 0, 2]),
            'j_ids': torch.tensor([4, 4, 0])}
    supervision.compute_supervision_fine(data)
    assert torch.equal(data['expec_f_gt_0'], torch.stack([mtx0[1, 5], mtx0[0, 0], mtx0[1, 2]]))
    assert torch.equal(data['expec_f_gt_1'], torch.stack([mtx1[1, 4], mtx1[0, 4], mtx1[1, 0]]))


def test_empty_supervision_falls_back_with_one_warning(caplog):
    img = torch.zeros(1, 1, 64, 96)
    none = torch.zeros(1, 0, 2)
    data = {'image0': img, 'image1': img, 'coarse_kp0': none, 'coarse_kp1': none, 'fine_kp0': none, 'fine_kp1': none}
    with caplog.at_level(logging.WARNING, logger="featurematching_amd"):
        supervision.compute_supervision_coarse(data, dense_gt=True)
    assert len([r for r in caplog.records if "No groundtruth coarse match" in r.getMessage()]) == 1
    for key in ('spv_b_ids', 'spv_i_ids', 'spv_j_ids'):
        assert data[key].dtype == torch.int64 and data[key].tolist() == [0], key
    assert data['conf_matrix_gt'].shape == (1, 96, 96) and not data['conf_matrix_gt'].any()
    data['spv_i_ids'][0] = 7                                 # three tensors, not one under three names
    assert data['spv_b_ids'].tolist() == [0] and data['spv_j_ids'].tolist() == [0]


def test_another_coarse_resolution_is_refused(golden):
    data = _data(_case(golden, (8, 12), 5), (8, 12))
    with pytest.raises(ValueError, match="resolution"):
        supervision.compute_supervision_coarse(data, {'MODULE': {'RESOLUTION': (16, 4)}})
    assert 'spv_i_ids' not in data


def test_data_preprocess_has_no_cpu_fallback():
    img = torch.zeros(1, 1, 64, 96)
    with pytest.raises(RuntimeError, match="GPU"):
        supervision.data_preprocess({'image0': img, 'image1': img, 'origin_kp0': torch.ones(1, 3, 2), 'origin_kp1': torch.ones(1, 3, 2)})
    with pytest.raises(ValueError):
        supervision.data_preprocess({'image0': img, 'image1': img, 'origin_kp0': torch.ones(2, 3, 2), 'origin_kp1': torch.ones(2, 3, 2)})


@pytest.mark.parametrize("bad", [[-0.5, 3.0], [96.0, 3.0], [3.0, 64.0], [float("nan"), 3.0]])
def test_restatement_knows_a_point_outside_its_grid(bad):
    good = np.array([[5.0, 5.0], [40.0, 40.0]], np.float32)
    assert sref.in_range(good, good, (8, 12), (8, 12))
    for which in (0, 1):
        kps = [good.copy(), good.copy()]
        kps[which][1] = bad
        assert not sref.in_range(*kps, (8, 12), (8, 12))


@pytest.mark.parametrize("hw,k", CASES)
def test_fine_loss_restatement_and_cpu_branch(golden, hw, k):
    g = _case(golden, hw, k)
    want = float(g["loss_f64"])
    loss, d0, d1 = sref.fine_loss(g["mkpts0_f"], g["mkpts1_f"], g["expec_f_gt_0"], g["expec_f_gt_1"])
    assert abs(loss - want) <= 1e-13 * abs(want)
    for got, key in ((d0, "g0_64"), (d1, "g1_64")):
        assert np.abs(got - g[key]).max() <= 1e-13 * np.abs(g[key]).max() and not got[:, 2].any()
    # the loss in torch ops (FineLoss's CPU branch, the GPU tests' yardstick): float64 is the reference's float64 ...
    a0 = torch.as_tensor(g["mkpts0_f"], dtype=torch.float64).requires_grad_(True)
    a1 = torch.as_tensor(g["mkpts1_f"], dtype=torch.float64).requires_grad_(True)
    val = modules.fine_loss_torch(a0, a1, torch.as_tensor(g["expec_f_gt_0"]).double(), torch.as_tensor(g["expec_f_gt_1"]).double())
    val.backward()
    assert abs(val.item() - want) <= 1e-13 * abs(want)
    assert np.abs(a0.grad.numpy() - g["g0_64"]).max() <= 1e-13 * np.abs(g["g0_64"]).max()
    assert np.abs(a1.grad.numpy() - g["g1_64"]).max() <= 1e-13 * np.abs(g["g1_64"]).max()
    # ... and the module in float32 is the reference in float32
    data = {'mkpts0_f': torch.as_tensor(g["mkpts0_f"]), 'mkpts1_f': torch.as_tensor(g["mkpts1_f"]),
            'expec_f_gt_0': torch.as_tensor(g["expec_f_gt_0"]), 'expec_f_gt_1': torch.as_tensor(g["expec_f_gt_1"])}
    got = modules.FineLoss()(data)
    assert got.dtype == torch.float32 and _close(got.item(), want, g["loss_f32"]), (got.item(), want)


def test_fine_loss_cpu_branch_edges():
    gt = torch.tensor([[3.0, 4.0], [0.0, 9.0]])
    zero = modules.fine_loss_torch(torch.zeros(2, 3, requires_grad=True), torch.ones(2, 3), gt, gt)
    assert zero.item() == 0 and zero.dim() == 0
    none = modules.fine_loss_torch(torch.ones(2, 3), torch.ones(2, 3), torch.zeros(2, 2), gt)
    assert torch.isnan(none)
    loss, d0, _ = sref.fine_loss(np.ones((2, 3)), np.ones((2, 3)), np.zeros((2, 2)), gt.numpy())
    assert np.isnan(loss) and not d0.any()


def _loss_data(g, hw, k):
    f0, f1 = synth.coarse_descriptors(SEED + k, 1, hw[0] * hw[1], 64, "borderline")
    assert np.allclose(g["desc_sums"], [f0.astype(np.float64).sum(), f1.astype(np.float64).sum()], rtol=0, atol=1e-9)
    data = _data(g, hw)
    supervision.compute_supervision_coarse(data, dense_gt=True)
    data.update({'b_ids': torch.as_tensor(g["b_ids"]), 'i_ids': torch.as_tensor(g["i_ids"]), 'j_ids': torch.as_tensor(g["j_ids"])})
    supervision.compute_supervision_fine(data)
    data.update({'conf_matrix': orc.conf_matrix(torch.as_tensor(f0), torch.as_tensor(f1), 0.1),
                 'mkpts0_f': torch.as_tensor(g["mkpts0_f"]).requires_grad_(True),
                 'mkpts1_f': torch.as_tensor(g["mkpts1_f"]).requires_grad_(True)})
    return data


@pytest.mark.parametrize("hw,k", CASES)
def test_loss_module_cpu_branch_against_the_references_forward(golden, hw, k):
    g = _case(golden, hw, k)
    data = _loss_data(g, hw, k)
    loss = modules.Loss(CONFIG).train()
    assert loss(data) is None
    assert data['loss'].requires_grad and data['loss'].dim() == 0
    assert _close(data['loss'].item(), float(g["fwd64_loss"]), g["fwd_train_loss"])
    sc = data['loss_scalars']
    assert tuple(sc) == SCALARS
    for s, dt in zip(SCALARS, g["scalar_dtypes"]):
        assert sc[s].dim() == 0 and sc[s].device.type == "cpu" and str(sc[s].dtype) == dt and not sc[s].requires_grad, s
    assert _close(sc['loss'].item(), float(g["fwd64_loss"]), g["fwd_train_loss"])
    assert _close(sc['loss_c'].item(), float(g["fwd64_loss_c"]), g["fwd_train_loss_c"])
    assert _close(sc['loss_f'].item(), float(g["loss_f64"]), g["fwd_train_loss_f"])
    assert sc['loss_pose'].item() == 0
    data['loss'].backward()
    assert data['mkpts0_f'].grad.abs().max() > 0 and not data['mkpts0_f'].grad[:, 2].any()
    loss.eval()
    loss(data)
    assert data['loss_scalars']['loss_f'].item() == 1.0 == float(g["fwd_eval_loss_f"])
    assert str(data['loss_scalars']['loss_f'].dtype) == "torch.float32"
    assert _close(data['loss'].item(), float(g["fwd64_loss"]), g["fwd_eval_loss"])


COARSE = {"focal": ("focal", False), "focal_sparse": ("focal", True), "xent": ("cross_entropy", False),
          "xent_sparse": ("cross_entropy", True)}


@pytest.mark.parametrize("form", list(COARSE))
@pytest.mark.parametrize("hw,k", CASES)
def test_dense_coarse_loss_in_every_form_against_the_references(golden, hw, k, form):
    """coarse_loss_torch (the coarse term of Loss without CoarseMatching's statistics): focal and cross entropy, dense and
    sparse supervision, with positives and without - float64 to rounding, gradients by their row and column sums,
    float32 under the loss bar; and the same through the module"""
    g = _case(golden, hw, k)
    coarse_type, sparse = COARSE[form]
    data = _loss_data(g, hw, k)
    args = (coarse_type, 0.25, 2.0, 1.0, 1.0, sparse)
    for tag, gt in (("", data['conf_matrix_gt']), ("nopos_", torch.zeros_like(data['conf_matrix_gt']))):
        want, ref32 = float(g[f"coarse_{tag}{form}_loss64"]), g[f"coarse_{tag}{form}_loss32"]
        c64 = data['conf_matrix'].double().requires_grad_(True)
        # (float64 of the float32 matrix, where the fixture's is computed in float64: equal to float32 accuracy only)
        assert _close(modules.coarse_loss_torch(c64, gt.double(), *args).item(), want, ref32), (form, tag)
        assert _close(modules.coarse_loss_torch(data['conf_matrix'], gt, *args).item(), want, ref32), (form, tag)
    f0, f1 = synth.coarse_descriptors(SEED + k, 1, hw[0] * hw[1], 64, "borderline")
    c64 = orc.conf_matrix(torch.as_tensor(f0).double(), torch.as_tensor(f1).double(), 0.1).requires_grad_(True)
    val = modules.coarse_loss_torch(c64, data['conf_matrix_gt'].double(), *args)
    want = float(g[f"coarse_{form}_loss64"])
    assert abs(val.item() - want) <= 1e-12 * abs(want)
    val.backward()
    for got, key in ((c64.grad.sum(2)[0], "grow"), (c64.grad.sum(1)[0], "gcol")):
        ref = g[f"coarse_{form}_{key}"]
        assert np.abs(got.numpy() - ref).max() <= 1e-12 * np.abs(ref).max(), (form, key)
    cfg = {'module': {'loss': dict(CONFIG['module']['loss'], coarse_type=coarse_type), 'match_coarse': {'sparse_spvs': sparse}}}
    loss = modules.Loss(cfg).train()
    loss(data)
    assert _close(data['loss_scalars']['loss_c'].item(), want, g[f"coarse_{form}_loss32"])
    with pytest.raises(ValueError):
        modules.coarse_loss_torch(c64, data['conf_matrix_gt'], 'hinge', 0.25, 2.0, 1.0, 1.0, False)


def test_pose_losses_are_not_implemented():
    for flag in ('old', 'new'):
        cfg = {'module': {'loss': dict(CONFIG['module']['loss'], pose_loss_cal_flag=flag), 'match_coarse': {'sparse_spvs': False}}}
        with pytest.raises(NotImplementedError):
            modules.Loss(cfg)
