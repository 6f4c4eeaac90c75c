"""One tiny training-mode chain of the drop-in pieces around the matcher (lightning_new.py:216-230 without Matcher):
data_preprocess -> compute_supervision_coarse -> CoarseMatching(loss_stats=True) -> FinePreprocess -> the torch fine
layers -> FineMatching -> compute_supervision_fine -> Loss -> backward().  Grid 12 x 16, C = 64, fine maps 48 x 64, W = 7.
The fine term is held to the loss bar of tests/test_gpu_fine_loss.py (profiles/fine_loss_accuracy.txt)."""
import pytest
import torch

from featurematching_amd import modules, supervision, synth
from featurematching_amd.transformer import LocalFeatureTransformer

import supervision_ref as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2 * 1.15e-7        # profiles/fine_loss_accuracy.txt: the largest e_ref / |loss64| over the inputs of tests/test_gpu_fine_loss.py
HC, WC, HF, WF, W = 12, 16, 48, 64, 7
LOSS_CFG = {'fine_correct_thr': 1.0, 'pos_weight': 1.0, 'neg_weight': 1.0, 'pose_loss_cal_flag': False, 'coarse_type': 'focal',
            'focal_alpha': 0.25, 'focal_gamma': 2.0, 'coarse_weight': 1.0, 'fine_weight': 0.25}
CONFIG = {'module': {'loss': LOSS_CFG, 'match_coarse': {'sparse_spvs': False}}}


def test_training_chain_loss_and_gradients():
    seed = 33
    c0, c1 = synth.coarse_descriptors(seed, 1, HC * WC, 64, "borderline")
    f0, f1 = synth.fine_maps(seed, 1, 64, HF, WF)
    leaves = [torch.as_tensor(a, device=DEV).requires_grad_(True) for a in (c0, c1, f0, f1)]
    img = torch.zeros(1, 1, HC * 8, WC * 8, device=DEV)
    data = {'image0': img, 'image1': img, 'hw0_i': (HC * 8, WC * 8), 'hw1_i': (HC * 8, WC * 8), 'hw0_c': (HC, WC),
            'hw1_c': (HC, WC), 'hw0_f': (HF, WF), 'hw1_f': (HF, WF),
            'origin_kp0': torch.as_tensor(sref.points(seed, 300, (HC, WC), 0), device=DEV)[None],
            'origin_kp1': torch.as_tensor(sref.points(seed, 300, (HC, WC), 1), device=DEV)[None]}
    torch.manual_seed(seed)
    cm = modules.CoarseMatching({'thr': 0.2, 'border_rm': 2, 'dsmax_temperature': 0.1}, loss_stats=True)
    fp = modules.FinePreprocess({'fine_concat_coarse_feat': True, 'fine_window_size': W, 'coarse': {'d_model': 64},
                                 'fine': {'d_model': 64}}).to(DEV)
    tf = LocalFeatureTransformer(dict(d_model=64, nhead=8, layer_names=['self', 'cross'], attention='linear')).to(DEV)
    fm = modules.FineMatching(window=W).to(DEV)
    loss = modules.Loss(CONFIG)
    for mod in (cm, fp, tf, fm, loss):
        mod.train()

    supervision.data_preprocess(data)
    supervision.compute_supervision_coarse(data)
    m = data['spv_i_ids'].shape[0]
    assert 100 < m < 192 and 'conf_matrix_gt' not in data
    cm(leaves[0], leaves[1], data)
    assert 'conf_matrix' not in data and torch.equal(data['i_ids'], data['spv_i_ids'])
    w0, w1 = fp(leaves[2], leaves[3], leaves[0], leaves[1], data)
    w0, w1 = tf(w0, w1)
    fm(w0, w1, data)
    supervision.compute_supervision_fine(data)
    assert torch.equal(data['expec_f_gt_1'], data['fine_kp1'][0])            # the j are distinct: every row its own point
    assert (data['expec_f_gt_0'][:, 0] != 0).all()
    loss(data)

    sc = data['loss_scalars']
    assert tuple(sc) == ("loss_c", "loss_f", "loss_pose", "loss")
    assert all(v.dim() == 0 and v.device.type == "cpu" and v.dtype == torch.float32 for v in sc.values())
    # loss = coarse_weight * CoarseLoss + fine_weight * fine loss: the same float32 expression from the parts ...
    loss_c = modules.CoarseLoss(LOSS_CFG)(data)                              # (the same bits on every run)
    assert sc['loss_c'].item() == loss_c.item() and sc['loss_pose'].item() == 0
    total = sc['loss_c'] * LOSS_CFG['coarse_weight'] + sc['loss_f'] * LOSS_CFG['fine_weight']
    assert data['loss'].item() == total.item() == sc['loss'].item()
    # ... with the fine part recomputed in float64 from the chain's own mkpts*_f
    args = (data['mkpts0_f'].detach(), data['mkpts1_f'].detach(), data['expec_f_gt_0'], data['expec_f_gt_1'])
    l64 = modules.fine_loss_torch(*(a.double() for a in args)).item()
    l32 = modules.fine_loss_torch(*args).item()
    print(f"ACC  chain    loss64 {l64:.9e}  e_ref/|loss64| {abs(l32 - l64) / l64:.3e}  e_hip/|loss64| "
          f"{abs(sc['loss_f'].item() - l64) / l64:.3e}")
    assert l64 > 0 and abs(sc['loss_f'].item() - l64) <= 4 * abs(l32 - l64) + FLOOR * l64
    # (6e-8: the float32 rounding, 2^-24, of the sum itself)
    want = loss_c.item() * LOSS_CFG['coarse_weight'] + l64 * LOSS_CFG['fine_weight']
    assert abs(data['loss'].item() - want) <= LOSS_CFG['fine_weight'] * (4 * abs(l32 - l64) + FLOOR * l64) + 6e-8 * want

    data['loss'].backward()
    for name, t in zip(("feat_c0", "feat_c1", "feat_f0", "feat_f1"), leaves):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().max().item() > 0, name
    for mod in (fp, tf, fm):
        for p in mod.parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all()
