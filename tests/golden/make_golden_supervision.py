#!/usr/bin/env python3
"""Writes tests/golden/supervision_small.npz from the REFERENCE's own data_preprocess (datasets/data_preprocessing.py),
compute_supervision_coarse / compute_supervision_fine (network/utils/supervision_new.py), Loss.compute_fine_loss and
Loss.forward (losses/loss.py), all unmodified.

    python tests/golden/make_golden_supervision.py PATH_TO_THE_REFERENCE_TREE

Needs no GPU.  The three files import loguru, cv2 and kornia, none of which the executed code uses beyond
logger.warning: stand-in modules in sys.modules serve the imports.

Cases {grid}_k{K}: grids 8x12 and 12x16 (equal for both images, 8-pixel cells), K in {1, 5, 300} correspondences drawn
uniformly and independently in both images (tests/supervision_ref.points: at K = 300 most cells hold several
correspondences, and many survivors share an image-0 cell).  Per case:
    kp0, kp1                          float32 [K, 2]: the input (origin_kp0 / origin_kp1 without the batch dimension)
    coarse_kp*, fine_kp*, lists_f*, fine_mtx_*   data_preprocess's outputs, as written (leading dimension 1)
    spv_i_ids, spv_j_ids              compute_supervision_coarse's ids.  With ONE survivor the reference's .squeeze() leaves
                                      0-dim ids and its len(i_ids) raises TypeError after conf_matrix_gt was written:
                                      coarse_raised = 1, and the ids stored are those 0-dim ids reshaped to [1]
    gt_pos                            int64 [K', 2]: where conf_matrix_gt is 1
    b_ids, i_ids, j_ids               the ids in use: the supervision ids followed by 7 random cell pairs, most of them
                                      unsupervised in one image or both (rows the fine loss must leave out)
    expec_f_gt_0, expec_f_gt_1        compute_supervision_fine's outputs
    mkpts0_f, mkpts1_f                float32 [M, 3]: the fine stage's stand-in output (supervision_ref.fine_inputs)
    loss_f32, loss_f64                compute_fine_loss in training mode on float32 / float64 inputs
    g0_64, g1_64                      float64 autograd's gradient of loss_f64 w.r.t. mkpts0_f / mkpts1_f
    desc_sums                         float64 [2]: sums of the descriptors behind conf_matrix (synth regenerates them:
                                      coarse_descriptors(SEED, 1, L, 64, 'borderline'), oracle.matcher_ref.conf_matrix)
    fwd_{train,eval}_{loss,loss_c,loss_f,loss_pose}   Loss.forward: data['loss'] and data['loss_scalars'] (focal, dense
                                      supervision, coarse_weight 1, fine_weight 0.25)
    fwd64_loss, fwd64_loss_c          the training-mode forward on float64 inputs
    coarse_{form}_loss32/_loss64      Loss.compute_coarse_loss(conf_matrix, conf_matrix_gt) alone on float32 / float64
                                      inputs, form in focal, focal_sparse (sparse_spvs), xent, xent_sparse;
    coarse_{form}_grow/_gcol          row and column sums of float64 autograd's gradient w.r.t. conf_matrix;
    coarse_nopos_{form}_loss32/_loss64   the same losses with an all-zero conf_matrix_gt (no positive)
    scalar_dtypes                     the dtypes of loss_scalars' four entries, as strings
Data only."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from featurematching_amd import synth          # noqa: E402
from oracle import matcher_ref as orc          # noqa: E402
import supervision_ref as sref                 # noqa: E402

GRIDS = ((8, 12), (12, 16))
KS = (1, 5, 300)
SEED = 47
N_EXTRA = 7
CONFIG = {'module': {'loss': {'fine_correct_thr': 1.0, 'pos_weight': 1.0, 'neg_weight': 1.0, 'pose_loss_cal_flag': False,
                              'coarse_type': 'focal', 'focal_alpha': 0.25, 'focal_gamma': 2.0, 'coarse_weight': 1.0,
                              'fine_weight': 0.25},
                     'match_coarse': {'sparse_spvs': False}}}
SCALARS = ("loss_c", "loss_f", "loss_pose", "loss")
COARSE = {"focal": ("focal", False), "focal_sparse": ("focal", True), "xent": ("cross_entropy", False),
          "xent_sparse": ("cross_entropy", True)}


def case_name(hw, k):
    return f"g{hw[0]}x{hw[1]}_k{k}"


def case_inputs(hw, k):
    seed = SEED + 1000 * hw[0] + k
    return sref.points(seed, k, hw, 0), sref.points(seed, k, hw, 1)


def extra_ids(hw, k):
    h = synth.hash_u64(SEED + 1000 * hw[0] + k, 5, 2 * N_EXTRA) % np.uint64(hw[0] * hw[1])
    return h[:N_EXTRA].astype(np.int64), h[N_EXTRA:].astype(np.int64)


def conf_matrix(hw, k, dtype=torch.float32):
    l = hw[0] * hw[1]
    f0, f1 = synth.coarse_descriptors(SEED + k, 1, l, 64, "borderline")
    return orc.conf_matrix(torch.as_tensor(f0, dtype=dtype), torch.as_tensor(f1, dtype=dtype), 0.1), f0, f1


def reference(ref_root):
    warn = types.SimpleNamespace(warning=print)
    sys.modules.setdefault("loguru", types.SimpleNamespace(logger=warn))
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    kornia, kutils = types.ModuleType("kornia"), types.ModuleType("kornia.utils")
    kutils.create_meshgrid = None
    kornia.utils = kutils
    sys.modules.setdefault("kornia", kornia)
    sys.modules.setdefault("kornia.utils", kutils)
    sys.path.insert(0, ref_root)
    from datasets.data_preprocessing import data_preprocess
    from network.utils.supervision_new import compute_supervision_coarse, compute_supervision_fine
    from losses.loss import Loss
    return data_preprocess, compute_supervision_coarse, compute_supervision_fine, Loss


def main(ref_root):
    data_preprocess, spv_coarse, spv_fine, Loss = reference(ref_root)
    out = {}
    for hw in GRIDS:
        for k in KS:
            c = case_name(hw, k) + "_"
            kp0, kp1 = case_inputs(hw, k)
            img = torch.zeros(1, 1, hw[0] * 8, hw[1] * 8)
            data = {'image0': img, 'image1': img, 'origin_kp0': torch.as_tensor(kp0)[None],
                    'origin_kp1': torch.as_tensor(kp1)[None], 'pair_names': c}
            out[c + "kp0"], out[c + "kp1"] = kp0, kp1
            data_preprocess(data)
            for key in ('coarse_kp0', 'coarse_kp1', 'fine_kp0', 'fine_kp1', 'lists_f0', 'lists_f1', 'fine_mtx_0', 'fine_mtx_1'):
                out[c + key] = data[key].numpy().copy()
            raised = 0
            try:
                spv_coarse(data, {'MODULE': {'RESOLUTION': (8, 2)}})
                i_spv, j_spv = data['spv_i_ids'], data['spv_j_ids']
            except TypeError:                    # len() of a 0-d tensor: one survivor (see above)
                raised = 1
                i_spv, j_spv = data['lists_f0'].squeeze().long().reshape(1), data['lists_f1'].squeeze().long().reshape(1)
            out[c + "coarse_raised"] = np.int64(raised)
            out[c + "spv_i_ids"], out[c + "spv_j_ids"] = i_spv.numpy().copy(), j_spv.numpy().copy()
            out[c + "gt_pos"] = torch.nonzero(data['conf_matrix_gt'][0]).numpy()
            xi, xj = extra_ids(hw, k)
            i_ids, j_ids = torch.cat([i_spv, torch.as_tensor(xi)]), torch.cat([j_spv, torch.as_tensor(xj)])
            data.update({'b_ids': torch.zeros_like(i_ids), 'i_ids': i_ids, 'j_ids': j_ids})
            spv_fine(data)
            g0, g1 = data['expec_f_gt_0'], data['expec_f_gt_1']
            e0, e1 = sref.fine_inputs(SEED + k, g0.numpy(), g1.numpy())
            for key, v in (("b_ids", data['b_ids']), ("i_ids", i_ids), ("j_ids", j_ids), ("expec_f_gt_0", g0),
                           ("expec_f_gt_1", g1)):
                out[c + key] = v.numpy().copy()
            out[c + "mkpts0_f"], out[c + "mkpts1_f"] = e0, e1
            loss = Loss(CONFIG).train()
            out[c + "loss_f32"] = np.float32(loss.compute_fine_loss(torch.as_tensor(e0), torch.as_tensor(e1), g0, g1).item())
            a0 = torch.as_tensor(e0, dtype=torch.float64).requires_grad_(True)
            a1 = torch.as_tensor(e1, dtype=torch.float64).requires_grad_(True)
            val = loss.compute_fine_loss(a0, a1, g0.double(), g1.double())
            val.backward()
            out[c + "loss_f64"] = np.float64(val.item())
            out[c + "g0_64"], out[c + "g1_64"] = a0.grad.numpy().copy(), a1.grad.numpy().copy()
            conf, f0, f1 = conf_matrix(hw, k)
            out[c + "desc_sums"] = np.array([f0.astype(np.float64).sum(), f1.astype(np.float64).sum()])
            data.update({'conf_matrix': conf, 'mkpts0_f': torch.as_tensor(e0), 'mkpts1_f': torch.as_tensor(e1)})
            for mode in ("train", "eval"):
                loss.train(mode == "train")
                loss(data)
                out[c + f"fwd_{mode}_loss"] = np.float32(data['loss'].item())
                for s in SCALARS:
                    v = data['loss_scalars'][s]
                    assert v.dim() == 0 and v.device.type == "cpu"
                    out[c + f"fwd_{mode}_{s}"] = np.float32(v.item())
                out[c + "scalar_dtypes"] = np.array([str(data['loss_scalars'][s].dtype) for s in SCALARS])
            d64 = dict(data)                     # the same forward on float64 inputs (training mode)
            d64.update({'conf_matrix': conf_matrix(hw, k, torch.float64)[0], 'mkpts0_f': torch.as_tensor(e0).double(),
                        'mkpts1_f': torch.as_tensor(e1).double(), 'expec_f_gt_0': g0.double(), 'expec_f_gt_1': g1.double()})
            loss.train()
            loss(d64)
            out[c + "fwd64_loss"] = np.float64(d64['loss'].item())
            out[c + "fwd64_loss_c"] = np.float64(d64['loss_scalars']['loss_c'].item())
            # Loss.compute_coarse_loss alone, in every form it has, with and without a positive
            for name, (coarse_type, sparse) in COARSE.items():
                cfg = {'module': {'loss': dict(CONFIG['module']['loss'], coarse_type=coarse_type),
                                  'match_coarse': {'sparse_spvs': sparse}}}
                closs = Loss(cfg).train()
                for tag, gt in (("", data['conf_matrix_gt']), ("nopos_", torch.zeros_like(data['conf_matrix_gt']))):
                    out[c + f"coarse_{tag}{name}_loss32"] = np.float32(closs.compute_coarse_loss(conf, gt).item())
                    c64 = conf_matrix(hw, k, torch.float64)[0].requires_grad_(True)
                    val = closs.compute_coarse_loss(c64, gt.double())
                    out[c + f"coarse_{tag}{name}_loss64"] = np.float64(val.item())
                    if val.requires_grad and tag == "":
                        val.backward()
                        out[c + f"coarse_{name}_grow"] = c64.grad.sum(2)[0].numpy().copy()
                        out[c + f"coarse_{name}_gcol"] = c64.grad.sum(1)[0].numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", "supervision_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for key, v in out.items():
        if "loss" in key:
            print(key, repr(v))
        if key.endswith("spv_i_ids"):
            print(key, len(v), "survivors,", len(v) - len(np.unique(v)), "repeated i")


if __name__ == "__main__":
    main(sys.argv[1])
