"""The reference's supervision steps with their names, keys and dtypes, around the matcher of a training step
(lightning_new.py:216-230: data_preprocess -> compute_supervision_coarse -> matcher -> compute_supervision_fine -> Loss):

    data_preprocess(data)                                     (datasets/data_preprocessing.py:31-64)
    compute_supervision_coarse(data, config=None, dense_gt=False)  (network/utils/supervision_new.py:12-47)
    compute_supervision_fine(data)                            (network/utils/supervision_new.py:49-58)

data_preprocess is ops.supervise_matches (HIP, one host read of the survivor count; the reference copies the
correspondences to the host and back around two np.unique calls) and, like it, needs its input on the GPU.  The other two
are index arithmetic on whatever device the data lives on.
"""
from __future__ import annotations

import logging

import torch

from . import ops

logger = logging.getLogger("featurematching_amd")

CELL = 8      # the reference's coarse resolution, hard-coded in data_preprocessing.py


@torch.no_grad()
def data_preprocess(data: dict) -> None:
    """Reads origin_kp0 / origin_kp1 [1, K, 2] and the shapes of image0 / image1; writes origin_kp*, coarse_kp*, fine_kp*
    [1, K', 2], lists_f* [1, K'] and fine_mtx_0 [1, L, 2] / fine_mtx_1 [1, S, 2].  N = 1, as the reference.  Each image
    is gridded with its own width (the reference uses image 0's for both: the same for equal image sizes)."""
    kp0, kp1 = data['origin_kp0'], data['origin_kp1']
    if kp0.dim() != 3 or kp0.shape[0] != 1 or kp1.shape != kp0.shape:
        raise ValueError("data_preprocess handles one pair: origin_kp0 / origin_kp1 must both be [1, K, 2]")
    hw0_c = (data['image0'].shape[-2] // CELL, data['image0'].shape[-1] // CELL)
    hw1_c = (data['image1'].shape[-2] // CELL, data['image1'].shape[-1] // CELL)
    out = ops.supervise_matches(kp0[0], kp1[0], hw0_c, hw1_c, CELL)
    data.update({'origin_kp0': kp0, 'origin_kp1': kp1})
    for key in ('coarse_kp0', 'coarse_kp1', 'fine_kp0', 'fine_kp1', 'fine_mtx_0', 'fine_mtx_1', 'lists_f0', 'lists_f1'):
        data[key] = out[key][None]


def _cell_ids(coarse_kp, w_c: int):
    """flat cell ids [K'] (int64) of cell corners [1, K', 2] in pixels on a grid w_c cells wide"""
    cx, cy = torch.div(coarse_kp[0], CELL, rounding_mode='floor').long().unbind(-1)
    return cx + cy * w_c


@torch.no_grad()
def compute_supervision_coarse(data: dict, config=None, dense_gt: bool = False) -> None:
    """Writes spv_b_ids, spv_i_ids, spv_j_ids (int64 [K']) from the cell corners data_preprocess left, and spv_fine_0 /
    spv_fine_1 = fine_kp0 / fine_kp1.  Without a correspondence the ids are the reference's stand-in [0], [0], [0]
    (supervision_new.py:37-41), with one warning.  `config`: the reference's; its config['MODULE']['RESOLUTION'][0] must
    be the 8 pixels data_preprocess grids with.  The dense data['conf_matrix_gt'] [1, L, S] (ones at the supervised
    entries) is written only with dense_gt=True: CoarseLoss reads the ids."""
    if config is not None and config['MODULE']['RESOLUTION'][0] != CELL:
        raise ValueError(f"coarse resolution {config['MODULE']['RESOLUTION'][0]}: data_preprocess grids with {CELL}-pixel cells")
    device = data['image0'].device
    (h0, w0), (h1, w1) = ((img.shape[-2] // CELL, img.shape[-1] // CELL) for img in (data['image0'], data['image1']))
    i_ids, j_ids = _cell_ids(data['coarse_kp0'], w0).to(device), _cell_ids(data['coarse_kp1'], w1).to(device)
    b_ids = torch.zeros_like(i_ids)
    if dense_gt:
        data['conf_matrix_gt'] = torch.zeros(1, h0 * w0, h1 * w1, device=device)
        data['conf_matrix_gt'][b_ids, i_ids, j_ids] = 1
    if i_ids.shape[0] == 0:
        logger.warning(f"No groundtruth coarse match found for: {data.get('pair_names')}")
        b_ids, i_ids, j_ids = (torch.zeros(1, dtype=torch.int64, device=device) for _ in range(3))
    data.update(spv_b_ids=b_ids, spv_i_ids=i_ids, spv_j_ids=j_ids, spv_fine_0=data['fine_kp0'], spv_fine_1=data['fine_kp1'])


@torch.no_grad()
def compute_supervision_fine(data: dict) -> None:
    """expec_f_gt_0 / expec_f_gt_1 [M, 2]: the ground-truth point of every match in use, looked up in the per-cell
    tables fine_mtx_0 [N, L, 2] / fine_mtx_1 [N, S, 2] by (b_ids, i_ids) / (b_ids, j_ids); zero where the cell has none."""
    for side, ids in ((0, 'i_ids'), (1, 'j_ids')):
        data[f'expec_f_gt_{side}'] = data[f'fine_mtx_{side}'][data['b_ids'], data[ids]]
