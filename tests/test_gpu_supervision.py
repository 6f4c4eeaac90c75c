"""The supervision kernels on the GPU (ops.supervise_matches, fm_supervise_matches) and the three drop-in functions of
featurematching_amd/supervision.py: every output equals the NumPy restatement (tests/supervision_ref.py, pinned to the
reference's fixture by tests/test_supervision_ref.py) exactly - ids as integers, floats bit for bit."""
import functools
import logging
import os

import numpy as np
import pytest
import torch

from featurematching_amd import _lib, ops, supervision

import supervision_ref as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "supervision_small.npz")
# K: none, one, a few, a wave, a wave + 1, several workgroups of the marking kernel, many per cell on every grid
KS = (0, 1, 5, 64, 65, 1000, 20000)
# 2x3: six cells; 8x12: the fixture's; 60x80: S = 4800 spans five workgroups of the scan; unequal grids
GRIDS = {"2x3": ((2, 3), (2, 3)), "8x12": ((8, 12), (8, 12)), "60x80": ((60, 80), (60, 80)), "uneq": ((15, 17), (11, 13))}
FLOAT_KEYS = tuple(k for k in sref.OUT_KEYS if not k.endswith("_ids"))


@functools.lru_cache(maxsize=None)
def _points(grid, k):
    hw0, hw1 = GRIDS[grid]
    return sref.points(900 + k, k, hw0, 0), sref.points(900 + k, k, hw1, 1)


@functools.lru_cache(maxsize=None)
def _reference(grid, k):
    return sref.supervise(*_points(grid, k), *GRIDS[grid])


def _hip(kp0, kp1, hw0, hw1):
    return ops.supervise_matches(torch.as_tensor(kp0, device=DEV), torch.as_tensor(kp1, device=DEV), hw0, hw1)


def _assert_same(got, want, what):
    for key in sref.OUT_KEYS:
        g = got[key].cpu().numpy()
        assert g.shape == want[key].shape and g.dtype == want[key].dtype, (what, key, g.shape, want[key].shape)
        if key in FLOAT_KEYS:
            assert np.array_equal(g.view(np.uint32), want[key].view(np.uint32)), (what, key)
        else:
            assert np.array_equal(g, want[key]), (what, key)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_every_output_equals_the_restatement(grid, k):
    want = _reference(grid, k)
    if k >= 1000:       # many correspondences per cell; and (but on six cells) image-0 cells shared by several survivors
        n = len(want["i_ids"])
        assert n < k and (grid == "2x3" or n - len(np.unique(want["i_ids"])) > 20)
    _assert_same(_hip(*_points(grid, k), *GRIDS[grid]), want, (grid, k))


def test_heavy_contention_the_first_occurrence_wins():
    """1000 correspondences into six cells: the atomicMin of the input index decides, whatever order they arrive in"""
    kp0, kp1 = _points("2x3", 1000)
    got = _hip(kp0, kp1, (2, 3), (2, 3))
    assert got["j_ids"].tolist() == [0, 3, 1, 4, 2, 5]                       # (cx1, cy1) order, not the order of j
    c1 = sref.cells(kp1).astype(np.int64)
    for t, j in enumerate(got["j_ids"].tolist()):
        first = int(np.nonzero(c1[:, 0] + 3 * c1[:, 1] == j)[0][0])
        assert np.array_equal(got["fine_kp1"][t].cpu().numpy(), kp1[first]) and np.array_equal(got["fine_kp0"][t].cpu().numpy(), kp0[first])


def test_points_on_cell_edges():
    """x = 8.0 is the first pixel of cell 1, the float just below it the last of cell 0; likewise at the grid's far edge"""
    below = np.nextafter(np.float32(8), np.float32(0))
    far = np.nextafter(np.float32(96), np.float32(0))
    kp1 = np.array([[8.0, 8.0], [below, below], [8.0, below], [below, 8.0], [far, 0.0], [0.0, np.nextafter(np.float32(64), np.float32(0))]], np.float32)
    kp0 = kp1[::-1].copy()
    want = sref.supervise(kp0, kp1, (8, 12), (8, 12))
    assert want["j_ids"].tolist() == [0, 12, 84, 1, 13, 11]
    _assert_same(_hip(kp0, kp1, (8, 12), (8, 12)), want, "edges")


def test_repeated_image0_cells_the_last_survivor_wins():
    """four image-1 cells, all from image-0 cell 5: fine_mtx_0[5] is the point of the survivor with the largest t"""
    kp1 = np.array([[50.0, 9.0], [3.0, 3.0], [20.0, 40.0], [9.0, 3.0], [51.0, 10.0]], np.float32)
    kp0 = np.array([[41.0, 1.0], [42.0, 2.0], [43.0, 3.0], [44.0, 4.0], [45.0, 5.0]], np.float32)
    got = _hip(kp0, kp1, (8, 12), (8, 12))
    assert got["i_ids"].tolist() == [5, 5, 5, 5] and got["j_ids"].tolist() == [0, 1, 62, 18]
    assert got["fine_mtx_0"][5].tolist() == [41.0, 1.0] and int((got["fine_mtx_0"] != 0).any(1).sum()) == 1
    _assert_same(got, sref.supervise(kp0, kp1, (8, 12), (8, 12)), "repeated i")


def test_two_runs_give_equal_outputs():
    for grid, k in (("8x12", 20000), ("60x80", 20000)):
        a, b = _hip(*_points(grid, k), *GRIDS[grid]), _hip(*_points(grid, k), *GRIDS[grid])
        for key in sref.OUT_KEYS:
            assert torch.equal(a[key], b[key]), (grid, key)


@pytest.mark.parametrize("bad", [[96.0, 3.0], [3.0, 64.0], [-0.5, 3.0], [3.0, -1e-3], [float("nan"), 3.0], [float("inf"), 3.0],
                                 [-1e-45, 3.0]])     # the smallest negative denormal: divides to -0, and is still outside
def test_a_point_outside_its_grid_raises(bad):
    kp0, kp1 = _points("8x12", 65)
    for which in (0, 1):
        kps = [kp0.copy(), kp1.copy()]
        kps[which][40] = bad
        assert not sref.in_range(*kps, (8, 12), (8, 12))
        with pytest.raises(_lib.FMatchError) as err:
            _hip(*kps, (8, 12), (8, 12))
        assert err.value.status == _lib.FM_E_RANGE
    _hip(kp0, kp1, (8, 12), (8, 12))                                        # the next call is unaffected


def test_argument_checks():
    kp = torch.zeros(4, 2, device=DEV)
    with pytest.raises(ValueError):
        ops.supervise_matches(kp, kp[:3], (8, 12), (8, 12))
    with pytest.raises(ValueError):
        ops.supervise_matches(kp, kp, (0, 12), (8, 12))
    with pytest.raises(RuntimeError):
        ops.supervise_matches(kp.cpu(), kp.cpu(), (8, 12), (8, 12))


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("k", (1, 5, 300))
@pytest.mark.parametrize("hw", ((8, 12), (12, 16)))
def test_drop_in_functions_reproduce_the_references_fixture_on_the_device(hw, k):
    pre = f"g{hw[0]}x{hw[1]}_k{k}_"
    g = {key[len(pre):]: _golden()[key] for key in _golden().files if key.startswith(pre)}
    img = torch.zeros(1, 1, hw[0] * 8, hw[1] * 8, device=DEV)
    data = {'image0': img, 'image1': img, 'origin_kp0': torch.as_tensor(g["kp0"], device=DEV)[None],
            'origin_kp1': torch.as_tensor(g["kp1"], device=DEV)[None]}
    supervision.data_preprocess(data)
    for key in ('coarse_kp0', 'coarse_kp1', 'fine_kp0', 'fine_kp1', 'lists_f0', 'lists_f1', 'fine_mtx_0', 'fine_mtx_1'):
        got = data[key]
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == g[key].shape, key
        assert np.array_equal(got.cpu().numpy().view(np.uint32), g[key].view(np.uint32)), key
    supervision.compute_supervision_coarse(data, dense_gt=True)
    for key in ("spv_i_ids", "spv_j_ids"):
        assert data[key].is_cuda and data[key].dtype == torch.int64 and np.array_equal(data[key].cpu().numpy(), g[key]), key
    assert data['spv_b_ids'].dtype == torch.int64 and not data['spv_b_ids'].any()
    assert np.array_equal(torch.nonzero(data['conf_matrix_gt'][0]).cpu().numpy(), g["gt_pos"])
    data.update({key: torch.as_tensor(g[key], device=DEV) for key in ("b_ids", "i_ids", "j_ids")})
    supervision.compute_supervision_fine(data)
    for key in ("expec_f_gt_0", "expec_f_gt_1"):
        assert np.array_equal(data[key].cpu().numpy().view(np.uint32), g[key].view(np.uint32)), key


def test_no_correspondence_on_the_device(caplog):
    img = torch.zeros(1, 1, 64, 96, device=DEV)
    data = {'image0': img, 'image1': img, 'origin_kp0': torch.zeros(1, 0, 2, device=DEV), 'origin_kp1': torch.zeros(1, 0, 2, device=DEV)}
    supervision.data_preprocess(data)
    assert data['fine_kp0'].shape == (1, 0, 2) and not data['fine_mtx_0'].any() and not data['fine_mtx_1'].any()
    with caplog.at_level(logging.WARNING, logger="featurematching_amd"):
        supervision.compute_supervision_coarse(data)
    assert len([r for r in caplog.records if "No groundtruth coarse match" in r.getMessage()]) == 1
    assert data['spv_i_ids'].tolist() == [0] and data['spv_i_ids'].is_cuda
