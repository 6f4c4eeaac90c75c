"""The fine loss on the GPU (ops.fine_loss, modules.FineLoss; fm_fine_loss_forward / _backward) against the reference's
expression (losses/loss.py:70-98; written in torch ops in modules.fine_loss_torch and pinned to the reference's own
numbers by tests/test_supervision_ref.py), evaluated by torch on the device in float64.

Loss bar: |loss_hip - loss64| <= 4 e_ref + FLOOR |loss64| with e_ref = |loss_ref32 - loss64| of the same expression
evaluated in float32 on the same input; FLOOR = twice the largest e_ref / |loss64| over this file's inputs.
Gradient bar, per element: |g_hip - g64| <= GTOL max|g64| with GTOL = 4 x the largest per-element error of float32 autograd
of the same expression over this file's inputs, relative to max|g64|.  Both numbers are measured on the reference
expression, never on the kernel: profiles/fine_loss_accuracy.txt."""
import functools

import numpy as np
import pytest
import torch

from featurematching_amd import modules, ops, synth

import supervision_ref as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2 * 1.15e-7        # profiles/fine_loss_accuracy.txt: the largest e_ref / |loss64| over the inputs of tests/test_gpu_fine_loss.py
GTOL = 4 * 1.85e-7         # profiles/fine_loss_accuracy.txt: the largest float32 autograd error / max|g64| over the same inputs
# below / at / above a wave and a workgroup, several workgroups; 70001: k_floss_partial caps its grid at 256 workgroups,
# so above 65 536 rows its grid-stride loop takes a second trip (in the first 4465 threads only)
SIZES = (1, 2, 63, 64, 65, 257, 4097, 70001)
CASES = [f"m{m}" for m in SIZES] + ["clamp"]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """float32 numpy (expec0, expec1, gt0, gt1).  m{M}: gt uniform over a 96 x 128 image; from M = 5 on every 5th row has
    gt0 x == 0 and every 7th gt1 x == 0 (rows the loss leaves out).  clamp: M = 65 with std = 0, 1e-12 (below the clamp's
    1e-10) and 1e-10 itself in a few rows of either image."""
    m = 65 if case == "clamp" else int(case[1:])
    seed = 300 + m + (1 if case == "clamp" else 0)
    g0, g1 = sref.points(seed, m, (12, 16), 0) + np.float32(0.5), sref.points(seed, m, (12, 16), 1) + np.float32(0.5)
    g0[4::5, 0] = 0
    g1[6::7, 0] = 0
    e0, e1 = sref.fine_inputs(seed, g0, g1)
    if case == "clamp":
        e0[3, 2], e0[10, 2], e0[11, 2] = 0.0, 1e-12, 1e-10
        e1[0, 2], e1[40, 2] = 1e-12, 0.0
    return e0, e1, g0, g1


def _evaluate(arrays, dtype):
    """(loss, d_expec0, d_expec1) of the reference's expression on the device"""
    e0, e1, g0, g1 = (torch.as_tensor(a, device=DEV, dtype=dtype) for a in arrays)
    e0.requires_grad_(True)
    e1.requires_grad_(True)
    loss = modules.fine_loss_torch(e0, e1, g0, g1)
    if loss.requires_grad:
        loss.backward()
    zero = torch.zeros_like(e0)
    return loss.item(), (zero if e0.grad is None else e0.grad), (zero if e1.grad is None else e1.grad)


@functools.lru_cache(maxsize=None)
def _reference(case):
    return _evaluate(_inputs(case), torch.float64), _evaluate(_inputs(case), torch.float32)


def _hip(arrays, scale=1.0, count=None):
    e0, e1, g0, g1 = (torch.as_tensor(a, device=DEV) for a in arrays)
    e0.requires_grad_(True)
    e1.requires_grad_(True)
    loss = ops.fine_loss(e0, e1, g0, g1, count=count)
    (scale * loss).backward()
    return loss, e0.grad, e1.grad


def _assert_close(case, got, ref64, ref32, scale=1.0):
    (l64, r0, r1), (l32, s0, s1) = ref64, ref32
    loss, d0, d1 = got
    e_ref = abs(l32 - l64)
    print(f"ACC  {case:8s} loss64 {l64:.9e}  e_ref/|loss64| {e_ref / abs(l64):.3e}  e_hip/|loss64| "
          f"{abs(loss.item() - l64) / abs(l64):.3e}")
    for name, g, r, s in (("d_expec0", d0, r0, s0), ("d_expec1", d1, r1, s1)):
        top = r.abs().max().item()
        print(f"GRAD {case:8s} {name} max|g64| {top:.3e}  e_ref32/max {(s.double() - r).abs().max().item() / top:.3e}  "
              f"e_hip/max {(g.double() / scale - r).abs().max().item() / top:.3e}")
    assert abs(loss.item() - l64) <= 4 * e_ref + FLOOR * abs(l64), (case, loss.item(), l64, e_ref)
    for g, r in ((d0, r0), (d1, r1)):
        top = r.abs().max().item()
        assert top > 0 and (g.double() / scale - r).abs().max().item() <= GTOL * top, case
        assert g.dtype == torch.float32 and g[:, 2].abs().max().item() == 0          # the weights are detached
        # rows left out: exactly zero.  They are the rows whose reference gradient is zero in x AND y; x alone does not
        # tell (m70001, row 4802 of image 0: expec x == gt x in float32, the row takes part and has a y gradient)
        assert (g[(r[:, :2] == 0).all(1)][:, :2] == 0).all()


@pytest.mark.parametrize("case", CASES)
def test_loss_and_gradients_against_float64_autograd_of_the_references_expression(case):
    e0, e1, g0, g1 = _inputs(case)
    if case not in ("m1", "m2"):
        assert (g0[:, 0] == 0).any() and (g0[:, 0] != 0).any() and (g1[:, 0] == 0).any()
    _assert_close(case, _hip(_inputs(case)), *_reference(case))


def test_upstream_gradient_scales_the_gradients():
    _assert_close("m257 x2.5", _hip(_inputs("m257"), scale=2.5), *_reference("m257"), scale=2.5)


def test_two_runs_give_the_same_bits():
    for case in ("m65", "m4097"):
        a, b = _hip(_inputs(case)), _hip(_inputs(case))
        assert all(torch.equal(x, y) for x, y in zip(a, b)), case
        assert torch.equal(a[0].terms, b[0].terms)


@pytest.mark.parametrize("images", [(0,), (1,), (0, 1)])
def test_every_row_left_out_is_nan_as_in_the_reference(images):
    arrays = [a.copy() for a in _inputs("m65")]
    for d in images:
        arrays[2 + d][:, 0] = 0
    l64, r0, r1 = _evaluate(arrays, torch.float64)
    loss, d0, d1 = _hip(arrays)
    assert np.isnan(l64) and torch.isnan(loss).item() and torch.isnan(loss.terms[list(images)]).all()
    for d, (r, g) in enumerate(((r0, d0), (r1, d1))):
        if d in images:                                     # no row of this image takes part: no gradient there
            assert not r.any() and not g.any()
        else:                                               # the other image's term and gradient are as ever
            assert torch.isfinite(loss.terms[d]) and (g.double() - r).abs().max().item() <= GTOL * r.abs().max().item()


def test_expec0_all_zero_gives_zero_loss_and_exactly_zero_gradients():
    e0, e1, g0, g1 = _inputs("m257")
    zero = np.zeros_like(e0)
    assert _evaluate((zero, e1, g0, g1), torch.float64)[0] == 0
    loss, d0, d1 = _hip((zero, e1, g0, g1), scale=3.0)
    assert loss.item() == 0 and not d0.any() and not d1.any() and d0.shape == e0.shape
    # entries that cancel are not "all zero" to the reference only when their sum is exactly 0: +a and -a are
    cancel = zero.copy()
    cancel[0, 0], cancel[1, 1] = 2.5, -2.5
    assert _evaluate((cancel, e1, g0, g1), torch.float64)[0] == 0
    assert _hip((cancel, e1, g0, g1))[0].item() == 0


def test_device_count_below_the_capacity():
    """m_max = 257 rows of storage, 100 counted: the loss of the first 100 rows; what lies beyond is never read (NaN
    there) and gets zero gradients"""
    arrays = [a.copy() for a in _inputs("m257")]
    head = [a[:100] for a in arrays]
    for a in arrays:
        a[100:] = np.nan
    count = torch.tensor([100], dtype=torch.int32, device=DEV)
    got = _hip(arrays, count=count)
    assert not got[1][100:].any() and not got[2][100:].any()
    _assert_close("m257/100", (got[0], got[1][:100], got[2][:100]), _evaluate(head, torch.float64), _evaluate(head, torch.float32))
    full = _hip(head)
    assert torch.equal(full[1], got[1][:100]) and abs(full[0].item() - got[0].item()) <= FLOOR * abs(full[0].item())


def test_empty_list_is_zero_and_keeps_the_graph():
    e0 = torch.zeros(0, 3, device=DEV, requires_grad=True)
    e1 = torch.zeros(0, 3, device=DEV, requires_grad=True)
    g = torch.zeros(0, 2, device=DEV)
    loss = ops.fine_loss(e0, e1, g, g)
    assert loss.item() == 0 and loss.dim() == 0 and loss.device.type == "cuda" and loss.dtype == torch.float32
    loss.backward()                                         # the fine term alone is a valid objective
    assert e0.grad.shape == (0, 3) and e1.grad.shape == (0, 3)


def test_module_and_argument_checks():
    e0, e1, g0, g1 = (torch.as_tensor(a, device=DEV) for a in _inputs("m63"))
    data = {'mkpts0_f': e0, 'mkpts1_f': e1, 'expec_f_gt_0': g0, 'expec_f_gt_1': g1}
    assert torch.equal(modules.FineLoss()(data), ops.fine_loss(e0, e1, g0, g1))
    with pytest.raises(ValueError):
        ops.fine_loss(e0[:, :2], e1, g0, g1)
    with pytest.raises(ValueError):
        ops.fine_loss(e0, e1, g0[:5], g1)
    with pytest.raises(RuntimeError):
        ops.fine_loss(e0.cpu(), e1.cpu(), g0.cpu(), g1.cpu())
    # strided views of a wider tensor are read as they should be (the wrapper makes them contiguous)
    wide = torch.zeros(63, 5, device=DEV)
    wide[:, :3] = e0
    assert torch.equal(ops.fine_loss(wide[:, :3], e1, g0, g1), ops.fine_loss(e0, e1, g0, g1))
