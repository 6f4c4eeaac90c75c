"""The yardsticks of the window crop tests (tests/fine_grad_ref.py: crop_ref, crop_adjoint) against torch's own unfold
with the same kernel_size / stride / padding, on the CPU: the forward equal, the adjoint equal to float64 autograd
through unfold.  The coarse grid is unfold's own output grid, so nothing here assumes h_c * stride == Hf."""
import pytest
import torch
import torch.nn.functional as F

from fine_grad_ref import CROP_CASES, CROP_MAP, crop_adjoint, crop_ref, crop_unfold, unfold_grid

N, HF, WF = CROP_MAP


def _unfold_windows(feat, w, stride, pad):
    """[N, L, W*W, Cf]: every window of unfold's grid, position wy * W + wx"""
    n, cf = feat.shape[:2]
    u = F.unfold(feat, kernel_size=w, stride=stride, padding=pad)           # [N, Cf*WW, L], rows c * WW + r
    return u.view(n, cf, w * w, -1).permute(0, 3, 2, 1)


def _ids(h_c, w_c, seed):
    g = torch.Generator().manual_seed(seed)
    cells = h_c * w_c
    i = torch.cat([torch.randint(cells, (200,), generator=g), torch.tensor([0, w_c - 1, cells - w_c, cells - 1]),
                   torch.full((30,), cells // 2)])
    b = torch.randint(N, (i.shape[0],), generator=g)
    p = torch.randperm(i.shape[0], generator=g)
    return b[p], i[p]


@pytest.mark.parametrize("cf,w,stride,pad", CROP_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_crop_ref_equals_unfold(cf, w, stride, pad, dtype):
    h_c, w_c = unfold_grid(HF, WF, w, stride, pad)
    feat = torch.randn(N, cf, HF, WF, generator=torch.Generator().manual_seed(cf + w)).to(dtype)
    b, i = _ids(h_c, w_c, 3)
    want = _unfold_windows(feat.float(), w, stride, pad)[b, i]
    got = crop_ref(feat, b, i, w, stride, pad, w_c)
    assert got.dtype == dtype and got.shape == (b.shape[0], w * w, cf)
    assert torch.equal(got.float(), want)
    # the differentiable route of the GPU tests is the same crop
    assert torch.equal(crop_unfold(feat.float(), b, i, w, stride, pad, h_c, w_c), want)


@pytest.mark.parametrize("cf,w,stride,pad", CROP_CASES)
def test_crop_adjoint_equals_autograd_through_unfold(cf, w, stride, pad):
    h_c, w_c = unfold_grid(HF, WF, w, stride, pad)
    b, i = _ids(h_c, w_c, 4)
    # multiples of 2^-20: every float64 sum of them is exact, so the order of the additions (index_add_ here, index_put
    # and col2im in autograd) cannot matter and the error must be exactly 0
    d_win = torch.randn(b.shape[0], w * w, cf, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    d_win = torch.round(d_win * 2 ** 20) / 2 ** 20
    feat = torch.zeros(N, cf, HF, WF, dtype=torch.float64, requires_grad=True)
    _unfold_windows(feat, w, stride, pad)[b, i].backward(d_win)
    got, reads = crop_adjoint(d_win, b, i, (N, cf, HF, WF), w, stride, w_c, pad)
    scale = feat.grad.abs().max().item()
    err = (got - feat.grad).abs().max().item()
    print(f"Cf={cf} W={w} stride={stride} pad={pad}: |crop_adjoint - autograd| {err:.3e}, max|g| {scale:.3e}")
    assert scale > 0 and err == 0.0
    ones = torch.zeros(N, 1, HF, WF, dtype=torch.float64, requires_grad=True)
    _unfold_windows(ones, w, stride, pad)[b, i].sum().backward()
    assert torch.equal(reads.double(), ones.grad)


def test_crop_yardsticks_when_the_grid_overhangs_the_map():
    """ids of a coarse grid larger than map / stride: windows partly or wholly in the padding are zero there and
    their gradient goes nowhere"""
    feat = torch.randn(N, 8, HF, WF, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    w, stride, pad, h_c, w_c = 7, 4, 2, 12, 14                  # 12 * 4 = 48 > 37, 14 * 4 = 56 > 45
    b = torch.tensor([0, 1, 1, 0, 1])
    i = torch.tensor([h_c * w_c - 1, 13, 11 * w_c, 5 * w_c + 11, 3 * w_c + 4])
    got = crop_ref(feat, b, i, w, stride, pad, w_c)
    assert (got[:3] == 0).all()                                 # wholly outside
    # cell (5, 11): origin (18, 42); columns 42..44 are inside, 45..48 outside
    ref = torch.zeros(7, 7, 8, dtype=torch.float64)
    ref[:, :3] = feat[0, :, 18:25, 42:45].permute(1, 2, 0)
    assert torch.equal(got[3], ref.view(49, 8))
    leaf = feat.clone().requires_grad_(True)
    via_unfold = crop_unfold(leaf, b, i, w, stride, pad, h_c, w_c)
    assert torch.equal(via_unfold.detach(), got)
    d_win = torch.randn(5, 49, 8, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    via_unfold.backward(d_win)
    adj, reads = crop_adjoint(d_win, b, i, (N, 8, HF, WF), w, stride, w_c, pad)
    assert torch.equal(adj, leaf.grad)
    assert reads.sum().item() == 49 + 7 * 3
