"""The fine stage's backward through the C ABI without a GPU: the four entry points load, validate their arguments on
the host and size their workspaces; and the backward formula the kernels implement (include/fmatch.h,
fm_fine_match_backward) is pinned against autograd, on the CPU, in float64."""
import ctypes as C

import torch

from featurematching_amd import _lib
from oracle import matcher_ref as orc

from fine_grad_ref import fine_backward, fine_forward

FM_E_NULL, FM_E_SHAPE, FM_E_UNSUPPORTED = -1, -2, -3
NEW = ("fm_fine_match_backward", "fm_fine_match_backward_workspace_bytes", "fm_gather_windows_backward",
       "fm_gather_windows_backward_workspace_bytes")
FAKE = C.c_void_p(256)          # never dereferenced: every call below returns before it launches anything


def test_symbols_load():
    _lib.load()                                                      # every name of the table resolves, or this raises
    for name in NEW:
        assert name in _lib.SIGNATURES


def _fine(lib, m_max, ww=49, cf=64, ptr=FAKE):
    return lib.fm_fine_match_backward(ptr, ptr, m_max, None, ww, cf, ptr, ptr, 1.0, ptr, ptr, ptr, 1 << 30, ptr, ptr, ptr,
                                      ptr, None)


def _crop(lib, m_max, ptr=FAKE, cf=64, w=7, layout=0):
    return lib.fm_gather_windows_backward(ptr, ptr, ptr, None, m_max, 1, cf, 120, 160, layout, w, 4, 2, 30, 40, ptr, 1 << 30,
                                          ptr, None)


def test_argument_checks():
    lib = _lib.load()
    assert _fine(lib, 0, ptr=None) == _lib.FM_OK
    assert _crop(lib, 0, ptr=None) == _lib.FM_OK
    assert _fine(lib, 8, ptr=None) == FM_E_NULL
    assert _crop(lib, 8, ptr=None) == FM_E_NULL
    assert _fine(lib, -1) == FM_E_SHAPE
    assert _crop(lib, -1) == FM_E_SHAPE
    for ww in (9, 36, 64):
        assert _fine(lib, 8, ww=ww) == FM_E_UNSUPPORTED
    assert _fine(lib, 8, cf=128) == FM_E_UNSUPPORTED
    assert _crop(lib, 8, cf=1024) == FM_E_UNSUPPORTED
    assert _crop(lib, 8, w=17) == FM_E_UNSUPPORTED
    assert _crop(lib, 8, layout=2) == FM_E_UNSUPPORTED


def test_crop_backward_shape_limits():
    """the crop backward takes any Cf <= 512 and W <= 15 in both layouts (no Cf % 4 rule, no LDS limit: those belong to
    the forward); what it refuses is refused before anything launches"""
    lib = _lib.load()
    for layout in (0, 1):
        assert _crop(lib, 8, cf=513, layout=layout) == FM_E_UNSUPPORTED
        assert _crop(lib, 8, w=16, layout=layout) == FM_E_UNSUPPORTED
        assert _crop(lib, 8, cf=0, layout=layout) == FM_E_SHAPE
        assert _crop(lib, 8, w=0, layout=layout) == FM_E_SHAPE
    assert _crop(lib, 8, layout=-1) == FM_E_UNSUPPORTED
    # the workspace is checked after the shape: too small, misaligned
    args = lambda ws, nbytes: (FAKE, FAKE, FAKE, None, 8, 1, 6, 120, 160, 1, 15, 4, 7, 30, 40, ws, nbytes, FAKE, None)
    need = lib.fm_gather_windows_backward_workspace_bytes(1, 30, 40, 8)
    assert need > 0
    assert lib.fm_gather_windows_backward(*args(FAKE, need - 1)) == -4
    assert lib.fm_gather_windows_backward(*args(C.c_void_p(264), need)) == -4


def test_workspace_bytes_monotone_in_m():
    lib = _lib.load()
    for ww in (25, 49):
        sizes = [lib.fm_fine_match_backward_workspace_bytes(m, ww) for m in (1, 10, 100, 1000, 4800, 20000)]
        assert all(a < b for a, b in zip(sizes, sizes[1:]))
        assert sizes[-1] >= 20000 * 2 * (ww + 1) * 4
    sizes = [lib.fm_gather_windows_backward_workspace_bytes(2, 60, 80, m) for m in (1, 10, 100, 1000, 4800, 20000)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes[-1] >= (2 * 4800 * 2 + 1 + 20000) * 4
    assert lib.fm_fine_match_backward_workspace_bytes(-1, 49) == 0
    assert lib.fm_gather_windows_backward_workspace_bytes(1, 30, 40, -1) == 0


def test_backward_formula_matches_autograd_float64():
    """the formula of fm_fine_match_backward (tests/fine_grad_ref.py) against float64 autograd of the restated forward,
    which itself agrees with the oracle (oracle.matcher_ref.fine_match, float32)"""
    g = torch.Generator().manual_seed(5)
    for w, spread in ((7, 1.0), (5, 1.0), (7, 0.05)):       # spread 0.05: flat heat maps, every variance well above 1e-10
        m, ww = 37, w * w
        win0 = (torch.randn(m, ww, 64, generator=g, dtype=torch.float64) * spread).requires_grad_(True)
        win1 = (torch.randn(m, ww, 64, generator=g, dtype=torch.float64) * spread).requires_grad_(True)
        mix0 = (torch.rand(ww + 1, generator=g, dtype=torch.float64) * 2 - 1).div(w).requires_grad_(True)
        mix1 = (torch.rand(ww + 1, generator=g, dtype=torch.float64) * 2 - 1).div(w).requires_grad_(True)
        k0 = torch.rand(m, 2, generator=g, dtype=torch.float64) * 100
        k1 = torch.rand(m, 2, generator=g, dtype=torch.float64) * 100
        scale = 2.0
        out0, out1 = fine_forward(win0, win1, mix0, mix1, k0, k1, scale)
        r0, r1 = orc.fine_match(win0.detach().float(), win1.detach().float(), mix0[:ww].detach().float(),
                                mix0[ww].detach().float(), mix1[:ww].detach().float(), mix1[ww].detach().float(),
                                k0.float(), k1.float(), scale)
        assert (out0.detach() - r0.double()).abs().max() < 1e-3 and (out1.detach() - r1.double()).abs().max() < 1e-3
        d0 = torch.randn(m, 3, generator=g, dtype=torch.float64)
        d1 = torch.randn(m, 3, generator=g, dtype=torch.float64)
        auto = torch.autograd.grad((out0 * d0).sum() + (out1 * d1).sum(), (win0, win1, mix0, mix1))
        mine = fine_backward(win0.detach(), win1.detach(), mix0.detach(), mix1.detach(), scale, d0, d1)
        for name, a, b in zip(("d_win0", "d_win1", "d_mix0", "d_mix1"), auto, mine):
            err = (a - b).abs().max().item()
            assert err <= 1e-9 * a.abs().max().item(), f"W={w} spread={spread} {name}: {err}"
