"""fm_supervise_matches and fm_fine_loss_forward / _backward through the C ABI without a GPU: the entry points load,
refuse bad arguments before anything launches and size their workspaces."""
import ctypes as C

from featurematching_amd import _lib

FM_E_NULL, FM_E_SHAPE, FM_E_UNSUPPORTED, FM_E_WORKSPACE = -1, -2, -3, -4
NEW = ("fm_supervise_workspace_bytes", "fm_supervise_matches", "fm_fine_loss_workspace_bytes", "fm_fine_loss_forward",
       "fm_fine_loss_backward")
FAKE = C.c_void_p(256)          # never dereferenced: every call below returns before it launches anything


def test_symbols_load():
    _lib.load()                                                      # every name of the table resolves, or this raises
    for name in NEW:
        assert name in _lib.SIGNATURES


def _supervise(lib, kp=FAKE, k=10, grid0=(8, 12), grid1=(8, 12), cell=8.0, ws=FAKE, ws_bytes=1 << 30, out=FAKE, mtx=FAKE,
               cap=10, count=FAKE):
    return lib.fm_supervise_matches(kp, kp, k, *grid0, *grid1, cell, ws, ws_bytes, out, out, out, out, out, out, out, out,
                                    mtx, mtx, cap, count, None)


def test_supervise_argument_checks():
    lib = _lib.load()
    assert _supervise(lib, kp=None) == FM_E_NULL
    assert _supervise(lib, ws=None) == FM_E_NULL
    assert _supervise(lib, out=None) == FM_E_NULL
    assert _supervise(lib, mtx=None) == FM_E_NULL
    assert _supervise(lib, count=None) == FM_E_NULL
    assert _supervise(lib, k=-1) == FM_E_SHAPE
    assert _supervise(lib, cap=-1) == FM_E_SHAPE
    assert _supervise(lib, cap=9) == FM_E_SHAPE                          # fewer rows than survivors there may be
    assert _supervise(lib, k=1000, cap=95) == FM_E_SHAPE                 # min(K, S) = 96
    for bad in (dict(grid0=(0, 12)), dict(grid0=(8, -1)), dict(grid1=(0, 12)), dict(grid1=(8, 0))):
        assert _supervise(lib, **bad) == FM_E_SHAPE, bad
    for bad in (dict(cell=0.0), dict(cell=-8.0), dict(cell=float("inf")), dict(cell=float("nan")), dict(grid0=(4097, 4096)),
                dict(grid1=(65536, 65536))):
        assert _supervise(lib, **bad) == FM_E_UNSUPPORTED, bad
    need = lib.fm_supervise_workspace_bytes(8, 12, 8, 12)
    assert _supervise(lib, ws_bytes=need - 1) == FM_E_WORKSPACE
    assert _supervise(lib, ws=C.c_void_p(264), ws_bytes=need) == FM_E_WORKSPACE
    # no correspondence is a valid call: NULL points and NULL per-survivor outputs get as far as the workspace check
    assert _supervise(lib, kp=None, k=0, out=None, cap=0, ws_bytes=16) == FM_E_WORKSPACE


def test_supervise_workspace_bytes():
    lib = _lib.load()
    for bad in ((0, 12, 8, 12), (8, 0, 8, 12), (8, 12, -1, 12), (8, 12, 8, 0), (4097, 4096, 8, 12), (8, 12, 65536, 65536)):
        assert lib.fm_supervise_workspace_bytes(*bad) == 0, bad
    sizes = [lib.fm_supervise_workspace_bytes(h, w, h, w) for h, w in ((1, 1), (2, 3), (8, 12), (60, 80), (480, 640), (4096, 4096))]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[3] >= 2 * 4800 * 4 and sizes[3] < 64 * 1024            # two int tables and the scan's block counts
    for l, s in (((8, 12), (60, 80)), ((60, 80), (8, 12)), ((15, 17), (11, 13))):
        assert lib.fm_supervise_workspace_bytes(*l, *s) % 256 == 0
        assert lib.fm_supervise_workspace_bytes(*l, *s) <= lib.fm_supervise_workspace_bytes(60, 80, 60, 80)


def _fine_calls(lib):
    def fwd(ptr=FAKE, gt=FAKE, stride=3, m=100, ws=FAKE, ws_bytes=1 << 20, out=FAKE, count=None):
        return lib.fm_fine_loss_forward(ptr, ptr, stride, gt, gt, m, count, ws, ws_bytes, out, None)

    def bwd(ptr=FAKE, gt=FAKE, stride=3, m=100, ws=FAKE, ws_bytes=1 << 20, out=FAKE, count=None):
        return lib.fm_fine_loss_backward(ptr, ptr, stride, gt, gt, m, ws, ws_bytes, out, out, out, None)
    return fwd, bwd


def test_fine_loss_argument_checks():
    lib = _lib.load()
    for call in _fine_calls(lib):
        assert call(ptr=None) == FM_E_NULL
        assert call(gt=None) == FM_E_NULL
        assert call(ws=None) == FM_E_NULL
        assert call(out=None) == FM_E_NULL
        assert call(m=-1) == FM_E_SHAPE
        assert call(stride=2) == FM_E_SHAPE
        assert call(stride=0) == FM_E_SHAPE
        need = lib.fm_fine_loss_workspace_bytes(100)
        assert call(ws_bytes=need - 1) == FM_E_WORKSPACE
        assert call(ws=C.c_void_p(264), ws_bytes=need) == FM_E_WORKSPACE
        assert call(m=0, ws_bytes=16) == FM_E_WORKSPACE                  # an empty list is a valid call up to here


def test_fine_loss_workspace_bytes():
    lib = _lib.load()
    assert lib.fm_fine_loss_workspace_bytes(-1) == 0
    sizes = [lib.fm_fine_loss_workspace_bytes(m) for m in (0, 1, 256, 257, 4097, 100000, 1 << 30)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    assert sizes[-1] == sizes[-2] < 64 * 1024                            # a bounded number of partial sums, whatever M
