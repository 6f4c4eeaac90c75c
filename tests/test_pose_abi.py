"""fm_estimate_pose / fm_pose_workspace_bytes / fm_debug_pose_solve through the C ABI without a GPU: the entry points load,
refuse bad arguments before anything launches - in the header's order - and size their workspace."""
import ctypes as C

from featurematching_amd import _lib

FM_OK, FM_E_NULL, FM_E_SHAPE, FM_E_UNSUPPORTED, FM_E_WORKSPACE = 0, -1, -2, -3, -4
FAKE = C.c_void_p(1024)         # never dereferenced: every call below returns before it launches anything
POINTERS = ("mkpts0", "mkpts1", "m_bids", "K0", "K1", "R_out", "t_out", "E_out", "inlier", "per_pair")
INF, NAN = float("inf"), float("nan")


def test_symbols_load():
    _lib.load()                                                      # every name of the table resolves, or this raises
    for name in ("fm_pose_workspace_bytes", "fm_estimate_pose"):
        assert name in _lib.SIGNATURES
    assert "fm_debug_pose_solve" in _lib.DEBUG_SIGNATURES
    assert len(_lib.SIGNATURES["fm_estimate_pose"][1]) == 20
    assert _lib.SIGNATURES["fm_pose_workspace_bytes"][0] == C.c_size_t


def call(lib, kpt_stride=2, d_count=None, m_max=300, N=2, pixel_thr=1.0, samples=64, seed=0, ws=FAKE, ws_bytes=1 << 40, **kw):
    p = {k: FAKE for k in POINTERS}
    p.update(kw)
    return lib.fm_estimate_pose(p["mkpts0"], p["mkpts1"], kpt_stride, p["m_bids"], d_count, m_max, N, p["K0"], p["K1"], pixel_thr,
                                samples, seed, ws, ws_bytes, p["R_out"], p["t_out"], p["E_out"], p["inlier"], p["per_pair"], None)


def test_argument_checks():
    lib = _lib.load()
    need = lib.fm_pose_workspace_bytes(2, 300, 64)
    assert need > 0
    for missing in POINTERS:
        assert call(lib, **{missing: None}) == FM_E_NULL, missing
    assert call(lib, d_count=None, ws_bytes=0) == FM_E_WORKSPACE         # d_count may be NULL
    for kw in (dict(N=0), dict(N=-1), dict(m_max=-1), dict(kpt_stride=1), dict(kpt_stride=0), dict(samples=0), dict(samples=-3)):
        assert call(lib, **kw) == FM_E_SHAPE, kw
    for thr in (0.0, -1.0, INF, NAN):
        assert call(lib, pixel_thr=thr) == FM_E_UNSUPPORTED, thr
    assert call(lib, samples=65537) == FM_E_UNSUPPORTED
    assert call(lib, samples=65536, ws_bytes=0) == FM_E_WORKSPACE        # ... 65536 and fewer are served
    assert call(lib, m_max=(1 << 31) // 8) == FM_E_UNSUPPORTED
    assert call(lib, m_max=(1 << 31) // 8 - 1, ws_bytes=0) == FM_E_WORKSPACE
    for stride in (2, 3, 5):
        assert call(lib, kpt_stride=stride, ws_bytes=0) == FM_E_WORKSPACE
    assert call(lib, ws_bytes=need - 1) == FM_E_WORKSPACE                # one byte short
    assert call(lib, ws=C.c_void_p(1024 + 8), ws_bytes=need) == FM_E_WORKSPACE
    assert call(lib, ws=None, ws_bytes=need) == FM_E_WORKSPACE
    # a missing pointer is reported before a bad shape, a bad shape before an unsupported one, that before the workspace
    assert call(lib, K1=None, N=0, samples=65537, ws_bytes=0) == FM_E_NULL
    assert call(lib, N=0, samples=65537, ws_bytes=0) == FM_E_SHAPE
    assert call(lib, kpt_stride=1, pixel_thr=0.0, ws_bytes=0) == FM_E_SHAPE
    assert call(lib, pixel_thr=NAN, ws_bytes=0) == FM_E_UNSUPPORTED
    assert call(lib, samples=65537, ws_bytes=0) == FM_E_UNSUPPORTED
    assert call(lib, ws_bytes=0) == FM_E_WORKSPACE


def test_empty_list_returns_after_the_checks():
    """m_max = 0: FM_OK once the checks have passed, nothing launched (there is no GPU here)"""
    lib = _lib.load()
    need = lib.fm_pose_workspace_bytes(2, 0, 64)
    assert need > 0
    assert call(lib, m_max=0, ws_bytes=need) == FM_OK
    assert call(lib, m_max=0, mkpts0=None) == FM_E_NULL
    assert call(lib, m_max=0, N=0) == FM_E_SHAPE
    assert call(lib, m_max=0, pixel_thr=-1.0) == FM_E_UNSUPPORTED
    assert call(lib, m_max=0, ws_bytes=need - 1) == FM_E_WORKSPACE


def test_workspace_query():
    ws = _lib.load().fm_pose_workspace_bytes
    counts = (0, 1, 4, 5, 63, 64, 65, 300, 4000, 100000, (1 << 31) // 8 - 1)
    sizes = [ws(2, m, 64) for m in counts]
    assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
    assert sizes == sorted(sizes)
    sizes = [ws(2, 300, s) for s in (1, 2, 63, 64, 65, 256, 2048, 65536)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    sizes = [ws(n, 300, 64) for n in (1, 2, 3, 4, 64, 1000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for args in ((0, 300, 64), (-1, 300, 64), (2, -1, 64), (2, 300, 0), (2, 300, -1), (2, 300, 65537), (2, (1 << 31) // 8, 64)):
        assert ws(*args) == 0, args
    # segments int32 [N + 1] | winners uint64 [N] | thresholds float64 [N] | normalised matches float64 [m_max, 4] |
    # candidate counts int32 [N samples] | candidates float64 [N samples, 10, 9], each on a 256-byte boundary
    up = lambda x: (x + 255) // 256 * 256
    for n, m, s in ((1, 0, 1), (2, 300, 64), (4, 4000, 2048), (3, 65, 65)):
        assert ws(n, m, s) == up(4 * (n + 1)) + up(8 * n) + up(8 * n) + up(32 * m) + up(4 * n * s) + up(720 * n * s), (n, m, s)


def test_debug_solver_checks():
    lib = _lib.load()
    f = lib.fm_debug_pose_solve
    assert f(None, FAKE, 4, FAKE, FAKE, None) == FM_E_NULL
    assert f(FAKE, None, 4, FAKE, FAKE, None) == FM_E_NULL
    assert f(FAKE, FAKE, 4, None, FAKE, None) == FM_E_NULL
    assert f(FAKE, FAKE, 4, FAKE, None, None) == FM_E_NULL
    assert f(FAKE, FAKE, 0, FAKE, FAKE, None) == FM_E_SHAPE
    assert f(FAKE, FAKE, -2, FAKE, FAKE, None) == FM_E_SHAPE
    assert f(None, FAKE, 0, FAKE, FAKE, None) == FM_E_NULL
