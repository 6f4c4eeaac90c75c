"""fm_window_merge_forward / _backward through the C ABI without a GPU: the entry points load, refuse bad arguments before
anything launches - in the header's order - and size their workspace."""
import ctypes as C

from featurematching_amd import _lib

FM_OK, FM_E_NULL, FM_E_SHAPE, FM_E_UNSUPPORTED, FM_E_WORKSPACE = 0, -1, -2, -3, -4
NEW = ("fm_window_merge_workspace_bytes", "fm_window_merge_forward", "fm_window_merge_backward")
FAKE = C.c_void_p(1024)         # never dereferenced: every call below returns before it launches anything
INPUTS = ("feat_f", "w_win", "ctx", "b_ids", "ids")
GEOM = dict(N=2, Cf=64, Hf=24, Wf=32, layout=0, W=7, stride=4, pad=2, h_c=6, w_c=8)
FRAG = 2 * 4096 * 4             # bytes of the weight in the kernels' operand order, forward and backward
SLAB = 4096 * 4                 # bytes of one workgroup's partial weight gradient


def test_symbols_load():
    _lib.load()                                                      # every name of the table resolves, or this raises
    for name in NEW:
        assert name in _lib.SIGNATURES


def _calls(lib):
    def geom(kw):
        g = dict(GEOM)
        g.update({k: kw.pop(k) for k in list(kw) if k in GEOM})
        return [g[k] for k in GEOM]

    def fwd(m_max=300, ws=FAKE, ws_bytes=1 << 40, **kw):
        g = geom(kw)
        p = {k: FAKE for k in INPUTS + ("out",)}
        p.update(kw)
        return lib.fm_window_merge_forward(p["feat_f"], *g, p["w_win"], p["ctx"], p["b_ids"], p["ids"], m_max, ws, ws_bytes,
                                           p["out"], None)

    def bwd(m_max=300, ws=FAKE, ws_bytes=1 << 40, **kw):
        g = geom(kw)
        p = {k: FAKE for k in INPUTS + ("g", "d_feat", "d_w_win", "d_ctx")}
        p.update(kw)
        return lib.fm_window_merge_backward(p["feat_f"], *g, p["w_win"], p["ctx"], p["b_ids"], p["ids"], m_max, p["g"], ws,
                                            ws_bytes, p["d_feat"], p["d_w_win"], p["d_ctx"], None)
    return fwd, bwd


def test_argument_checks():
    lib = _lib.load()
    fwd, bwd = _calls(lib)
    need = lib.fm_window_merge_workspace_bytes(2, 6, 8, 300, 7)
    assert need > 0
    for call, own in ((fwd, ("out",)), (bwd, ("g", "d_ctx"))):
        for missing in INPUTS + own:
            assert call(**{missing: None}) == FM_E_NULL, missing
        for size in ("N", "Cf", "Hf", "Wf", "W", "stride", "h_c", "w_c"):
            for bad in (0, -1):
                assert call(**{size: bad}) == FM_E_SHAPE, (size, bad)
        assert call(m_max=-1) == FM_E_SHAPE
        for cf in (32, 63, 65, 128):
            assert call(Cf=cf) == FM_E_UNSUPPORTED, cf
        for w in (1, 3, 6, 9):
            assert call(W=w) == FM_E_UNSUPPORTED, w
        assert call(pad=-1) == FM_E_UNSUPPORTED
        for layout in (-1, 2):
            assert call(layout=layout) == FM_E_UNSUPPORTED
        assert call(m_max=(1 << 24) // 49 + 1) == FM_E_UNSUPPORTED           # more than 2^24 tokens
        assert call(m_max=(1 << 24) // 49, ws_bytes=0) == FM_E_WORKSPACE     # ... 2^24 and fewer are served
        assert call(W=5, m_max=(1 << 24) // 25 + 1) == FM_E_UNSUPPORTED
        assert call(W=5, m_max=(1 << 24) // 25, ws_bytes=0) == FM_E_WORKSPACE
        for stride, pad in ((1, 0), (2, 3), (8, 2)):
            assert call(stride=stride, pad=pad, ws_bytes=0) == FM_E_WORKSPACE
        assert call(layout=1, ws_bytes=0) == FM_E_WORKSPACE
        assert call(ws_bytes=need - 1) == FM_E_WORKSPACE             # one byte short
        assert call(ws=C.c_void_p(1024 + 8), ws_bytes=need) == FM_E_WORKSPACE
        assert call(ws=None, ws_bytes=need) == FM_E_WORKSPACE
        # a missing pointer is reported before a bad shape, a bad shape before an unsupported one, that before the workspace
        assert call(feat_f=None, Hf=0, Cf=32, ws_bytes=0) == FM_E_NULL
        assert call(Hf=0, Cf=32, ws_bytes=0) == FM_E_SHAPE
        assert call(m_max=-1, W=9, ws_bytes=0) == FM_E_SHAPE
        assert call(Cf=32, ws_bytes=0) == FM_E_UNSUPPORTED
        assert call(W=9, ws_bytes=0) == FM_E_UNSUPPORTED
        assert call(ws_bytes=0) == FM_E_WORKSPACE


def test_null_weight_and_map_gradients_are_accepted():
    lib = _lib.load()
    _, bwd = _calls(lib)
    assert bwd(d_w_win=None, ws_bytes=0) == FM_E_WORKSPACE               # passes every check before the workspace
    assert bwd(d_feat=None, ws_bytes=0) == FM_E_WORKSPACE                # a frozen backbone: no map gradient
    assert bwd(d_feat=None, d_w_win=None, ws_bytes=0) == FM_E_WORKSPACE
    assert bwd(ws_bytes=0) == FM_E_WORKSPACE
    assert bwd(d_w_win=None, d_ctx=None) == FM_E_NULL                    # the other gradients stay required


def test_empty_list_returns_at_once():
    """m_max = 0: FM_OK before any argument is looked at, nothing launched (there is no GPU here)"""
    lib = _lib.load()
    fwd, bwd = _calls(lib)
    for call in (fwd, bwd):
        assert call(m_max=0) == FM_OK
        assert call(m_max=0, ws=None, ws_bytes=0) == FM_OK
        assert call(m_max=0, feat_f=None, Cf=65, W=9) == FM_OK


def test_workspace_query():
    ws = _lib.load().fm_window_merge_workspace_bytes
    counts = (0, 1, 2, 3, 5, 6, 21, 300, 1400, 4000, 100000, (1 << 24) // 49)
    for w in (5, 7):
        sizes = [ws(2, 6, 8, m, w) for m in counts]
        assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
        assert sizes == sorted(sizes)                                # it does not decrease with m_max
    assert ws(2, 6, 8, 300, 7) >= ws(2, 6, 8, 300, 5)
    assert ws(4, 60, 80, 300, 7) >= ws(1, 60, 80, 300, 7)            # nor with the batch (the crop backward's lists)
    for args in ((0, 6, 8, 300, 7), (-1, 6, 8, 300, 7), (2, 0, 8, 300, 7), (2, 6, 0, 300, 7), (2, 6, 8, -1, 7),
                 (2, 6, 8, 300, 0), (2, 6, 8, 300, 3), (2, 6, 8, 300, 9), (2, 6, 8, (1 << 24) // 49 + 1, 7),
                 (2, 6, 8, (1 << 24) // 25 + 1, 5), (1 << 16, 1 << 8, 1 << 8, 300, 7)):
        assert ws(*args) == 0, args
    # the fragments, one slab per workgroup of the backward (one per 128 tokens, at most 256), g w_win [m_max, W W, 64] and
    # the crop backward's own workspace, each on a 256-byte boundary
    crop = _lib.load().fm_gather_windows_backward_workspace_bytes
    up = lambda x: (x + 255) // 256 * 256
    for m, w in ((1, 7), (3, 7), (300, 7), (300, 5), (1400, 7)):
        tokens = m * w * w
        groups = min(256, (tokens + 127) // 128)
        assert ws(2, 6, 8, m, w) == FRAG + groups * SLAB + up(tokens * 64 * 4) + up(crop(2, 6, 8, m)), (m, w)
