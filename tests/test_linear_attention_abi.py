"""fm_linear_attention_forward / _backward through the C ABI without a GPU: the entry points load, refuse bad arguments
before anything launches and size their state and workspace."""
import ctypes as C

from featurematching_amd import _lib

FM_E_NULL, FM_E_SHAPE, FM_E_UNSUPPORTED, FM_E_WORKSPACE = -1, -2, -3, -4
NEW = ("fm_linear_attention_state_bytes", "fm_linear_attention_workspace_bytes", "fm_linear_attention_forward",
       "fm_linear_attention_backward")
FAKE = C.c_void_p(256)          # never dereferenced: every call below returns before it launches anything
WINDOW, LONG = (3, 25, 49, 8, 8), (2, 300, 200, 8, 32)
SLAB = 8 * 33 * 32 * 4          # bytes of A | Ksum of one sample


def test_symbols_load():
    _lib.load()                                                      # every name of the table resolves, or this raises
    for name in NEW:
        assert name in _lib.SIGNATURES


def _calls(lib):
    def fwd(q=FAKE, k=FAKE, v=FAKE, masks=(None, None), dims=LONG, eps=1e-6, ws=FAKE, ws_bytes=1 << 40, state=FAKE, out=FAKE,
            g=FAKE):
        return lib.fm_linear_attention_forward(q, k, v, *masks, *dims, eps, ws, ws_bytes, state, out, None)

    def bwd(q=FAKE, k=FAKE, v=FAKE, masks=(None, None), dims=LONG, eps=1e-6, ws=FAKE, ws_bytes=1 << 40, state=FAKE, out=FAKE,
            g=FAKE):
        return lib.fm_linear_attention_backward(q, k, v, *masks, g, state, *dims, eps, ws, ws_bytes, out, out, out, None)
    return fwd, bwd


def test_argument_checks():
    lib = _lib.load()
    fwd, bwd = _calls(lib)
    for call in (fwd, bwd):
        for missing in ("q", "k", "v", "out", "ws", "state"):
            assert call(**{missing: None}) == FM_E_NULL, missing
        for i in range(5):                                           # N, L, S, H, D: zero and negative
            for bad in (0, -1):
                dims = list(LONG)
                dims[i] = bad
                assert call(dims=dims) == FM_E_SHAPE, dims
        for dims in ((2, 300, 200, 8, 16), (2, 300, 200, 4, 32), (2, 300, 200, 4, 8), (3, 65, 49, 8, 8), (3, 49, 65, 8, 8),
                     (2, 300, 200, 16, 16), (65536, 3, 3, 8, 32)):
            assert call(dims=dims) == FM_E_UNSUPPORTED, dims
        for eps in (0.0, -1e-6, float("nan")):
            assert call(eps=eps) == FM_E_UNSUPPORTED, eps
            assert call(eps=eps, dims=WINDOW) == FM_E_UNSUPPORTED, eps
        need = lib.fm_linear_attention_workspace_bytes(*LONG)
        assert call(ws_bytes=need - 1) == FM_E_WORKSPACE             # one byte short
        assert call(ws=C.c_void_p(264), ws_bytes=need) == FM_E_WORKSPACE
        # a missing pointer is reported before a bad shape, a bad shape before an unsupported one, that before the workspace
        assert call(q=None, dims=(0, 300, 200, 8, 16), ws_bytes=0) == FM_E_NULL
        assert call(dims=(0, 300, 200, 8, 16), ws_bytes=0) == FM_E_SHAPE
        assert call(dims=(2, 300, 200, 8, 16), ws_bytes=0) == FM_E_UNSUPPORTED
    assert bwd(g=None) == FM_E_NULL
    assert bwd(g=None, dims=WINDOW) == FM_E_NULL
    # the window route has no state and no workspace, but its other pointers and its shape are checked all the same
    assert fwd(q=None, dims=WINDOW, ws=None, state=None) == FM_E_NULL
    assert fwd(out=None, dims=WINDOW, ws=None, state=None) == FM_E_NULL
    assert bwd(out=None, dims=WINDOW, ws=None, state=None) == FM_E_NULL
    assert fwd(dims=(3, 0, 49, 8, 8), ws=None, state=None) == FM_E_SHAPE


def test_byte_queries():
    lib = _lib.load()
    state, ws = lib.fm_linear_attention_state_bytes, lib.fm_linear_attention_workspace_bytes
    for dims in (WINDOW, (1, 1, 1, 8, 8), (130, 64, 64, 8, 8), (4000, 49, 25, 8, 8)):          # the window route
        assert state(*dims) == 0 and ws(*dims) == 0, dims
    for dims in ((0, 300, 200, 8, 32), (2, -1, 200, 8, 32), (2, 300, 0, 8, 32), (2, 300, 200, 8, 16), (2, 300, 200, 4, 32),
                 (3, 65, 49, 8, 8), (65536, 3, 3, 8, 32)):                                      # invalid or unsupported
        assert state(*dims) == 0 and ws(*dims) == 0, dims
    # the long route: the state is one slab per sample whatever L and S; the workspace grows with N and with S
    for n in (1, 2, 7):
        assert state(n, 300, 200, 8, 32) == n * SLAB
        assert state(n, 1, 4800, 8, 32) == n * SLAB
    by_n = [ws(n, 4800, 4800, 8, 32) for n in (1, 2, 3, 8)]
    assert by_n[0] > 0 and all(a < b for a, b in zip(by_n, by_n[1:]))
    by_s = [ws(1, 64, s, 8, 32) for s in (1, 64, 65, 129, 4800, 9600)]
    assert by_s[0] > 0 and all(a <= b for a, b in zip(by_s, by_s[1:])) and by_s[0] < by_s[3] < by_s[4] < by_s[5]
    for dims in (LONG, (1, 1, 1, 8, 32), (1, 4800, 4800, 8, 32), (3, 33, 700, 8, 32)):
        assert ws(*dims) % 256 == 0 and ws(*dims) >= SLAB
    # a bounded number of partial slabs per sample, however long the sequences
    assert ws(1, 1 << 20, 1 << 20, 8, 32) == ws(1, 1 << 24, 1 << 24, 8, 32) <= 257 * SLAB
