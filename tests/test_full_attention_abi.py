"""fm_full_attention_forward / _backward through the C ABI without a GPU: the entry points load, refuse bad arguments
before anything launches, in the order the header states, and size their state and workspace."""
import ctypes as C

from featurematching_amd import _lib

FM_E_NULL, FM_E_SHAPE, FM_E_UNSUPPORTED, FM_E_WORKSPACE = -1, -2, -3, -4
NEW = ("fm_full_attention_state_bytes", "fm_full_attention_workspace_bytes", "fm_full_attention_forward",
       "fm_full_attention_backward")
FAKE = C.c_void_p(256)          # never dereferenced: every call below returns before it launches anything
FINE, COARSE = (3, 25, 49, 8, 8), (2, 300, 200, 8, 32)
UNSUPPORTED = ((2, 300, 200, 8, 16), (2, 300, 200, 4, 32), (2, 300, 200, 4, 8), (2, 300, 200, 16, 16), (2, 300, 200, 8, 64),
               (1 << 18, 32, 32, 8, 32), (1, 1 << 23, 1, 8, 32), (1, 1, 1 << 25, 8, 8))      # the last three: 2^31 elements


def _up256(x):
    return (x + 255) // 256 * 256


def test_symbols_load():
    _lib.load()                                                      # every name of the table resolves, or this raises
    for name in NEW:
        assert name in _lib.SIGNATURES


def _calls(lib):
    def fwd(q=FAKE, k=FAKE, v=FAKE, dims=COARSE, ws=FAKE, ws_bytes=1 << 40, state=FAKE, out=FAKE, **_):
        return lib.fm_full_attention_forward(q, k, v, *dims, ws, ws_bytes, state, out, None)

    def bwd(q=FAKE, k=FAKE, v=FAKE, dims=COARSE, ws=FAKE, ws_bytes=1 << 40, state=FAKE, out=FAKE, g=FAKE, dq=FAKE, dk=FAKE,
            dv=FAKE):
        return lib.fm_full_attention_backward(q, k, v, out, g, state, *dims, ws, ws_bytes, dq, dk, dv, None)
    return fwd, bwd


def test_argument_checks():
    lib = _lib.load()
    fwd, bwd = _calls(lib)
    for call in (fwd, bwd):
        for dims in (COARSE, FINE):
            for missing in ("q", "k", "v", "out", "ws"):
                assert call(dims=dims, **{missing: None}) == FM_E_NULL, missing
        for i in range(5):                                           # N, L, S, H, D: zero and negative
            for bad in (0, -1):
                dims = list(COARSE)
                dims[i] = bad
                assert call(dims=dims) == FM_E_SHAPE, dims
        for dims in UNSUPPORTED:
            assert call(dims=dims) == FM_E_UNSUPPORTED, dims
        for dims in (COARSE, FINE):
            need = lib.fm_full_attention_workspace_bytes(*dims)
            assert need > 0
            assert call(dims=dims, ws_bytes=need - 1) == FM_E_WORKSPACE          # one byte short
            assert call(dims=dims, ws=C.c_void_p(264), ws_bytes=need) == FM_E_WORKSPACE
        # a missing pointer is reported before a bad shape, a bad shape before an unsupported one, that before the workspace
        assert call(q=None, dims=(0, 300, 200, 8, 16), ws_bytes=0) == FM_E_NULL
        assert call(dims=(0, 300, 200, 8, 16), ws_bytes=0) == FM_E_SHAPE
        assert call(dims=(0, 300, 200, 8, 16), ws=None, ws_bytes=0) == FM_E_SHAPE        # no workspace to miss: its query is 0
        assert call(dims=(2, 300, 200, 8, 16), ws_bytes=0) == FM_E_UNSUPPORTED
        assert call(dims=(2, 300, 200, 8, 16), ws=None, ws_bytes=0) == FM_E_UNSUPPORTED
        assert call(ws_bytes=0) == FM_E_WORKSPACE
    # the state: NULL is the forward's inference call (it gets as far as the workspace check), the backward needs it
    assert fwd(state=None, ws_bytes=0) == FM_E_WORKSPACE
    assert bwd(state=None) == FM_E_NULL
    for missing in ("g", "out", "dq", "dk", "dv"):
        assert bwd(**{missing: None}) == FM_E_NULL, missing
        assert bwd(dims=(0, 300, 200, 8, 16), **{missing: None}) == FM_E_NULL, missing


def test_byte_queries():
    lib = _lib.load()
    state, ws = lib.fm_full_attention_state_bytes, lib.fm_full_attention_workspace_bytes
    for dims in ((0, 300, 200, 8, 32), (2, -1, 200, 8, 32), (2, 300, 0, 8, 32), (2, 300, 200, 0, 32), (2, 300, 200, 8, 0)) \
            + UNSUPPORTED:
        assert state(*dims) == 0 and ws(*dims) == 0, dims
    for dims in (FINE, COARSE, (1, 1, 1, 8, 8), (1, 1, 1, 8, 32), (4000, 49, 25, 8, 8), (1, 4800, 4800, 8, 32), (3, 33, 700, 8, 32),
                 (70000, 3, 3, 8, 8)):
        n, l, s, h, d = dims
        assert state(*dims) == _up256(4 * n * l * h), dims
        assert ws(*dims) > 0 and ws(*dims) % 256 == 0, dims
        assert ws(*dims) <= 4 * (n * l + 2 * n * s) * h * d + 256, dims            # at most q + k + v, + 256
    # not of order L * S
    assert ws(1, 1 << 14, 1 << 14, 8, 32) <= 3 * 4 * (1 << 14) * 256 + 256
    by_n = [ws(n, 4800, 4800, 8, 32) for n in (1, 2, 3, 8)]
    assert all(a <= b for a, b in zip(by_n, by_n[1:])) and by_n[0] < by_n[-1]
    # just below the element bound
    assert ws((1 << 18) - 1, 32, 32, 8, 32) > 0 and state(1, (1 << 23) - 1, 1, 8, 32) > 0


def test_batch_is_not_bounded_by_a_grid_dimension():
    """N = 70000 is beyond a 65535 grid limit: the shape passes the UNSUPPORTED check and fails only on its workspace"""
    lib = _lib.load()
    fwd, bwd = _calls(lib)
    dims = (70000, 3, 3, 8, 8)
    need = lib.fm_full_attention_workspace_bytes(*dims)
    assert need == _up256(4 * 70000 * 3 * 8)
    assert fwd(dims=dims, ws_bytes=need - 1) == FM_E_WORKSPACE
    assert bwd(dims=dims, ws_bytes=need - 1) == FM_E_WORKSPACE
