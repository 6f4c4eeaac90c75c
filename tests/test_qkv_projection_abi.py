"""fm_qkv_projection_forward / _backward through the C ABI without a GPU: the entry points load, refuse bad arguments
before anything launches - in the header's order - and size their workspace."""
import ctypes as C

from featurematching_amd import _lib

FM_E_NULL, FM_E_SHAPE, FM_E_UNSUPPORTED, FM_E_WORKSPACE = -1, -2, -3, -4
NEW = ("fm_qkv_projection_workspace_bytes", "fm_qkv_projection_forward", "fm_qkv_projection_backward")
X, SRC = C.c_void_p(256), C.c_void_p(512)      # never dereferenced: every call below returns before it launches anything
FAKE = C.c_void_p(1024)
WEIGHTS = ("wq", "wk", "wv")
GRADS = ("d_wq", "d_wk", "d_wv")
FRAG = 6 * 4096 * 4             # bytes of the weights in the kernels' operand order, forward and backward
SLAB = 3 * 4096 * 4             # bytes of one workgroup's partial weight gradients
MIB = 1 << 20


def test_symbols_load():
    _lib.load()                                                      # every name of the table resolves, or this raises
    for name in NEW:
        assert name in _lib.SIGNATURES


def _calls(lib):
    def fwd(Tx=1000, Ts=900, d=64, ws=FAKE, ws_bytes=1 << 40, **ptr):
        p = {"x": X, "src": SRC, **{k: FAKE for k in WEIGHTS + ("q", "k", "v")}}
        p.update(ptr)
        return lib.fm_qkv_projection_forward(p["x"], p["src"], *[p[k] for k in WEIGHTS], Tx, Ts, d, ws, ws_bytes, p["q"],
                                             p["k"], p["v"], None)

    def bwd(Tx=1000, Ts=900, d=64, ws=FAKE, ws_bytes=1 << 40, **ptr):
        p = {"x": X, "src": SRC, **{k: FAKE for k in WEIGHTS + GRADS + ("gq", "gk", "gv", "d_x", "d_src")}}
        p.update(ptr)
        return lib.fm_qkv_projection_backward(p["x"], p["src"], *[p[k] for k in WEIGHTS], p["gq"], p["gk"], p["gv"], Tx, Ts, d,
                                              ws, ws_bytes, p["d_x"], p["d_src"], *[p[k] for k in GRADS], None)
    return fwd, bwd


def test_argument_checks():
    lib = _lib.load()
    fwd, bwd = _calls(lib)
    need = lib.fm_qkv_projection_workspace_bytes(1000, 900, 64)
    assert need > 0
    for call, own in ((fwd, ("q", "k", "v")), (bwd, ("gq", "gk", "gv", "d_x"))):
        for missing in ("x", "src") + WEIGHTS + own:
            assert call(**{missing: None}) == FM_E_NULL, missing
        for bad in (0, -1):
            assert call(Tx=bad) == FM_E_SHAPE
            assert call(Ts=bad) == FM_E_SHAPE
            assert call(d=bad) == FM_E_SHAPE
        for d in (32, 63, 65, 128, 256):
            assert call(d=d) == FM_E_UNSUPPORTED, d
        assert call(Tx=(1 << 24) + 1) == FM_E_UNSUPPORTED
        assert call(Ts=(1 << 24) + 1) == FM_E_UNSUPPORTED
        assert call(Tx=1 << 22, Ts=1 << 24, ws_bytes=0) == FM_E_WORKSPACE    # 2^22 and 2^24 tokens are served
        assert call(ws_bytes=need - 1) == FM_E_WORKSPACE             # one byte short
        assert call(ws=C.c_void_p(1024 + 8), ws_bytes=need) == FM_E_WORKSPACE
        assert call(ws=None, ws_bytes=need) == FM_E_WORKSPACE
        # a missing pointer is reported before a bad shape, a bad shape before an unsupported one, that before the workspace
        assert call(x=None, Tx=0, d=32, ws_bytes=0) == FM_E_NULL
        assert call(Tx=0, d=32, ws_bytes=0) == FM_E_SHAPE
        assert call(d=32, ws_bytes=0) == FM_E_UNSUPPORTED
        assert call(ws_bytes=0) == FM_E_WORKSPACE


def test_self_mode_is_the_same_address():
    lib = _lib.load()
    fwd, bwd = _calls(lib)
    for call in (fwd, bwd):
        assert call(src=X, Tx=1000, Ts=1000, ws_bytes=0) == FM_E_WORKSPACE   # self mode passes every check before the workspace
        assert call(src=X, Tx=1000, Ts=900) == FM_E_SHAPE            # one tensor, two lengths
        assert call(src=X, Tx=1000, Ts=900, d=32, ws_bytes=0) == FM_E_SHAPE  # before the unsupported d
        assert call(src=X, Tx=1000, Ts=900, wq=None) == FM_E_NULL    # and behind a missing pointer
        assert call(Tx=1000, Ts=900, ws_bytes=0) == FM_E_WORKSPACE   # two tensors, two lengths: cross mode
    # d_src: not looked at in self mode, required in cross mode - before the shape
    assert bwd(src=X, Tx=1000, Ts=1000, d_src=None, ws_bytes=0) == FM_E_WORKSPACE
    assert bwd(d_src=None) == FM_E_NULL
    assert bwd(d_src=None, Tx=0) == FM_E_NULL


def test_gradient_pointers_all_or_none():
    lib = _lib.load()
    _, bwd = _calls(lib)
    none = {k: None for k in GRADS}
    assert bwd(ws_bytes=0, **none) == FM_E_WORKSPACE                 # all NULL passes the pointer check
    assert bwd(ws_bytes=0) == FM_E_WORKSPACE                         # and so do all three
    for k in GRADS:
        assert bwd(**{k: None}) == FM_E_NULL, k                      # two of three
        assert bwd(**{**none, k: FAKE}) == FM_E_NULL, k              # one of three
        assert bwd(src=X, Ts=1000, **{k: None}) == FM_E_NULL, k      # in self mode too
    assert bwd(Tx=0, **{GRADS[0]: None}) == FM_E_NULL                # before the shape


def test_workspace_query():
    ws = _lib.load().fm_qkv_projection_workspace_bytes
    counts = (1, 2, 127, 128, 129, 1000, 32768, 32769, 196000, 1 << 22, 1 << 24)
    for Tx in counts:
        for Ts in counts:
            assert 0 < ws(Tx, Ts, 64) <= 64 * MIB and ws(Tx, Ts, 64) % 256 == 0, (Tx, Ts)
    for Tx, Ts, d in ((1000, 1000, 32), (1, 1, 32), (1000, 1000, 256), (0, 5, 64), (5, 0, 64), (-1, 5, 64), (5, -1, 64),
                      (1000, 1000, 0), ((1 << 24) + 1, 5, 64), (5, (1 << 24) + 1, 64)):
        assert ws(Tx, Ts, d) == 0, (Tx, Ts, d)
    # it does not decrease with either token count
    for other in (1, 1000, 1 << 24):
        sizes = [ws(T, other, 64) for T in counts]
        assert sizes == sorted(sizes)
        sizes = [ws(other, T, 64) for T in counts]
        assert sizes == sorted(sizes)
    # the operand fragments and one slab per workgroup of the backward: a workgroup per 128 tokens of x and per 128 of src
    # (the query does not know the mode and sizes for cross mode), at most 256 of them - constant from there on
    assert ws(1, 1, 64) == ws(128, 128, 64) == FRAG + 2 * SLAB
    assert ws(129, 128, 64) - ws(128, 128, 64) == SLAB and ws(128, 129, 64) - ws(128, 128, 64) == SLAB
    assert ws(128 * 128, 128 * 128, 64) == FRAG + 256 * SLAB
    assert ws(128 * 128, 128 * 128, 64) == ws(1 << 24, 1 << 24, 64) == ws(1 << 24, 1, 64) == ws(1, 1 << 24, 64)
