"""fm_coarse_tail_forward / _backward through the C ABI without a GPU: the entry points load, refuse bad arguments before
anything launches - in the header's order - and size their state and workspace."""
import ctypes as C

from featurematching_amd import _lib

FM_E_NULL, FM_E_SHAPE, FM_E_UNSUPPORTED, FM_E_WORKSPACE = -1, -2, -3, -4
NEW = ("fm_coarse_tail_state_bytes", "fm_coarse_tail_workspace_bytes", "fm_coarse_tail_forward", "fm_coarse_tail_backward")
FAKE = C.c_void_p(256)          # never dereferenced: every call below returns before it launches anything
INPUTS = ("x", "a", "w_merge", "ln1_w", "ln1_b", "w_mlp0", "w_mlp2", "ln2_w", "ln2_b")
GRADS = ("d_w_merge", "d_ln1_w", "d_ln1_b", "d_w_mlp0", "d_w_mlp2", "d_ln2_w", "d_ln2_b")
CHUNK, SPLIT, ROW_TOKENS = 8192, 512, 64         # kCtChunk, kCtSplit, kCtLnTok of csrc/coarse_tail.hip
TOKEN = (256 + 512 + 512 + 256 + 512 + 1) * 4    # bytes of a token's intermediates: m, c, h, o, dp, r1
SLAB = (512 * 512 + 256 * 512 + 256 * 256) * 4   # bytes of one split's partial weight gradients
ROW = 4 * 256 * 4                                # bytes of one LayerNorm workgroup's partial sums
MIB = 1 << 20


def test_symbols_load():
    _lib.load()                                                      # every name of the table resolves, or this raises
    for name in NEW:
        assert name in _lib.SIGNATURES
    enc = "fm_encoder_tail_"
    for name in NEW:                                                 # the argument lists are the d = 64 siblings'
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[enc + name[len("fm_coarse_tail_"):]]


def _calls(lib):
    def fwd(T=1000, d=256, eps=(1e-5, 1e-5), ws=FAKE, ws_bytes=1 << 40, state=None, **ptr):
        p = {k: FAKE for k in INPUTS + ("y",)}
        p.update(ptr)
        return lib.fm_coarse_tail_forward(*[p[k] for k in INPUTS], T, d, *eps, ws, ws_bytes, state, p["y"], None)

    def bwd(T=1000, d=256, eps=(1e-5, 1e-5), ws=FAKE, ws_bytes=1 << 40, state=None, **ptr):
        p = {k: FAKE for k in INPUTS + GRADS + ("d_y", "d_x", "d_a")}
        p.update(ptr)
        return lib.fm_coarse_tail_backward(*[p[k] for k in INPUTS], p["d_y"], state, T, d, *eps, ws, ws_bytes, p["d_x"],
                                           p["d_a"], *[p[k] for k in GRADS], None)
    return fwd, bwd


def test_argument_checks():
    lib = _lib.load()
    fwd, bwd = _calls(lib)
    need = lib.fm_coarse_tail_workspace_bytes(1000, 256)
    assert need > 0
    for call, own in ((fwd, ("y",)), (bwd, ("d_y", "d_x", "d_a"))):
        for missing in INPUTS + own:
            assert call(**{missing: None}) == FM_E_NULL, missing
        # the state query answers 0, so a NULL state (every call here) is no FM_E_NULL: the next check speaks
        assert lib.fm_coarse_tail_state_bytes(1000, 256) == 0 and call(state=None, ws_bytes=0) == FM_E_WORKSPACE
        for bad in (0, -1):
            assert call(T=bad) == FM_E_SHAPE
            assert call(d=bad) == FM_E_SHAPE
        for d in (32, 64, 128, 255, 257, 512):
            assert call(d=d) == FM_E_UNSUPPORTED, d
        assert call(T=(1 << 24) + 1) == FM_E_UNSUPPORTED
        assert call(T=1 << 24, ws_bytes=0) == FM_E_WORKSPACE         # 2^24 tokens are served
        for eps in (0.0, -1e-5, float("nan")):
            assert call(eps=(eps, 1e-5)) == FM_E_UNSUPPORTED, eps
            assert call(eps=(1e-5, eps)) == FM_E_UNSUPPORTED, eps
        assert call(ws_bytes=need - 1) == FM_E_WORKSPACE             # one byte short
        assert call(ws=C.c_void_p(264), ws_bytes=need) == FM_E_WORKSPACE
        assert call(ws=None, ws_bytes=need) == FM_E_WORKSPACE
        # a missing pointer is reported before a bad shape, a bad shape before an unsupported one, that before the workspace
        assert call(x=None, T=0, d=32, ws_bytes=0) == FM_E_NULL
        assert call(T=0, d=32, eps=(0.0, 0.0), ws_bytes=0) == FM_E_SHAPE
        assert call(d=64, ws_bytes=0) == FM_E_UNSUPPORTED
        assert call(eps=(0.0, 1e-5), ws_bytes=0) == FM_E_UNSUPPORTED
        assert call(ws_bytes=0) == FM_E_WORKSPACE


def test_gradient_pointers_all_or_none():
    lib = _lib.load()
    _, bwd = _calls(lib)
    none = {k: None for k in GRADS}
    assert bwd(ws_bytes=0, **none) == FM_E_WORKSPACE                 # all NULL passes the pointer check
    assert bwd(ws_bytes=0) == FM_E_WORKSPACE                         # and so do all seven
    for k in GRADS:
        assert bwd(**{k: None}) == FM_E_NULL, k                      # six of seven
        assert bwd(**{**none, k: FAKE}) == FM_E_NULL, k              # one of seven
    assert bwd(T=0, **{GRADS[0]: None}) == FM_E_NULL                 # before the shape


def _layout(T):
    """the workspace of csrc/coarse_tail.hip's ct_layout: regions from 256-byte boundaries"""
    n = min(CHUNK, (T + ROW_TOKENS - 1) // ROW_TOKENS * ROW_TOKENS)
    pad = lambda b: (b + 255) // 256 * 256
    regions = [n * 256 * 4, n * 512 * 4, n * 512 * 4, n * 256 * 4, n * 512 * 4, n * 4,
               (n + SPLIT - 1) // SPLIT * SLAB, n // ROW_TOKENS * ROW]
    return sum(pad(b) for b in regions)


def test_byte_queries():
    lib = _lib.load()
    state, ws = lib.fm_coarse_tail_state_bytes, lib.fm_coarse_tail_workspace_bytes
    for T in (1, 2, 127, 128, 129, 1000, 196000, 1 << 22, 1 << 24):
        assert state(T, 256) <= 16 * T
        assert 0 < ws(T, 256) <= 128 * MIB and ws(T, 256) % 256 == 0, T
        assert ws(T, 256) == _layout(T), T
    for T, d in ((1000, 32), (1, 64), (1000, 64), (1000, 512), (0, 256), (-1, 256), (1000, 0), ((1 << 24) + 1, 256)):
        assert state(T, d) == 0 and ws(T, d) == 0, (T, d)
    # a chunk's worth of tokens at the most: the size grows in steps of 64 tokens up to kCtChunk = 8192 and is the same
    # from there on, whatever the number of chunks
    assert ws(1, 256) == ws(64, 256) < ws(65, 256) == ws(128, 256)
    assert ws(128, 256) - ws(64, 256) == 64 * TOKEN + ROW            # (the same slab count: 512 tokens per slab)
    assert ws(513, 256) - ws(512, 256) == 64 * TOKEN + ROW + SLAB    # a second slab
    assert ws(CHUNK - 64, 256) < ws(CHUNK, 256) == ws(CHUNK + 1, 256) == ws(196000, 256) == ws(1 << 24, 256)
    assert ws(CHUNK, 256) == CHUNK * TOKEN + 16 * SLAB + 128 * ROW
