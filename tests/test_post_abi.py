"""fm_epipolar_errors through the C ABI without a GPU: the entry point loads and refuses bad arguments before anything
launches, in the header's order (an empty list first, then missing pointers, then shapes)."""
import ctypes as C

from featurematching_amd import _lib

FM_OK, FM_E_NULL, FM_E_SHAPE = 0, -1, -2
FAKE = C.c_void_p(1024)         # never dereferenced: every call below returns before it launches anything
REQUIRED = ("mkpts0", "mkpts1", "m_bids", "T_0to1", "K0", "K1", "epi_errs")
OPTIONAL = ("d_count", "inlier", "per_pair")


def call(lib, kpt_stride=2, m_max=300, N=2, thr=1e-4, **kw):
    p = {k: FAKE for k in REQUIRED + OPTIONAL}
    p.update(kw)
    return lib.fm_epipolar_errors(p["mkpts0"], p["mkpts1"], kpt_stride, p["m_bids"], p["d_count"], m_max, N, p["T_0to1"], p["K0"],
                                  p["K1"], thr, p["epi_errs"], p["inlier"], p["per_pair"], None)


def test_symbol_loads():
    _lib.load()                                                      # every name of the table resolves, or this raises
    assert "fm_epipolar_errors" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["fm_epipolar_errors"]
    assert restype == C.c_int
    assert len(argtypes) == 15


def test_argument_checks():
    """every call passes N <= 0, a stride below 2 or a missing pointer, so none reaches the launch (there is no GPU here)"""
    lib = _lib.load()
    for missing in REQUIRED:
        assert call(lib, **{missing: None}) == FM_E_NULL, missing
        assert call(lib, N=0, kpt_stride=1, **{missing: None}) == FM_E_NULL, missing      # a missing pointer comes first
    for kw in (dict(N=0), dict(N=-1), dict(m_max=-1), dict(m_max=-300), dict(kpt_stride=1), dict(kpt_stride=0), dict(kpt_stride=-2),
               dict(N=0, kpt_stride=3), dict(m_max=1, N=-5)):
        assert call(lib, **kw) == FM_E_SHAPE, kw
    # the optional pointers may be missing: the shape is still what is refused
    for optional in OPTIONAL:
        assert call(lib, N=0, **{optional: None}) == FM_E_SHAPE, optional
    assert call(lib, N=0, d_count=None, inlier=None, per_pair=None) == FM_E_SHAPE


def test_empty_list_is_served_before_any_check():
    """m_max = 0: nothing to do and nothing launched, whatever else is passed (an empty tensor has no address)"""
    lib = _lib.load()
    assert call(lib, m_max=0) == FM_OK
    assert call(lib, m_max=0, **{k: None for k in REQUIRED + OPTIONAL}) == FM_OK
    assert call(lib, m_max=0, N=0, kpt_stride=0) == FM_OK
