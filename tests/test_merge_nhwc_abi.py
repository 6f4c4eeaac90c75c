"""fm_gather_merge_windows_nhwc (crop + context merge on channels-last maps): every status the host decides, with
pointers that are never dereferenced - each call returns before it launches (runs without a GPU)."""
import ctypes as C

from featurematching_amd import _lib

OK, E_NULL, E_SHAPE, E_UNSUPPORTED = 0, -1, -2, -3


def _call(lib, **kw):
    one = C.c_void_p(256)        # a non-NULL address that is never dereferenced on these paths
    a = dict(feat_f0=one, feat_f1=one, map_dtype=_lib.FM_F32, N=1, Cf=64, Hf0=8, Wf0=8, Hf1=8, Wf1=8, W=7, stride=4, pad=2,
             h0c=2, w0c=2, h1c=2, w1c=2, packed_w=one, ctx0=one, ctx1=one, b_ids=one, i_ids=one, j_ids=one, d_count=None,
             m_max=3, out0=one, out1=one, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.fm_gather_merge_windows_nhwc(*a.values())


ONE_IMAGE = dict(feat_f1=None, ctx1=None, j_ids=None, out1=None, Hf1=0, Wf1=0, h1c=0, w1c=0)


def test_no_matches_is_a_no_op_whatever_else_is_passed():
    lib = _lib.load()
    assert _call(lib, m_max=0) == OK
    assert _call(lib, m_max=0, feat_f0=None, feat_f1=None, packed_w=None, ctx0=None, ctx1=None, b_ids=None, i_ids=None,
                 j_ids=None, out0=None, out1=None) == OK
    assert _call(lib, m_max=0, Cf=32, W=9, map_dtype=9, N=0) == OK


def test_null_pointers_two_image_form():
    lib = _lib.load()
    for name in ("feat_f0", "packed_w", "ctx0", "ctx1", "b_ids", "i_ids", "j_ids", "out0", "out1"):
        assert _call(lib, **{name: None}) == E_NULL, name
    # NULL comes before the shape and the support checks, as in the family
    assert _call(lib, out0=None, Cf=32, N=0) == E_NULL


def test_null_pointers_one_image_form():
    """feat_f1 == NULL: ctx1, j_ids, out1 and the image-1 sizes are ignored (NULL / 0 pass the checks); what image 0
    needs is still required."""
    lib = _lib.load()
    for name in ("feat_f0", "packed_w", "ctx0", "b_ids", "i_ids", "out0"):
        assert _call(lib, **dict(ONE_IMAGE, **{name: None})) == E_NULL, name
    # the one-image form gets past the NULL and shape checks without image 1's arguments: Cf = 32 is what stops it
    assert _call(lib, **dict(ONE_IMAGE, Cf=32)) == E_UNSUPPORTED
    assert _call(lib, **dict(ONE_IMAGE, W=9)) == E_UNSUPPORTED


def test_shapes():
    lib = _lib.load()
    assert _call(lib, m_max=-1) == E_SHAPE
    for name in ("N", "Hf0", "Wf0", "Hf1", "Wf1", "stride", "h0c", "w0c", "h1c", "w1c"):
        for bad in (0, -3):
            assert _call(lib, **{name: bad}) == E_SHAPE, (name, bad)
    for name in ("N", "Hf0", "Wf0", "stride", "h0c", "w0c"):
        assert _call(lib, **dict(ONE_IMAGE, **{name: 0})) == E_SHAPE, name
    assert _call(lib, **dict(ONE_IMAGE, m_max=-1)) == E_SHAPE
    # a bad shape is reported ahead of an unsupported one
    assert _call(lib, Hf0=0, Cf=32) == E_SHAPE


def test_unsupported():
    lib = _lib.load()
    for cf in (32, 128, 0):
        assert _call(lib, Cf=cf) == E_UNSUPPORTED
    for w in (9, 3, 15, 0):
        assert _call(lib, W=w) == E_UNSUPPORTED
    for dt in (3, -1, 17):
        assert _call(lib, map_dtype=dt) == E_UNSUPPORTED
        assert _call(lib, **dict(ONE_IMAGE, map_dtype=dt)) == E_UNSUPPORTED
