"""The three fm_dual_softmax_* entry points through the C ABI without a GPU: every single defect of an argument row is
refused with the status the entry point has always given it, and the pairs of defects on which the entry points differ
keep their precedence.  No call below launches anything: the pointers are never dereferenced.  The expected statuses
were read off the library as it was before the entry points shared one status function (dsm_status, csrc/dsm_grad.hip);
tools/dsm_status_sweep.py prints the whole table, pairs included, for two builds to compare."""
import ctypes as C

import pytest

from featurematching_amd import _lib

FM_OK, FM_E_NULL, FM_E_SHAPE, FM_E_UNSUPPORTED, FM_E_WORKSPACE = 0, -1, -2, -3, -4
FAKE = C.c_void_p(256)          # never dereferenced
N, L, S, CH = 1, 100, 90, 64
HEAD = ("feat0", "feat1", "n", "l", "s", "c", "t", "ofs_r", "sum_r", "pitch_r", "ofs_c", "sum_c", "pitch_c")
TAILS = {
    "fm_dual_softmax_conf_at": ("b_ids", "i_ids", "j_ids", "k", "conf", "stream"),
    "fm_dual_softmax_backward": ("b_ids", "i_ids", "j_ids", "gc", "k", "ws", "ws_bytes", "d_feat0", "d_feat1", "stream"),
    "fm_dual_softmax_backward_dense": ("g", "ws", "ws_bytes", "d_feat0", "d_feat1", "stream"),
}
VALUES = dict(n=N, l=L, s=S, c=CH, t=0.1, pitch_r=128, pitch_c=128, k=8, ws_bytes=1 << 30, stream=None)
POINTERS = {name: [a for a in HEAD + tail if a not in VALUES] for name, tail in TAILS.items()}
SIZES = (dict(n=0), dict(n=-3), dict(l=0), dict(s=0), dict(s=-3), dict(pitch_r=L - 1), dict(pitch_c=S - 1))
UNSUPPORTED = (dict(c=0), dict(c=6), dict(c=260), dict(t=0.0), dict(t=-1.0), dict(t=float("nan")))


def call(name, **changes):
    """the entry point on its valid row with `changes` applied (a pointer's name -> None or another address)"""
    row = {a: VALUES.get(a, FAKE) for a in HEAD + TAILS[name]}
    assert set(changes) <= set(row), (name, changes)
    row.update(changes)
    return getattr(_lib.load(), name)(*row.values())


@pytest.mark.parametrize("name", list(TAILS))
def test_every_single_defect(name):
    for ptr in POINTERS[name]:
        assert call(name, **{ptr: None}) == FM_E_NULL, ptr
    for bad in SIZES:
        assert call(name, **bad) == FM_E_SHAPE, bad
    if "k" in TAILS[name]:
        assert call(name, k=-1) == FM_E_SHAPE
    for bad in UNSUPPORTED:
        assert call(name, **bad) == FM_E_UNSUPPORTED, bad
    if "ws" in TAILS[name]:
        need = _lib.load().fm_dual_softmax_backward_workspace_bytes(N, L, S, CH)
        assert need > 0
        assert call(name, ws_bytes=need - 1) == FM_E_WORKSPACE
        assert call(name, ws=C.c_void_p(264), ws_bytes=need) == FM_E_WORKSPACE       # a valid row, misaligned


def test_conf_at_answers_an_empty_list_before_it_looks_at_anything():
    name = "fm_dual_softmax_conf_at"
    assert call(name, k=0) == FM_OK
    for ptr in POINTERS[name]:
        assert call(name, k=0, **{ptr: None}) == FM_OK, ptr
    assert call(name, k=0, n=0, c=6, t=0.0) == FM_OK
    # ... and at its lists before at K's sign
    assert call(name, k=-1, i_ids=None) == FM_E_NULL


def test_backward_needs_its_lists_only_when_it_has_entries():
    name = "fm_dual_softmax_backward"
    for ptr in ("b_ids", "i_ids", "j_ids", "gc"):
        assert call(name, **{ptr: None}, n=0) == FM_E_NULL, ptr                     # K > 0: NULL lists come before the sizes
        assert call(name, k=-1, **{ptr: None}) == FM_E_SHAPE, ptr
    need = _lib.load().fm_dual_softmax_backward_workspace_bytes(N, L, S, CH)
    none = dict(b_ids=None, i_ids=None, j_ids=None, gc=None)
    assert call(name, k=0, **none, ws_bytes=need - 1) == FM_E_WORKSPACE          # K = 0 gets as far as the workspace
    assert call(name, k=0, **none, d_feat1=None) == FM_E_NULL


@pytest.mark.parametrize("name", list(TAILS))
def test_precedence(name):
    """NULL, then the sizes, then what the kernels are not built for, then the workspace"""
    if "k" in TAILS[name]:
        assert call(name, k=-1, c=6) == FM_E_SHAPE
    assert call(name, n=0, feat1=None) == FM_E_NULL
    assert call(name, pitch_c=S - 1, t=0.0) == FM_E_SHAPE
    if "ws" in TAILS[name]:
        assert call(name, c=6, ws_bytes=16) == FM_E_UNSUPPORTED
        assert call(name, l=0, ws=C.c_void_p(264)) == FM_E_SHAPE
        assert call(name, ws=None, ws_bytes=16, c=6) == FM_E_NULL
