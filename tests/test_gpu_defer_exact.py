"""Deferred exact dot products of the screening on the GPU: switched off against switched on (fm_debug_defer_exact), bit
for bit.

With the deferral on (the common path's default), k_screen_rows lists an entry whose integer screening product proves it
significant for its row and its column with a tagged index (bit 30) and a stand-in value, without gathering the two
descriptor rows (tests/test_defer_model.py pins the rule on the CPU); k_select uses a stand-in only in the e / e = 1.0f of
an entry that is alone in its row's and in its column's list and forms the exact product - the screening's own
arithmetic, csrc/fm_exact_device.h - of every other tagged entry before anything reads it.  So every output of the coarse
stage must be IDENTICAL to the run with the deferral off: ids, conf bits, keypoints, count, status word, dense_cnt.  The
`on` run is also held against the float64 yardstick of tests/coarse_ref.py at the bars of tests/test_gpu_coarse_edges.py.

Pairs: the planted units of tests/test_gpu_unit_cert.py (its constructions, imported): L = S = 96, C in {256, 64},
N in {1, 3}; every pair holds ~90 lone peaks (the stand-in path) besides what is planted in unit (0, 0) of sample 0:
  one      a lone peak                                     -> stand-in kept (certified unit)
  two      two lone peaks in one unit                      -> stand-ins kept (swept unit: the hit walk's select chain)
  row      two partners in row 3 (cnt = 2)                 -> both resolved in the row's list
  col      two rows in column 5 (ccnt = 2)                 -> the one-entry rows 3 and 10 resolved through the column's list
  both     row 3 holds columns 5 and 20, column 5 rows 3 and 10
  tie      column 20 == column 5: the two conf must stay equal bit for bit
  above / below   the bisected second entry of test_gpu_unit_cert.py, just above / below row 3's integer threshold
  tails    L = 70 / S = 50 and L = 65 / S = 129
  float16 / bfloat16 descriptors; c_in = 40 (fewer 4-vectors than the 16 lanes of an entry) and c_in = 200
  cand_slots 4 and 16
  2 x 2 against 3 x 3 cells, N = 2: padding rows in the resolving wave, resolved entries in the second sample
  the dense resume: a peaked and a 'borderline' sample through fm_coarse_match_auto (one attempt: the flat sample's dense part
           is added to the common path's results, the peaked sample's tagged lists are read again)
  one 4800 x 4800, C = 256 'peaky' pair: most listed entries deferred.
The counter of deferred entries (counted with the switch at 2) must be 0 with the switch off and > 0 with it on wherever
the pair holds a lone peak - every case here: the test cannot pass with the feature silently off."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from featurematching_amd import _lib, synth

import coarse_ref as cr
import test_gpu_coarse_edges as edges
import test_gpu_unit_cert as uc

pytestmark = pytest.mark.gpu
OFF, ON = 1, 2
SHAPES = [(256, 1), (64, 3)]


def _extras(out):
    """deferred-entry counter, dense_cnt and the number of listed entries of a finished call, from its workspace"""
    lib = _lib.load()
    n, l, s, c = out['shape']
    lay = (C.c_int64 * 3)()
    assert lib.fm_debug_defer_exact_layout(n, l, s, c, out['slots'], lay, 3) == 0
    gen = (C.c_int64 * 41)()
    assert lib.fm_debug_coarse_layout(n, l, s, c, out['slots'], gen, 41) == 0
    assert lay[1] == 1 << 30
    o0 = out['base'] - out['ws'].data_ptr()

    def rd(off, count):
        return out['ws'][o0 + off:o0 + off + 4 * count].view(torch.int32).cpu().numpy()
    lp = int(gen[4])
    listed = np.minimum(rd(gen[10], n * lp).reshape(n, lp)[:, :l], out['slots'])
    return dict(count=int(rd(lay[0], 1)[0]), dense_cnt=rd(gen[34], n).copy(), listed=int(listed.sum()))


def _run(cs, mode, **kw):
    lib = _lib.load()
    prev = lib.fm_debug_defer_exact(mode)
    try:
        out = edges._call(cs, 0, **kw)
        out['x'] = _extras(out)
    finally:
        lib.fm_debug_defer_exact(prev)
    return out


def _off_on(cs, y=None, tag="", **kw):
    """both runs; identical outputs; the counter; the `on` run against the yardstick; returns the `on` run"""
    off, on = _run(cs, OFF, **kw), _run(cs, ON, **kw)
    assert off['st'] == 0 and on['st'] == 0, (off['st'], off['info'], on['st'], on['info'])
    assert (off['m'], off['info'], off['hint']) == (on['m'], on['info'], on['hint'])
    for k in ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_c', 'mkpts1_c'):
        assert off[k].tobytes() == on[k].tobytes(), k
    assert np.array_equal(off['x']['dense_cnt'], on['x']['dense_cnt'])
    print(f"DEFER {tag}: M {on['m']}  listed {on['x']['listed']}  deferred {on['x']['count']}")
    assert off['x']['count'] == 0 and 0 < on['x']['count'], (off['x']['count'], on['x']['count'])
    if y is not None:
        on['mode'], on['first'] = 0, None
        bad = edges._list_errors(on, y) or edges._value_errors(tag, ("defer_exact", tag), on, cs, y)
        assert not bad, bad
    return on


@functools.lru_cache(maxsize=None)
def _both(c, n):
    """row 3 holds columns 5 and 20 (0.9 x), column 5 rows 3 and 10 (0.9 x): the 'row' and 'col' plants of
    test_gpu_unit_cert.py at once"""
    f0, f1, idx = uc._base(4000 + c, n, 96, 96, c)
    uc._clear_unit00(idx)
    uc._plant(idx, 3, 5)
    f0, f1, idx = uc._base(4000 + c, n, 96, 96, c, idx)
    f0[0, idx[0][20]] *= 1e-4
    f1[0, 20] = 0.9 * f0[0, 3] + 0.4 * synth.normal(77, 9, (c,))
    f1[0, int(np.nonzero(idx[0] == 10)[0][0])] *= 1e-4
    f0[0, 10] = 0.9 * f0[0, 3] + 0.1 * synth.normal(78, 9, (c,))
    uc._finish(f0, f1, idx)
    return cr._case(f0, f1, uc.HW[96], uc.HW[96], border=0)


def _pairs_of(on, b, i=None, j=None):
    m = on['m']
    sel = on['b_ids'][:m] == b
    if i is not None:
        sel &= on['i_ids'][:m] == i
    if j is not None:
        sel &= on['j_ids'][:m] == j
    return sel


@pytest.mark.parametrize("c,n", SHAPES)
@pytest.mark.parametrize("name", ["one", "two", "row", "col", "tie"])
def test_planted_units_off_against_on(name, c, n):
    cs = uc._pair(name, c, n)
    on = _off_on(cs, uc._yard(name, c, n), f"{name} C={c} N={n}")
    assert on['x']['count'] >= 0.5 * on['x']['listed']          # the lone peaks of the pair
    if name == "tie":                                            # both tied entries, the same conf bits
        sel = _pairs_of(on, 0, i=3)
        assert sorted(on['j_ids'][:on['m']][sel].tolist()) == [5, 20]
        assert on['mconf'][:on['m']][sel][0].tobytes() == on['mconf'][:on['m']][sel][1].tobytes()


@pytest.mark.parametrize("c,n", SHAPES)
def test_two_partners_in_a_row_and_two_rows_in_a_column_at_once(c, n):
    cs = _both(c, n)
    _off_on(cs, cr.yardstick(cs), f"both C={c} N={n}")


@pytest.mark.parametrize("c,n", SHAPES)
def test_second_entry_just_above_and_just_below_the_row_threshold(c, n):
    """column 20 = alpha x column 5, alpha bisected on `runner-up > thr_r[3]` as in test_gpu_unit_cert.py"""
    def above(alpha):
        a = uc._run(uc._pair("scaled", c, n, alpha), uc.ON)['arrays']
        return int(a['umax2'][0, 0, 0]) > int(a['thr_r'][0, 3])
    lo, hi = 0.3, 1.0
    assert above(hi) and not above(lo)
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if above(mid) else (mid, hi)
    for alpha in (lo, hi):
        _off_on(uc._pair("scaled", c, n, alpha), uc._yard("scaled", c, n, alpha), f"scaled {alpha:.5f} C={c} N={n}")


@pytest.mark.parametrize("c,n", SHAPES)
@pytest.mark.parametrize("name", ["tails70", "tails65"])
def test_tails_off_against_on(name, c, n):
    _off_on(uc._pair(name, c, n), uc._yard(name, c, n), f"{name} C={c} N={n}")


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", ["row", "col"])
def test_half_precision_descriptors(name, dtype):
    base = uc._pair(name, 256, 1)
    cs = dict(base, f0=cr.round_to(base['f0'], dtype), f1=cr.round_to(base['f1'], dtype), dtype=dtype)
    _off_on(cs, cr.yardstick(cs), f"{name} {dtype}")


@pytest.mark.parametrize("c", [40, 200])
@pytest.mark.parametrize("name", ["row", "col"])
def test_channel_counts_below_the_padded_ones(name, c):
    """c_in = 40: 10 4-vectors for the 16 lanes of an entry; c_in = 200: the last of a lane's four vectors partly beyond"""
    _off_on(uc._pair(name, c, 1), uc._yard(name, c, 1), f"{name} c_in={c}")


@pytest.mark.parametrize("slots", [4, 16])
@pytest.mark.parametrize("name", ["row", "col"])
def test_cand_slots_4_and_16(name, slots):
    _off_on(uc._pair(name, 256, 1), uc._yard(name, 256, 1), f"{name} slots={slots}", slots=slots)


def test_padding_rows_share_the_wave_that_resolves():
    """2 x 2 against 3 x 3 cells, N = 2 (a grid of tests/coarse_ref.py): four rows per sample, so the lanes of padding rows
    sit in the wave whose groups of 16 lanes form the exact products - of BOTH samples: a resolving lane takes row, column
    and sample from the entry's lane.  Every partner-less column owns a significant entry, so rows hold several"""
    key = ("grid", 256, 4)
    assert cr.case(key)['f0'].shape[:2] == (2, 4)
    _off_on(cr.case(key), cr.yard(key), str(key))


def test_dense_resume_reads_the_tagged_lists_of_the_unflagged_sample():
    """sample 0 peaked ('col': a resolved pair besides the lone peaks), sample 1 'borderline' (unit-gain descriptors: the
    whole matrix lies inside the significance window, every unit holds more entries than the exact phase resolves):
    fm_coarse_match_auto answers in ONE attempt - the common path reports flat similarity, the dense part is added and
    the assignment runs again on the lists the screening left"""
    p = uc._pair("col", 256, 1)
    g0, g1 = synth.coarse_descriptors(40, 1, 96, 256, "borderline")
    cs = dict(p, f0=np.concatenate([p['f0'], g0]), f1=np.concatenate([p['f1'], g1]))
    on = _off_on(cs, cr.yardstick(cs), "dense resume", auto=True)
    assert (on['hint'] >> 24) & 0xff == 1 and on['hint'] & _lib.FM_MODE_DENSE
    assert on['x']['dense_cnt'][0] == 0 and on['x']['dense_cnt'][1] > 0
    assert _pairs_of(on, 0).sum() > 50


def test_one_headline_size_pair_off_against_on():
    """one 640x480 'peaky' pair (L = S = 4800, C = 256): identical outputs, most listed entries deferred"""
    f0, f1 = synth.coarse_descriptors(1017, 1, 4800, 256, "peaky")
    on = _off_on(cr._case(f0, f1, uc.HW[4800], uc.HW[4800]), tag="4800 x 4800")
    assert on['m'] > 3000 and on['x']['count'] > 0.5 * on['x']['listed']
