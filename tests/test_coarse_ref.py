"""Pins tests/coarse_ref.py - the float64 yardstick of tests/test_gpu_coarse_edges.py - without a GPU: against the
independent brute-force oracle, against the three reference-written known-answer fixtures, and the conditions that let
the GPU tests demand equal id lists (an empty undecided set, M > 0, a non-zero float32 error to measure against).
Lines starting with E32 are part of the record profiles/coarse_edges_accuracy.txt (`pytest -s`)."""
import numpy as np
import pytest

from helpers import load_kats
from oracle import matcher_ref as orc

import coarse_ref as cr


def _ids(y):
    return list(zip(y['b_ids'].tolist(), y['i_ids'].tolist(), y['j_ids'].tolist()))


@pytest.mark.parametrize("key", [("channel", 4, "borderline", "float32"), ("channel", 100, "mixed", "bfloat16"),
                                 ("grid", 100, 1), ("grid", 256, 3), ("grid", 100, 5), ("arg", "border1_peaky"),
                                 ("arg", "border3_peaky"), ("arg", "thr0p02"), ("arg", "temp1")])
def test_yardstick_against_the_bruteforce_oracle(key):
    cs, y = cr.case(key), cr.yard(key)
    bf = orc.coarse_match_bruteforce(cs['f0'], cs['f1'], cs['hw0'], cs['hw1'], cs.get('thr', 0.2), cs.get('border', 2),
                                     cs.get('temp', 0.1))
    assert [t[:3] for t in bf] == _ids(y)
    if bf:
        assert np.abs(np.array([t[3] for t in bf]) - y['mconf64']).max() <= 1e-13


def test_border_slicing_semantics():
    """oracle.mask_border: 0 removes nothing, half a grid side or more removes everything (the slices overlap)"""
    assert len(cr.yard(("arg", "border0_peaky"))['i_ids']) > len(cr.yard(("arg", "border1_peaky"))['i_ids']) > \
        len(cr.yard(("arg", "border2_peaky"))['i_ids']) > 0
    assert len(cr.yard(("arg", "border3_peaky"))['i_ids']) == 0 == len(cr.yard(("arg", "border3_borderline"))['i_ids'])
    y = cr.yard(("arg", "border2_peaky"))           # 6x7 keeps 2x3 cells, 9x5 keeps 5x1: different per image
    assert set((y['i_ids'] // 7).tolist()) <= {2, 3} and set((y['i_ids'] % 7).tolist()) <= {2, 3, 4}
    assert set((y['j_ids'] % 5).tolist()) == {2} and set((y['j_ids'] // 5).tolist()) <= {2, 3, 4, 5, 6}


FIXTURES = [("kats", n) for n in ("tie", "empty", "batch3", "rect_scale", "thr05_b1", "thr0p5_b0")] + \
           [("kats_r2", "scale_big")] + [("kats_r3", n) for n in cr.KATS_R3]


@pytest.mark.parametrize("fixture,name", FIXTURES)
def test_yardstick_against_the_reference_written_fixtures(fixture, name):
    """ids in order, keypoints bit for bit, mconf within the float32 reference's error of this input (e32) + 1 ulp"""
    key = ("kat", fixture, name)
    y, k = cr.yard(key), cr.case(key)['fixture']
    assert not len(y['undecided']), y['undecided'][:5]
    assert np.array_equal(y['b_ids'], k['b_ids']) and np.array_equal(y['i_ids'], k['i_ids']) and np.array_equal(y['j_ids'], k['j_ids'])
    assert y['mkpts0_c'].dtype == np.float32 and np.array_equal(y['mkpts0_c'], k['mkpts0_c']) and np.array_equal(y['mkpts1_c'], k['mkpts1_c'])
    if len(k['mconf']):
        assert np.abs(y['mconf64'] - k['mconf']).max() <= y['e32_conf'] + 2.0 ** -24


def test_the_c32_and_the_straddle_fixtures():
    """C = 32 (kats 'tie', 'empty') is below the smallest padded count; the thr straddle of kats_r2 is UNDECIDED by
    construction (one entry one ulp from thr) and the yardstick says so"""
    assert cr.case(("kat", "kats", "tie"))['f0'].shape[2] == 32
    for name in ("thr_below", "thr_above"):
        key = ("kat", "kats_r2", name)
        i_s, j_s = [int(v) for v in cr.case(key)['fixture']['straddle']]
        assert [tuple(u) for u in cr.yard(key)['undecided'].tolist()] == [(0, i_s, j_s)]


def test_constructed_ties_keep_both_entries_with_the_same_bits():
    r3 = [int(v) for v in cr.case(("kat", "kats_r3", "c100_tie"))['fixture']['tie']]
    for key, b, cols in ((("kat", "kats", "tie"), 0, (28, 35)), (("kat", "kats_r3", "c100_tie"), r3[0], r3[2:])):
        y = cr.yard(key)
        sel = (y['b_ids'] == b) & np.isin(y['j_ids'], cols)
        assert sel.sum() == 2 and len(set(y['i_ids'][sel].tolist())) == 1
        assert y['mconf64'][sel][0] == y['mconf64'][sel][1]
        m = cr.case(key)['fixture']['mconf'][sel]
        assert m[0].tobytes() == m[1].tobytes()


def test_one_row_against_many_columns_is_the_column_softmax_alone():
    """L = 1: the softmax over dim 1 is 1 everywhere, conf = the softmax over dim 2"""
    import torch
    y = cr.yard(("grid", 100, 1))
    assert torch.equal(y['conf64'], torch.softmax(y['sim64'], 2)) and y['lse_c'].equal(y['sim64'][:, 0])
    y = cr.yard(("grid", 256, 0))                   # one cell each: conf == 1
    assert y['conf64'].flatten().tolist() == [1.0, 1.0] and len(y['i_ids']) == 2


@pytest.mark.parametrize("group", ["channel_float32", "channel_float16", "channel_bfloat16", "batch", "grid", "arg", "train", "kat"])
def test_every_gpu_case_is_decided(group):
    """the undecided set is empty, M > 0 unless the border removes everything, the float32 reference has an error"""
    keys = [k for k in cr.gpu_case_keys() if (k[0] + "_" + k[3] if k[0] == "channel" else k[0]) == group]
    assert keys
    for key in keys:
        y = cr.yard(key)
        m = len(y['i_ids'])
        print(f"E32 {str(key):48s} M {m:4d} (float32 oracle {len(y['matches32']['i_ids']):4d})  e32_conf {y['e32_conf']:.3e}  "
              f"e32_lse {y['e32_lse']:.3e}  undecided {len(y['undecided'])}")
        assert not len(y['undecided']), (key, y['undecided'][:5])
        assert (m == 0) if cr.built_empty(key) else (m > 0), key
        one_by_one = key[0] == "grid" and cr.GRIDS[key[2]] == ((1, 1), (1, 1))       # conf == 1 in any arithmetic
        assert y['e32_conf'] > 0 or one_by_one, key
        assert y['e32_lse'] > 0 or one_by_one or y['lse_r'].abs().max() == 0, key
        if key[0] == "train":
            assert len(cr.supervision(key)) > 60
        cr.yard.cache_clear()
