"""tests/dsm_grad_ref.py pinned on the CPU: its closed-form gradients against float64 autograd through the reference's
expression (coarse_matching_new.py:64-68; the loss cases through tests/coarse_loss_ref.py as well), its term bound, its
handed statistics, and - for every case of the table tests/test_gpu_dsm_grad.py runs - the condition the case is named
for, on the reference alone."""
import numpy as np
import pytest
import torch

import coarse_loss_ref as clr
import dsm_grad_ref as dr

SMALL = [n for n, c in dr.CASES.items() if c.N <= 2]


def _modes(name):
    return [(name, m) for m in dr.CASES[name].modes]


def _close(tag, got, want, bound, rel):
    """|got - want| <= rel * bound elementwise (bound == 0: equal)"""
    for side in range(2):
        err = np.abs(got[side] - want[side])
        assert np.all(err <= rel * bound[side]), (tag, side, float((err / np.maximum(bound[side], 1e-300)).max()))


@pytest.mark.parametrize("name,mode", [p for n in SMALL + ["split_n85"] for p in _modes(n)])
def test_closed_form_equals_float64_autograd_within_1e12_of_the_term_bound(name, mode):
    c, d, r = dr.CASES[name], dr.build(name), dr.reference(name, mode)
    a0, a1, conf = dr.autograd(d['f0'], d['f1'], c.temp, r['g_dense'])
    _close((name, mode), (a0, a1), r['ref'], r['T'], 1e-12)
    assert np.abs(conf.numpy() - d['sm']['conf']).max() <= 1e-14
    if mode in dr.LOSSES:            # the whole chain descriptors -> conf -> loss in one autograd graph
        b0 = torch.as_tensor(d['f0'], dtype=torch.float64).requires_grad_(True)
        b1 = torch.as_tensor(d['f1'], dtype=torch.float64).requires_grad_(True)
        cm = clr.conf_matrix(b0, b1, dr.t32(c.temp))
        loss = clr.masked_loss(cm, clr.gt_mask(cm.shape, *torch.as_tensor(d['ids']).T), mode, lo=clr.LO32, hi=clr.HI32)
        loss[0].backward()
        _close((name, mode, "loss"), (b0.grad.numpy(), b1.grad.numpy()), r['ref'], r['T'], 1e-12)
        assert abs(loss[0].item() - r['loss64'][0]) <= 1e-13 * abs(r['loss64'][0])


@pytest.mark.parametrize("name", list(dr.CASES))
def test_term_bound_holds_and_case_conditions(name):
    c, d = dr.CASES[name], dr.build(name)
    sm, ids = d['sm'], d['ids']
    assert c.C % 4 == 0 and 4 <= c.C <= 256
    assert np.all((ids >= 0) & (ids < np.array([c.N, c.L, c.S]))), "an id outside its range"
    assert len(ids) == {"none": 0, "one": 1, "k1025": 1025}.get(c.entries, len(ids))
    if c.entries not in ("none",):
        assert len(ids) > 0
    if c.skip is not None:
        assert c.N > c.skip and not np.any(ids[:, 0] == c.skip) and np.any(ids[:, 0] != c.skip)
    if c.bits:                       # bit-reproducible listed entries: no row and no column twice
        assert len({(b, i) for b, i, _ in ids.tolist()}) == len(ids) == len({(b, j) for b, _, j in ids.tolist()})
    if c.entries == "triple3":
        assert sum(tuple(t) == tuple(ids[0]) for t in ids.tolist()) == 3
    if c.entries == "row":
        assert len(set(ids[:, 1].tolist())) == 1 and len(ids) == c.S
    if c.entries == "col":
        assert len(set(ids[:, 2].tolist())) == 1 and len(ids) == c.L
    if any(m in dr.LOSSES for m in c.modes):      # the loss takes DISTINCT triples
        assert len({tuple(t) for t in ids.tolist()}) == len(ids) > 0
    if c.z is not None:
        assert (dr.zsplit(c.N, c.L), dr.zsplit(c.N, c.S)) == c.z
    for mode in c.modes:
        r = dr.reference(name, mode)
        for side in range(2):
            assert np.all(np.abs(r['ref'][side]) <= r['T'][side] * (1 + 1e-12)), (mode, side)
            assert np.all(np.isfinite(r['T'][side])) and r['U'][side].shape == (c.N, 1, c.C) and r['U'][side].max() < 1e-33
        if mode == "dense0" or (mode == "sparse" and c.entries == "none"):
            assert r['T'][0].max() == 0 and r['T'][1].max() == 0
        elif c.skip is not None and mode == "sparse":
            assert r['T'][0][c.skip].max() == 0 and r['T'][1][c.skip].max() == 0 and r['T'][0].max() > 0
        else:
            assert r['T'][0].max() > 0 and r['T'][1].max() > 0
        if c.kind == "saturated":
            ratio = max(np.abs(r['ref'][s]).max() / r['T'][s].max() for s in range(2))
            assert ratio < 1e-3, (mode, ratio)
    if c.kind == "soft":             # what the loss runs on: 1 / (1 - conf) < 20, entries either side of the clamp's lower bound
        assert sm['conf'].max() < 0.95 and 0 < (sm['conf'] < clr.LO32).sum() < sm['conf'].size // 20
    assert c.kind == "soft" or not any(m in dr.LOSSES for m in c.modes)
    if c.kind == "peaky":
        assert sm['conf'][ids[:, 0], ids[:, 1], ids[:, 2]].min() > 1 - 1e-3 and np.abs(sm['sim']).max() > 100
    if c.kind == "flat":
        assert np.abs(sm['A'] - 1.0 / c.L).max() <= 1e-12 and np.abs(sm['B'] - 1.0 / c.S).max() <= 1e-12
    if c.kind == "scaled":
        row = min(c.L - 1, dr.SCALED_ROW)
        assert row % 32 not in (0, 31) or c.L <= 2
        assert np.abs(sm['sim'][:, row]).max() > 10 * np.abs(np.delete(sm['sim'], row, 1)).max() / 3


def test_the_table_holds_every_split_and_edge_the_kernels_have():
    assert {z for c in dr.CASES.values() if c.z for z in c.z} == {1, 2, 3, 4}
    assert dr.CASES["split33x33"].z == (4, 4) and -(-33 // 32) == 2          # Z = 4 over 2 tiles: two empty slices
    assert [dr.zsplit(n, 33) for n in (85, 86, 127, 128, 255, 256)] == [4, 3, 3, 2, 2, 1]
    assert [dr.zsplit(1, 1), dr.zsplit(2, 4800), dr.zsplit(16, 1024), dr.zsplit(1000, 64)] == [4, 2, 1, 1]
    assert len(dr.REGULAR) > 40 and all(dr.CASES[n].kind in ("borderline", "soft") for n in dr.REGULAR)


@pytest.mark.parametrize("name", ["tile33x97", "data_peaky", "temp0.05", "chan68"])
def test_handed_statistics(name):
    """the statistics restate the two softmaxes in the kernels' convention; NaN beyond L and S; delta is what it says"""
    c, d = dr.CASES[name], dr.build(name)
    ofs_r, sum_r, ofs_c, sum_c, delta = dr.stats(d['f0'], d['f1'], c.temp, c.L + 7, c.S + 1)
    assert ofs_r.shape == (c.N, c.L + 7) and sum_c.shape == (c.N, c.S + 1) and ofs_r.dtype == sum_c.dtype == np.float32
    assert np.isnan(ofs_r[:, c.L:]).all() and np.isnan(sum_r[:, c.L:]).all() and np.isnan(ofs_c[:, c.S:]).all()
    assert np.isfinite(ofs_r[:, :c.L]).all() and np.isfinite(sum_c[:, :c.S]).all()
    y = d['sm']['x'] * dr.k2_f32(c.C, c.temp)
    a = np.exp2(y + ofs_c[:, None, :c.S].astype(np.float64)) / sum_c[:, None, :c.S]
    b = np.exp2(y + ofs_r[:, :c.L, None].astype(np.float64)) / sum_r[:, :c.L, None]
    # k2's float32 rounding (2^-24 relative) times the distance from the maximum, and the two float32 roundings of a pair
    slack = 2.0 ** -23 * (1 + np.abs(d['sm']['sim']).max() * 2)
    assert np.abs(a - d['sm']['A']).max() <= slack and np.abs(b - d['sm']['B']).max() <= slack
    assert 0.999 <= sum_r[:, :c.L].min() and sum_r[:, :c.L].max() <= c.S * (1 + 1e-6)
    assert 0 < delta <= slack
    assert delta == max(dr.stats_delta(ofs_r[:, :c.L], sum_r[:, :c.L], d['sm']['lse_r']),
                        dr.stats_delta(ofs_c[:, :c.S], sum_c[:, :c.S], d['sm']['lse_c']))
