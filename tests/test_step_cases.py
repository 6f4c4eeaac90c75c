"""The input sets of tests/step_cases.py on the CPU: the oracle's match counts are the ones the replay schedules are
written for (they go up and down from one seed to the next, and the empty set has none), and no confidence of any set
lies within 4e-5 of the threshold, so a HIP step's match set must equal the oracle's with no guard band."""
import numpy as np
import pytest
import torch

import step_cases as sc
from oracle import matcher_ref as orc


def _conf(s):
    return orc.conf_matrix(torch.as_tensor(s['f0']), torch.as_tensor(s['f1']), 0.1).numpy()


@pytest.mark.parametrize("c,dist", sorted(sc.COUNTS))
def test_counts_and_guard_band(c, dist):
    singles, pairs = sc.COUNTS[(c, dist)]
    sets = [sc.input_set(dist, seed, 1, c, 5) for seed in sc.SEEDS] + [sc.input_set(dist, seed, 2, c, 5) for seed in (7001, 7003)]
    for s, want in zip(sets, singles + pairs):
        ref = orc.coarse_match(s['f0'], s['f1'], sc.HW_I, sc.HW_C, sc.HW_C, thr=sc.THR, border_rm=sc.BORDER_RM)
        m = int(ref['i_ids'].shape[0])
        gap = float(np.abs(_conf(s).astype(np.float64) - sc.THR).min())
        print(f"RPL step_cases {sc.name_of(s):34s} M {m:3d}  min |conf - thr| {gap:.3e}")
        assert m == want, (sc.name_of(s), m, want)
        assert gap > sc.GUARD, (sc.name_of(s), gap)
    steps = np.diff(singles)
    assert (steps < 0).any() and (steps > 0).any()          # from one seed to the next the count moves both ways


@pytest.mark.parametrize("c", [64, 256])
def test_empty_set_has_no_match(c):
    for n in (1, 2):
        s = sc.input_set("empty", 7001, n, c, 5)
        assert not s['f1'].any() and s['f0'].any()
        ref = sc.oracle_of(s)
        assert ref['i_ids'].shape[0] == 0
        assert float(np.abs(_conf(s) - sc.THR).min()) > sc.GUARD


def test_oracle_of_a_set_is_match_features():
    """the shared yardstick: same ids and counts as coarse_match, fine keypoints per match, and oracle_errors accepts it
    and rejects a count, an id, a confidence and a keypoint that are off"""
    s = sc.input_set("peaky", 7002, 1, 64, 7)
    ref = sc.oracle_of(s)
    m = ref['i_ids'].shape[0]
    assert m == 44 and ref['mkpts0_f'].shape == (m, 3) and ref['mkpts1_f'].shape == (m, 3)
    got = {k: np.concatenate([ref[k], ref[k][:3]]) for k in ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c", "mconf",
                                                             "mkpts0_f", "mkpts1_f")}      # capacity-sized: stale rows beyond M
    assert sc.oracle_errors(got, m, ref) == []
    assert sc.oracle_errors(got, m + 1, ref)
    for k, delta in (("j_ids", 1), ("mconf", 2e-5), ("mkpts1_f", 2e-3), ("mkpts0_c", 8)):
        off = dict(got)
        off[k] = got[k].copy()
        off[k][m - 1] += delta
        assert sc.oracle_errors(off, m, ref), k
    assert sc.bit_errors(got, got, m) == [] and sc.bit_errors(off, got, m) == ["mkpts0_c"]
