"""The unit certificate of the screening as a numpy model, against brute force (no GPU).

The max pass with the top-2 epilogue (k_max_i8<C, true>) publishes, for every 32 x 32 unit of the integer screening
product, its maximum M1, its second-largest valid entry M2 COUNTED WITH MULTIPLICITY (a tie gives M2 == M1; a unit with
one valid entry gives kQMasked) and the place of one entry equal to M1, encoded as the accumulator sees it:
(lane << 4) | register, lane = 32 * h + column, row = (register & 3) + 8 * (register >> 2) + 4 * h.  k_thresh publishes
the smallest integer threshold of every 32-row block and 32-column unit (padded lines carry 0x3fffffff).  k_screen_rows
parks entry (i, j) iff acc > min(thr_r[i], thr_c[j]); for a unit with M2 <= Tmin = min(block minimum, unit minimum) it
parks the entry at the published place iff M1 > min of ITS two thresholds and nothing else, without forming the unit.
This file pins that rule: the parked set of the model equals brute force's, entry for entry, on random tiles that are
built to hold ties, single valid entries, thresholds between the two largest values and fully padded units."""
import numpy as np
import pytest

K_Q_MASKED = -(1 << 30)
PAD_THR = 0x3FFFFFFF


def max_pass_top2(q, l, s):
    """step 1: (M1, M2, upos) per unit from the keys (value << 4) | register, as the kernel forms them"""
    lp, sp = q.shape
    nrb, nu = lp // 32, sp // 32
    m1 = np.empty((nrb, nu), np.int64)
    m2 = np.empty((nrb, nu), np.int64)
    upos = np.empty((nrb, nu), np.int64)
    masked = -(1 << 26)
    reg, lanes = np.arange(16), np.arange(64)
    for rb in range(nrb):
        for u in range(nu):
            rows = rb * 32 + ((reg & 3) + 8 * (reg >> 2))[None, :] + 4 * (lanes >> 5)[:, None]      # [lane][register]
            cols = np.broadcast_to(u * 32 + (lanes & 31)[:, None], rows.shape)
            v = np.where((rows >= l) | (cols >= s), masked, q[rows, cols].astype(np.int64))
            keys = (v << 4) | reg[None, :]
            flat = np.sort(keys.ravel())
            k1, k2 = flat[-1], flat[-2]
            lane = int(np.argmax((keys == k1).any(1)))   # the first lane that holds the largest key
            v1, v2 = k1 >> 4, k2 >> 4
            m1[rb, u] = K_Q_MASKED if v1 <= masked else v1
            m2[rb, u] = K_Q_MASKED if v2 <= masked else v2
            upos[rb, u] = (lane << 4) | (k1 & 15)
    return m1, m2, upos


def thresh_minima(thr_r, thr_c):
    """step 2"""
    return thr_r.reshape(-1, 32).min(1), thr_c.reshape(-1, 32).min(1)


def screen(q, l, s, thr_r, thr_c, m1, m2, upos, tmin_r, tmin_c, use_cert):
    """step 3: the parked set {(i, j)} and how many units the certificate resolved"""
    parked, ncert = set(), 0
    for rb in range(q.shape[0] // 32):
        for u in range(q.shape[1] // 32):
            if use_cert and m2[rb, u] <= min(tmin_r[rb], tmin_c[u]):
                ncert += 1
                g, lane = int(upos[rb, u]) & 15, int(upos[rb, u]) >> 4
                i = rb * 32 + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5)
                j = u * 32 + (lane & 31)
                if m1[rb, u] > min(thr_r[i], thr_c[j]):
                    parked.add((i, j))
                continue
            for i in range(rb * 32, min(rb * 32 + 32, l)):
                for j in range(u * 32, min(u * 32 + 32, s)):
                    if q[i, j] > min(thr_r[i], thr_c[j]):
                        parked.add((i, j))
    return parked, ncert


def brute(q, l, s, thr_r, thr_c):
    i, j = np.nonzero(q[:l, :s] > np.minimum(thr_r[:l, None], thr_c[None, :s]))
    return set(zip(i.tolist(), j.tolist()))


def second_largest_with_multiplicity(vals):
    v = np.sort(np.asarray(vals))
    return int(v[-2]) if v.size > 1 else K_Q_MASKED


@pytest.mark.parametrize("seed", range(12))
def test_parked_set_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    l, s = [(70, 50), (65, 97), (64, 64), (33, 33), (96, 40), (1, 1)][seed % 6]
    lp, sp = -(-l // 32) * 32, -(-s // 32) * 32
    span = [3, 40, 4000, 4_000_000][seed % 4]            # few distinct values -> ties; up to the int8 product's range
    q = rng.integers(-span, span + 1, (lp, sp)).astype(np.int64)
    for _ in range(3):                                   # peaks, some of them doubled exactly
        i, j = rng.integers(0, l), rng.integers(0, s)
        q[i, j] = 3 * span
        if rng.random() < 0.5:
            q[rng.integers(0, l), rng.integers(0, s)] = 3 * span
    # thresholds: mostly between the bulk and the peaks (a unit with one peak certifies), one line in sixty inside the
    # bulk (its units hold several significant entries and take the sweep)
    thr_r = rng.integers(span, 3 * span + 2, lp).astype(np.int64)
    thr_c = rng.integers(span, 3 * span + 2, sp).astype(np.int64)
    thr_r = np.where(rng.random(lp) < 1 / 60, rng.integers(-span, span + 1, lp), thr_r)
    thr_c = np.where(rng.random(sp) < 1 / 60, rng.integers(-span, span + 1, sp), thr_c)
    # unit (0, 0) certifies by construction: one peak, every other entry in the bulk, no threshold below the bulk's top
    q[:32, :32] = np.minimum(q[:32, :32], span)
    q[rng.integers(0, min(l, 32)), rng.integers(0, min(s, 32))] = 3 * span
    thr_r[:32] = rng.integers(span, 3 * span + 2, 32)
    thr_c[:32] = rng.integers(span, 3 * span + 2, 32)
    thr_r[l:], thr_c[s:] = PAD_THR, PAD_THR
    m1, m2, upos = max_pass_top2(q, l, s)
    for rb in range(lp // 32):                           # the top-2 itself, against sorting the unit's valid entries
        for u in range(sp // 32):
            valid = q[rb * 32:min(rb * 32 + 32, l), u * 32:min(u * 32 + 32, s)].ravel()
            assert m1[rb, u] == (valid.max() if valid.size else K_Q_MASKED)
            assert m2[rb, u] == second_largest_with_multiplicity(valid)
    tmin_r, tmin_c = thresh_minima(thr_r, thr_c)
    want = brute(q, l, s, thr_r, thr_c)
    got, ncert = screen(q, l, s, thr_r, thr_c, m1, m2, upos, tmin_r, tmin_c, True)
    assert got == want
    assert screen(q, l, s, thr_r, thr_c, m1, m2, upos, tmin_r, tmin_c, False)[0] == want
    assert ncert > 0 and m2[0, 0] <= min(tmin_r[0], tmin_c[0])       # (the certificate is exercised, not vacuous)


def test_a_tie_never_certifies_a_significant_unit():
    """two equal maxima above the thresholds: M2 == M1 > Tmin, the unit takes the sweep; below them it certifies as empty"""
    q = np.zeros((32, 32), np.int64)
    q[3, 5] = q[10, 20] = 100
    m1, m2, upos = max_pass_top2(q, 32, 32)
    assert m1[0, 0] == m2[0, 0] == 100
    for thr, cert, n in ((50, 0, 2), (100, 1, 0)):
        t = np.full(32, thr, np.int64)
        got, ncert = screen(q, 32, 32, t, t, m1, m2, upos, *thresh_minima(t, t), True)
        assert ncert == cert and len(got) == n


def test_a_unit_with_one_valid_entry_certifies():
    q = np.full((96, 160), 7, np.int64)
    m1, m2, upos = max_pass_top2(q, 65, 129)
    assert m1[2, 4] == 7 and m2[2, 4] == K_Q_MASKED and m1[2, 3] == m2[2, 3] == 7
    g, lane = int(upos[2, 4]) & 15, int(upos[2, 4]) >> 4
    assert ((g & 3) + 8 * (g >> 2) + 4 * (lane >> 5), lane & 31) == (0, 0)
