"""The numbers a run is judged by, at the edges the scene tests leave out: the pose estimate (csrc/pose.hip) with intrinsics
of its own for every pair and image, with pixel thresholds other than 1, with more pairs than matches and on degenerate
geometry; the epipolar errors (csrc/post.hip) over several workgroups, under a count in every form, with ids that are no
pair, on exact geometry and for a pure rotation.  The yardsticks are tests/pose_ref.py's: the float64 restatement of the
pose estimate and the float64 formula of the epipolar distance.

The epipolar distance is measured in the residual: with d = r^2 w, |sqrt(d) - sqrt(d64)| <= c eps32 S sqrt(w64), S the sum
of the absolute values of the products r = p1 . E p0 is made of (pose_ref.residual_bound says why).  c is not the
kernel's: the same measure of a plain float32 NumPy transcription of the formula against float64 is 0.6999 at most over
this file's cases (pose_ref.transcription_measure, pinned by tests/test_pose_ref.py), and c = 4 x that = 2.800; the factor
of four allows for another order of summation and for fused multiply-adds.
"""
import functools

import numpy as np
import pytest
import torch

import pose_ref as pr
from featurematching_amd import post

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_FLOAT32 = 4 * pr.transcription_measure()


def dev(x):
    return torch.as_tensor(x, device=DEV)


def call(k0, k1, bids, K0, K1, **kw):
    out = post.estimate_poses(dev(k0), dev(k1), dev(bids), dev(K0), dev(K1), **kw)
    return {k: getattr(out, k).cpu().numpy() for k in out._fields}


def epipolar(k0, k1, bids, T, K0, K1, **kw):
    epi, inl, per = post.epipolar_errors(dev(k0), dev(k1), dev(bids), dev(T), dev(K0), dev(K1), **kw)
    return epi.cpu().numpy(), inl.cpu().numpy(), per.cpu().numpy()


edge_scene = functools.lru_cache(maxsize=None)(pr.edge_scene)


# ---- pose: intrinsics, thresholds ---------------------------------------------------------------------------------------
def same_as_restatement(out, b, ref, sc=None):
    """pair `b` of `out` is the restatement's `ref`: the same decision, counts and mask, the same candidate to the rounding
    of two root finders (the tolerances of test_gpu_pose.test_noise_free_scene); sc: angles against its ground truth"""
    assert bool(out["ok"][b]) == ref["ok"]
    assert int(out["per_pair"][b, 1]) == ref["inliers"] and int(out["per_pair"][b, 2]) == ref["votes"]
    E = out["E"][b].ravel()
    assert min(np.abs(E - ref["E"]).max(), np.abs(E + ref["E"]).max()) <= 1e-9
    if sc is not None and ref["ok"]:
        r_err, t_ang = pr.rotation_angle_deg(out["R"][b], sc["R"]), pr.vector_angle_deg(out["t"][b], sc["t"])
        r_ref, t_ref = pr.rotation_angle_deg(ref["R"], sc["R"]), pr.vector_angle_deg(ref["t"], sc["t"])
        print(f"pair {b}: R_err {r_err:.3e} (restatement {r_ref:.3e}), t angle {t_ang:.3e} ({t_ref:.3e}) degrees")
        assert abs(r_err - r_ref) <= 1e-6 and abs(t_ang - t_ref) <= 1e-6


def truth_mask(sc, pixel_thr=1.0):
    q0, q1 = pr.normalise(sc["k0"], sc["K0"]), pr.normalise(sc["k1"], sc["K1"])
    return pr.sampson(sc["E"].ravel(), q0, q1) < pr.threshold2(sc["K0"], sc["K1"], pixel_thr)


def test_every_pair_and_image_has_its_own_intrinsics():
    scenes = [edge_scene(f"intr{b}") for b in range(3)]
    k0, k1, bids, K0, K1, _ = pr.batch(scenes)
    assert not np.array_equal(K0, K1) and len({K.tobytes() for K in list(K0) + list(K1)}) == 6
    out = call(k0, k1, bids, K0, K1, samples=256, seed=0)
    pr.check_bookkeeping(out, k0, k1, bids, K0, K1)
    for b, sc in enumerate(scenes):
        ref = pr.estimate(sc["k0"], sc["k1"], K0[b], K1[b], seed=0, b=b, samples=256)
        assert ref["ok"]
        same_as_restatement(out, b, ref, sc)
        assert np.array_equal(out["inliers"][bids == b], truth_mask(sc))


def test_pixel_threshold():
    sc = edge_scene("thr")
    k0, k1, bids, K0, K1, _ = pr.batch([sc])
    refs = [pr.estimate(sc["k0"], sc["k1"], K0[0], K1[0], seed=0, samples=256, pixel_thr=thr) for thr in pr.PIXEL_THRS]
    assert len({ref["inliers"] for ref in refs}) == 3       # a threshold that is ignored cannot give all three
    for thr, ref in zip(pr.PIXEL_THRS, refs):
        out = call(k0, k1, bids, K0, K1, samples=256, seed=0, pixel_thr=thr)
        pr.check_bookkeeping(out, k0, k1, bids, K0, K1, pixel_thr=thr)
        assert ref["ok"]
        same_as_restatement(out, 0, ref, sc)
        assert np.array_equal(out["inliers"], ref["mask"])


# ---- pose: more pairs than matches ----------------------------------------------------------------------------------------
PAIRS = 300


@pytest.mark.parametrize("live", [(7, 298), (0,), (PAIRS - 1,)])
def test_more_pairs_than_matches(live):
    """N + 1 > m_max, and N + 1 > 256: the segments, the winners' words and the thresholds of most pairs are written by
    threads that own no match, those of the last pairs by a second workgroup"""
    k0, k1, bids, K0, K1, _ = pr.sparse_batch(PAIRS, live)
    assert len(k0) == 40 and sorted(set(bids)) == sorted(live) and len({K.tobytes() for K in K0}) == PAIRS
    out = call(k0, k1, bids, K0, K1, samples=64, seed=4)
    pr.check_bookkeeping(out, k0, k1, bids, K0, K1)
    assert list(np.flatnonzero(out["per_pair"][:, 0])) == sorted(live) and not out["ok"][np.setdiff1d(np.arange(PAIRS), live)].any()
    for b in live:
        rows = bids == b
        ref = pr.estimate(k0[rows], k1[rows], K0[b], K1[b], seed=4, b=b, samples=64)
        assert ref["ok"]
        same_as_restatement(out, b, ref)
        alone = call(k0[rows], k1[rows], bids[rows], K0, K1, samples=64, seed=4)     # the same pair with no other in the list
        for key in ("R", "t", "E", "per_pair", "ok"):
            assert np.array_equal(alone[key][b], out[key][b]), key
        assert np.array_equal(alone["inliers"], out["inliers"][rows])


# ---- pose: degenerate geometry ----------------------------------------------------------------------------------------------
def test_planar_scene():
    """every point on one plane: the five-point solver has no planar degeneracy, and the answer is the restatement's (the
    seed is one where the true essential matrix beats its planar twin on the redrawn matches: pose_ref.EDGE_SCENES)"""
    sc = edge_scene("planar")
    k0, k1, bids, K0, K1, _ = pr.batch([sc])
    out = call(k0, k1, bids, K0, K1, samples=256, seed=0)
    pr.check_bookkeeping(out, k0, k1, bids, K0, K1)
    ref = pr.estimate(sc["k0"], sc["k1"], K0[0], K1[0], seed=0, samples=256)
    assert ref["ok"]
    same_as_restatement(out, 0, ref, sc)
    assert np.array_equal(out["inliers"], truth_mask(sc))
    assert pr.same_bits(call(k0, k1, bids, K0, K1, samples=256, seed=0), out)


def degenerate(name):
    intr0, intr1 = pr.pair_intrinsics(5)
    if name == "rotation":
        return pr.pure_rotation(90, 64, intr0=intr0, intr1=intr1)
    return pr.repeated(91, 64, distinct=8 if name == "repeated" else 1, intr0=intr0, intr1=intr1)


@pytest.mark.parametrize("name", ["rotation", "repeated", "one_row"])
def test_degenerate_geometry(name):
    """a pure rotation, eight matches repeated, one match repeated: whether a sample yields a candidate is rounding luck, so
    only what holds for any outcome is asked (check_bookkeeping, any_outcome) - and the same bits twice"""
    k0, k1, bids, K0, K1, _ = pr.batch([degenerate(name)])
    for samples in (64, 256):
        out = call(k0, k1, bids, K0, K1, samples=samples, seed=0)
        print(f"{name}, {samples} samples: per_pair {out['per_pair'][0].tolist()}")
        pr.check_bookkeeping(out, k0, k1, bids, K0, K1, any_outcome=True)
        assert int(out["per_pair"][0, 1]) == int(out["inliers"].sum())
        assert pr.same_bits(call(k0, k1, bids, K0, K1, samples=samples, seed=0), out)


# ---- epipolar errors --------------------------------------------------------------------------------------------------------
case = functools.lru_cache(maxsize=None)(pr.epipolar_case)
reference = functools.lru_cache(maxsize=None)(pr.epipolar_reference)


def check_epipolar(got, bids, n, d64, S, w, thr):
    """epi within the bound of d64 in the residual, NaN where d64 is; flags as float64's wherever the bound cannot decide
    the comparison otherwise; per_pair exact given the flags"""
    epi, inl, per = got
    exists = ~np.isnan(d64)
    assert np.array_equal(np.isnan(epi), ~exists) and not inl[~exists].any()
    bound = pr.residual_bound(S[exists], w[exists], C_FLOAT32)
    err = np.abs(np.sqrt(epi[exists].astype(np.float64)) - np.sqrt(d64[exists]))
    print(f"largest |sqrt(d) - sqrt(d64)| / (eps32 S sqrt(w)) {(err / bound).max() * C_FLOAT32:.4f} (allowed {C_FLOAT32:.4f})")
    assert (err <= bound).all()
    # d < thr in float32 can differ from d64 < thr only where sqrt(thr) lies within the bound of sqrt(d64)
    sure = np.abs(np.sqrt(d64[exists]) - np.sqrt(float(np.float32(thr)))) > bound
    assert np.array_equal(inl[exists][sure], (d64[exists] < float(np.float32(thr)))[sure])
    live = np.asarray(bids)[exists]
    assert per[:, 0].tolist() == np.bincount(live, minlength=n).tolist()
    assert per[:, 1].tolist() == np.bincount(live, weights=inl[exists], minlength=n).astype(np.int64).tolist()
    return int((~sure).sum())


@pytest.mark.parametrize("thr", [1e-4, 1e-6])
@pytest.mark.parametrize("stride", [2, 3])
def test_epipolar_errors_over_three_workgroups(stride, thr):
    k0, k1, bids, T, K0, K1 = case("noisy")
    assert len(k0) == 700 and len(T) == 3
    junk = np.full((len(k0), stride - 2), 7.5, np.float32)
    got = epipolar(np.hstack([k0, junk]), np.hstack([k1, junk]), bids, T, K0, K1, inlier_thr=thr)
    check_epipolar(got, bids, 3, *reference("noisy"), thr)
    inliers = got[2][:, 1]
    assert 0 < inliers.sum() < 700 and (thr == 1e-4 or inliers.sum() < 400)     # 1e-6 splits the noisy inliers themselves
    if stride == 3:
        plain = epipolar(k0, k1, bids, T, K0, K1, inlier_thr=thr)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, plain))


COUNTS = (0, 1, 255, 256, 257, 700, 705, -3)


@functools.lru_cache(maxsize=None)
def truncated(rows):
    k0, k1, bids, T, K0, K1 = case("noisy")
    return epipolar(k0[:rows], k1[:rows], bids[:rows], T, K0, K1, inlier_thr=1e-6)


@pytest.mark.parametrize("form", ["device_int32", "device_int64", "host"])
def test_epipolar_errors_under_a_count(form):
    """rows behind the count do not exist: NaN, not inliers, in no pair's counters; the rows in front are the truncated
    list's, bit for bit.  The count may be an int32 or int64 tensor on the device or a tensor on the host"""
    k0, k1, bids, T, K0, K1 = case("noisy")
    for value in COUNTS:
        count = {"device_int32": lambda: torch.tensor([value], dtype=torch.int32, device=DEV),
                 "device_int64": lambda: torch.tensor([value], dtype=torch.int64, device=DEV),
                 "host": lambda: torch.tensor(value, dtype=torch.int64)}[form]()
        epi, inl, per = epipolar(k0, k1, bids, T, K0, K1, inlier_thr=1e-6, count=count)
        rows = max(0, min(value, len(k0)))
        assert np.isnan(epi[rows:]).all() and not inl[rows:].any(), value
        e_ref, i_ref, p_ref = truncated(rows)
        assert np.array_equal(epi[:rows], e_ref) and np.array_equal(inl[:rows], i_ref) and np.array_equal(per, p_ref), value
        assert per[:, 0].tolist() == np.bincount(bids[:rows], minlength=3).tolist(), value
        assert not np.isnan(e_ref).any()


FOREIGN = (-1, -2, 3, 10, 2 ** 32, 2 ** 32 + 1, -2 ** 32)


def test_epipolar_errors_with_ids_that_are_no_pair():
    """ids outside [0, N) - N and N + 7, negative ones, and ones whose low 32 bits alone would name a pair - are NaN, not
    inliers and counted nowhere; the rest is the list without them; estimate_poses counts the same rows per pair"""
    k0, k1, bids, T, K0, K1 = case("noisy")
    M = len(k0) + 3 * len(FOREIGN)
    at = np.sort(np.argsort(pr.synth.hash_u64(12, 3, M), kind="stable")[:3 * len(FOREIGN)])   # where the foreign rows go
    ours = np.setdiff1d(np.arange(M), at)
    w0, w1, wb = (np.zeros((M,) + a.shape[1:], a.dtype) for a in (k0, k1, bids))
    w0[ours], w1[ours], wb[ours] = k0, k1, bids
    w0[at], w1[at], wb[at] = k0[:len(at)], k1[:len(at)], np.tile(np.array(FOREIGN, np.int64), 3)   # real keypoints, no pair
    assert at.min() < 256 < at.max() and (np.diff(wb) < 0).any()
    epi, inl, per = epipolar(w0, w1, wb, T, K0, K1, inlier_thr=1e-6)
    assert np.isnan(epi[at]).all() and not inl[at].any()
    e_ref, i_ref, p_ref = truncated(len(k0))
    assert np.array_equal(epi[ours], e_ref) and np.array_equal(inl[ours], i_ref) and np.array_equal(per, p_ref)
    assert per[:, 0].tolist() == np.bincount(bids, minlength=3).tolist()
    poses = call(w0, w1, wb, K0, K1, samples=64, seed=0, sorted_bids=False)
    assert poses["per_pair"][:, 0].tolist() == per[:, 0].tolist() and not poses["inliers"][at].any()


def test_epipolar_errors_of_exact_geometry():
    """matches projected in float64 and rounded to float32 lie on their lines to rounding: d is within the bound of 0"""
    k0, k1, bids, T, K0, K1 = case("exact")
    d64, S, w = reference("exact")
    got = epipolar(k0, k1, bids, T, K0, K1)
    assert check_epipolar(got, bids, 3, d64, S, w, 1e-4) == 0 and got[1].all()
    bound = pr.residual_bound(S, w, C_FLOAT32)
    print(f"largest sqrt(d) / bound {(np.sqrt(got[0].astype(np.float64)) / bound).max():.3f}, of float64 {(np.sqrt(d64) / bound).max():.3f}")
    assert (got[0].astype(np.float64) <= bound ** 2).all()


def test_epipolar_errors_of_a_pure_rotation():
    """t = 0: E = 0, r = 0 and w = inf, so d is NaN - in float64 as in float32 - and no match is an inlier by accident"""
    k0, k1, bids, T, K0, K1 = case("rotation")
    assert not T[0, :3, 3].any()
    d64, _, _ = reference("rotation")
    assert np.isnan(d64).all()
    for thr in (1e-4, np.inf):
        epi, inl, per = epipolar(k0, k1, bids, T, K0, K1, inlier_thr=thr)
        assert np.isnan(epi).all() and not inl.any() and per.tolist() == [[len(k0), 0]]
