"""The pose estimate without a GPU: the metric functions of post.py against the reference's own (tests/golden/
pose_metrics.npz, written by tests/golden/make_golden_pose_metrics.py), the NumPy restatement of the device solver
(tests/pose_ref.py) on noise-free samples, its sampling, and what the Python entry points decide on the host."""
import os
import time

import numpy as np
import pytest
import torch

import pose_ref as pr
from featurematching_amd import post, synth

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_metrics.npz"))
# the restatement evaluates the reference's float64 expressions; a sum may associate differently by an ulp or two
TOL = 1e-12


def test_relative_pose_error_matches_the_reference():
    for p in range(GOLD["T"].shape[0]):
        t_err, R_err = post.relative_pose_error(GOLD["T"][p], GOLD["R"][p], GOLD["t"][p])
        assert abs(t_err - GOLD["t_err"][p]) <= TOL and abs(R_err - GOLD["R_err"][p]) <= TOL * 180, p
    assert GOLD["t_err"][0] == 0 and GOLD["R_err"][1] == 0           # (the fixture holds the exact and the clipped case)
    # t_err is a distance between translations, not an angle: doubling t changes it
    T, R, t = GOLD["T"][3], GOLD["R"][3], GOLD["t"][3]
    assert abs(post.relative_pose_error(T, R, 2 * t)[0] - np.linalg.norm(T[:3, 3] - 2 * t)) <= TOL


def test_error_auc_matches_the_reference():
    for k in "abcde":
        got = post.error_auc(list(GOLD[f"auc_in_{k}"]), [1, 2, 3], ret_dict=False)
        assert np.abs(np.array(got) - GOLD[f"auc_{k}"]).max() <= TOL, k
    d = post.error_auc(list(GOLD["auc_in_a"]), [1, 2, 3])
    assert list(d) == ["auc@5", "auc@10", "auc@20"]                   # the thresholds argument is ignored, as there


def test_epidist_prec_matches_the_reference():
    for k, n in (("a", 4), ("b", 1), ("c", 2)):
        errs = np.array([GOLD[f"epi_{k}_{j}"] for j in range(n)] + [None], dtype=object)[:n]
        got = post.epidist_prec(errs, list(GOLD["prec_thr"]), ret_dict=False)
        assert np.abs(np.array(got, np.float64) - GOLD[f"prec_{k}"]).max() <= TOL, k
    assert list(post.epidist_prec([GOLD["epi_a_0"]], [5e-4])) == ["prec@5e-04"]


def test_aggregate_metrics_matches_the_reference():
    ids = GOLD["agg_ids"]
    metrics = {"identifiers": [f"pair{i}" for i in ids], "R_errs": list(GOLD["agg_R"]), "t_errs": list(GOLD["agg_t"]),
               "epi_errs": [GOLD[f"agg_epi_{j}"] for j in range(len(ids))]}
    got = post.aggregate_metrics(metrics, epi_err_thr=5e-4)
    assert list(got) == ["auc@5", "auc@10", "auc@20", "prec@5e-04"]
    assert np.abs(np.array(list(got.values()), np.float64) - GOLD["agg_out"]).max() <= TOL
    # of a repeated identifier the last index counts: changing an earlier duplicate changes nothing
    metrics["R_errs"][0] = 1e3
    again = post.aggregate_metrics(metrics, epi_err_thr=5e-4)
    assert list(again.values()) == list(got.values())


@pytest.mark.parametrize("roots", ["numpy", "dk"])
def test_restatement_recovers_the_true_essential_matrix(roots):
    for seed in pr.SOLVER_SEEDS:
        q0, q1, E_true = pr.exact_samples(seed, 200)
        t0 = time.perf_counter()
        Es, count = pr.solve5(q0, q1, roots)
        # vectorised over hypotheses: 200 with np.roots take about 30 ms, the bar is a second (the Durand-Kerner
        # restatement is for experiments and is not timed)
        assert roots != "numpy" or time.perf_counter() - t0 < 1.0
        found = pr.found_true(Es, count, E_true)
        assert found.sum() >= 196, (seed, roots, int(found.sum()))    # at least 98 %
        assert count.max() <= 10 and count.min() >= 0
        E3 = Es.reshape(200, 10, 3, 3)
        Et = np.swapaxes(E3, 2, 3)
        res = np.linalg.norm(2 * E3 @ Et @ E3 - np.trace(E3 @ Et, axis1=2, axis2=3)[..., None, None] * E3, axis=(2, 3))
        live = np.arange(10)[None] < count[:, None]
        assert res[live].max() <= 1e-9
        assert np.abs(np.linalg.norm(Es, axis=2)[live] - 1).max() <= 1e-12
        h = np.concatenate([q0, np.ones((200, 5, 1))], 2), np.concatenate([q1, np.ones((200, 5, 1))], 2)
        epi = np.abs(np.einsum("hpi,hcij,hpj->hcp", h[1], E3, h[0])).max(2)
        assert epi[live].max() <= 1e-9


def test_sampling_is_the_documented_hash():
    idx, valid = pr.sample_indices(5, 3, 37, 300)
    assert valid.all() or valid.sum() >= 290
    key = synth._stream_key(5, 3)
    for h in (0, 1, 17, 299):
        with np.errstate(over="ignore"):
            draws = [int(synth._splitmix64(np.array([np.uint64(8 * h + k) * synth._GOLD + key], np.uint64))[0] % np.uint64(37))
                     for k in range(8)]
        first = list(dict.fromkeys(draws))
        assert bool(valid[h]) == (len(first) >= 5)
        if valid[h]:
            assert list(idx[h]) == first[:5]
    assert all(len(set(r)) == 5 and min(r) >= 0 and max(r) < 37 for r in idx[valid])
    assert not pr.sample_indices(5, 3, 4, 16)[1].any()               # fewer than five matches: no hypothesis
    some = pr.sample_indices(5, 3, 5, 64)[1]
    assert some.any() and not some.all()                              # five matches: only draws that hit all five
    assert not np.array_equal(pr.sample_indices(5, 4, 37, 8)[0], pr.sample_indices(5, 3, 37, 8)[0])


def test_restatement_estimates_a_noise_free_pose():
    sc = pr.scene(11, 120, outliers=0.3)
    est = pr.estimate(sc["k0"], sc["k1"], sc["K"], sc["K"], seed=0, samples=64)
    assert est["ok"] and est["votes"] == est["inliers"]
    q0, q1 = pr.normalise(sc["k0"], sc["K"]), pr.normalise(sc["k1"], sc["K"])
    truth = pr.sampson(sc["E"].ravel(), q0, q1) < pr.threshold2(sc["K"], sc["K"])
    assert np.array_equal(est["mask"], truth)
    assert pr.rotation_angle_deg(est["R"], sc["R"]) < 0.05 and pr.vector_angle_deg(est["t"], sc["t"]) < 0.5
    assert not pr.estimate(sc["k0"][:4], sc["k1"][:4], sc["K"], sc["K"])["ok"]


def test_gpu_scenes_have_no_match_on_the_threshold():
    """tests/test_gpu_pose.py compares inlier masks exactly; a match whose distance to the TRUE essential matrix lies
    within 1e-9 (relative) of the threshold would make that a coin toss.  None of the seeded scenes has one."""
    for name, kw in pr.SCENES.items():
        sc = pr.scene(**kw)
        q0, q1 = pr.normalise(sc["k0"], sc["K"]), pr.normalise(sc["k1"], sc["K"])
        assert not pr.in_band(sc["E"], q0, q1, pr.threshold2(sc["K"], sc["K"])).any(), name


@pytest.mark.parametrize("name", pr.NOISE_FREE)
def test_restatement_finds_the_ground_truth_inliers_of_the_noise_free_scenes(name):
    sc = pr.scene(**pr.SCENES[name])
    q0, q1 = pr.normalise(sc["k0"], sc["K"]), pr.normalise(sc["k1"], sc["K"])
    truth = pr.sampson(sc["E"].ravel(), q0, q1) < pr.threshold2(sc["K"], sc["K"])
    for roots in ("numpy", "dk"):
        est = pr.estimate(sc["k0"], sc["k1"], sc["K"], sc["K"], seed=0, samples=256, roots=roots)
        assert est["ok"] and np.array_equal(est["mask"], truth), roots
        assert pr.rotation_angle_deg(est["R"], sc["R"]) < 0.01 and pr.vector_angle_deg(est["t"], sc["t"]) < 0.1
        if name in pr.BACKWARD:          # the pose is the -t decomposition the name stands for
            R, t = pr.decompose(est["E"])[pr.BACKWARD[name]]
            assert np.array_equal(R, est["R"]) and np.array_equal(t, est["t"])


# ---- the scenes and yardsticks of tests/test_gpu_post_edges.py ------------------------------------------------------------
def test_intrinsics_are_optional_and_existing_scenes_keep_theirs():
    for name, kw in pr.SCENES.items():
        sc = pr.scene(**kw)
        assert np.array_equal(sc["K"], pr.K) and np.array_equal(sc["K0"], pr.K) and np.array_equal(sc["K1"], pr.K), name
    k0, k1, bids, K0, K1, T = pr.batch([pr.scene(**pr.SCENES["noisy64"]), pr.edge_scene("intr2")])
    assert np.array_equal(K0[0], pr.K) and np.array_equal(K1[0], pr.K) and K0.dtype == K1.dtype == np.float32
    sc = pr.edge_scene("intr2")
    assert np.array_equal(K0[1], sc["K0"]) and np.array_equal(K1[1], sc["K1"]) and not np.array_equal(sc["K0"], sc["K1"])
    assert bids.tolist() == [0] * 64 + [1] * 70 and T.shape == (2, 4, 4)
    # the exact normalised coordinates are the float32 keypoints' under the scene's own intrinsics, to float32's rounding
    assert np.abs(pr.normalise(sc["k0"], sc["K0"]) - sc["q0"]).max() < 1e-6
    inl = ~sc["outlier"]
    assert np.abs(pr.normalise(sc["k1"], sc["K1"]) - sc["q1"])[inl].max() < 1e-6
    seen = set()
    for b in range(300):
        for fx, fy, cx, cy in pr.pair_intrinsics(b):
            assert 390 <= min(fx, fy) and max(fx, fy) <= 920 and max(fx, fy) / min(fx, fy) >= 1.1
            assert 15 <= abs(cx - pr.CX) <= 45 and 15 <= abs(cy - pr.CY) <= 45
            seen.add((fx, fy, cx, cy))
    assert len(seen) == 600


@pytest.mark.parametrize("name", ["intr0", "intr1", "intr2", "planar"])
def test_restatement_finds_the_ground_truth_inliers_of_the_edge_scenes(name):
    """chosen like clean30: the restatement's winner has exactly the ground truth's inliers, under the stream index the
    GPU test estimates the scene at, and no match lies on the threshold"""
    sc = pr.edge_scene(name)
    b = pr.EDGE_SCENES[name]["pair"] if name.startswith("intr") else 0
    q0, q1 = pr.normalise(sc["k0"], sc["K0"]), pr.normalise(sc["k1"], sc["K1"])
    thr2 = pr.threshold2(sc["K0"], sc["K1"])
    truth = pr.sampson(sc["E"].ravel(), q0, q1) < thr2
    assert not pr.in_band(sc["E"], q0, q1, thr2).any()
    assert truth.sum() >= (~sc["outlier"]).sum() and 0.25 < sc["outlier"].mean() < 0.4
    # the two near-line matches: a threshold formed from either image's focal lengths alone decides one of them otherwise
    for Ka in (sc["K0"], sc["K1"]) if name != "planar" else ():
        assert not np.array_equal(pr.sampson(sc["E"].ravel(), q0, q1) < pr.threshold2(Ka, Ka), truth)
    for roots in ("numpy", "dk"):
        est = pr.estimate(sc["k0"], sc["k1"], sc["K0"], sc["K1"], seed=0, b=b, samples=256, roots=roots)
        assert est["ok"] and np.array_equal(est["mask"], truth), roots
        assert not pr.in_band(est["E"], q0, q1, thr2).any()
        assert pr.rotation_angle_deg(est["R"], sc["R"]) < 0.01 and pr.vector_angle_deg(est["t"], sc["t"]) < 0.1
    if name == "planar":
        X = np.concatenate([sc["q0"], np.ones((len(q0), 1))], 1)
        assert np.linalg.matrix_rank(np.concatenate([X / (X @ np.array(pr.PLANE))[:, None], np.ones((len(q0), 1))], 1), tol=1e-9) == 3


def test_threshold_scene_tells_the_thresholds_apart():
    sc = pr.edge_scene("thr")
    q0, q1 = pr.normalise(sc["k0"], sc["K0"]), pr.normalise(sc["k1"], sc["K1"])
    counts = []
    for thr in pr.PIXEL_THRS:
        thr2 = pr.threshold2(sc["K0"], sc["K1"], thr)
        ests = [pr.estimate(sc["k0"], sc["k1"], sc["K0"], sc["K1"], seed=0, samples=256, pixel_thr=thr, roots=r) for r in ("numpy", "dk")]
        for est in ests:
            assert est["ok"] and not pr.in_band(est["E"], q0, q1, thr2).any()
        assert np.array_equal(ests[0]["mask"], ests[1]["mask"])
        counts.append(ests[0]["inliers"])
    # of the six near-line matches one lies below 0.5 px, two more below 1 px, two more below 3 px
    assert counts[1] - counts[0] == 2 and counts[2] - counts[1] == 2, counts


@pytest.mark.parametrize("live", [(7, 298), (0,), (299,)])
def test_sparse_batches_have_a_pose_in_every_live_pair(live):
    k0, k1, bids, K0, K1, _ = pr.sparse_batch(300, live)
    assert len(k0) == 40 and K0.shape == (300, 3, 3)
    for b in live:
        rows = bids == b
        q0, q1 = pr.normalise(k0[rows], K0[b]), pr.normalise(k1[rows], K1[b])
        ests = [pr.estimate(k0[rows], k1[rows], K0[b], K1[b], seed=4, b=b, samples=64, roots=r) for r in ("numpy", "dk")]
        for est in ests:
            assert est["ok"] and est["inliers"] >= 0.7 * rows.sum()
            assert not pr.in_band(est["E"], q0, q1, pr.threshold2(K0[b], K1[b])).any()
        assert np.array_equal(ests[0]["mask"], ests[1]["mask"])


def test_degenerate_generators():
    rot = pr.pure_rotation(90, 64)
    assert not rot["t"].any() and not rot["E"].any() and not rot["T"][:3, 3].any()
    h0 = np.concatenate([rot["q0"], np.ones((64, 1))], 1) @ rot["R"].T                 # q1 is the rotated ray, nothing else
    assert np.abs(h0[:, :2] / h0[:, 2:] - rot["q1"]).max() < 1e-14
    rep = pr.repeated(91, 64)
    assert len(np.unique(rep["k0"], axis=0)) == 8 and np.array_equal(rep["k0"][:8], rep["k0"][8:16]) and len(rep["k1"]) == 64
    one = pr.repeated(91, 64, distinct=1)
    assert len(np.unique(np.hstack([one["k0"], one["k1"]]), axis=0)) == 1
    assert not pr.estimate(one["k0"], one["k1"], one["K0"], one["K1"], samples=64)["ok"]


def test_epipolar_yardsticks():
    """the float64 formula and its float32 transcription against the oracle's float32 torch restatement (which
    tests/test_oracle.py pins to the reference's fixture), in the measure the GPU tests use; the transcription's own error,
    from which their c is taken; the exact case's float64 distances, small against the bound"""
    from oracle import matcher_ref as orc
    measured = pr.transcription_measure()
    assert abs(measured - 0.6999) < 5e-4, measured           # the figure in the header of tests/test_gpu_post_edges.py
    c = 4 * measured
    for name in ("noisy", "exact"):
        case = pr.epipolar_case(name)
        d64, S, w = pr.epipolar_reference(name)
        torch32 = orc.symmetric_epipolar_errors(*(torch.as_tensor(a) for a in case)).numpy()
        assert pr.residual_measure(torch32, d64, S, w).max() <= c
        plain = pr.epipolar_rows(pr.symmetric_epipolar, *case)
        assert np.array_equal(plain, d64)
    k0, k1, bids, T, K0, K1 = pr.epipolar_case("noisy")
    assert np.bincount(bids).tolist() == [260, 300, 140] and len({K.tobytes() for K in list(K0) + list(K1)}) == 6
    d64, S, w = pr.epipolar_reference("exact")
    assert (np.sqrt(d64) <= 0.6 * pr.residual_bound(S, w, c)).all()
    assert np.isnan(pr.epipolar_reference("rotation")[0]).all()
    assert np.isnan(pr.epipolar_rows(pr.symmetric_epipolar_f32, *pr.epipolar_case("rotation"))).all()


def test_estimate_pose_needs_five_matches():
    k = np.zeros((4, 2), np.float32)
    assert post.estimate_pose(k, k, np.eye(3), np.eye(3), 0.5, conf=0.99999) is None
    assert post.estimate_pose(k[:0], k[:0], np.eye(3), np.eye(3), 0.5) is None


def test_estimate_poses_refuses_cpu_tensors():
    k = torch.zeros(8, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        post.estimate_poses(k, k, torch.zeros(8, dtype=torch.long), torch.eye(3)[None], torch.eye(3)[None])


def test_package_exports():
    import featurematching_amd as fa
    for name in ("estimate_poses", "estimate_pose", "relative_pose_error", "compute_pose_errors", "error_auc", "epidist_prec",
                 "aggregate_metrics"):
        assert getattr(fa, name) is getattr(post, name)
