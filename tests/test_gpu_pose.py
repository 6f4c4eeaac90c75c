"""The device pose estimate (csrc/pose.hip, post.estimate_poses) against the float64 NumPy restatement tests/pose_ref.py:
the solver alone, segment and tile edges, exact bookkeeping, noise-free and noisy scenes, determinism, the drop-in."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pose_ref as pr
from pose_ref import check_bookkeeping, same_bits
from featurematching_amd import _lib, post

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.as_tensor(x, device=DEV)


def call(k0, k1, bids, K0, K1, **kw):
    out = post.estimate_poses(dev(k0), dev(k1), dev(bids), dev(K0), dev(K1), **kw)
    return {k: getattr(out, k).cpu().numpy() for k in out._fields}


@functools.lru_cache(maxsize=None)
def scene(name=None, **kw):
    return pr.scene(**(pr.SCENES[name] if name else kw))


@functools.lru_cache(maxsize=None)
def reference(name, seed, samples, b=0):
    sc = scene(name)
    return pr.estimate(sc["k0"], sc["k1"], sc["K"], sc["K"], seed=seed, b=b, samples=samples)


# ---- the solver alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", pr.SOLVER_SEEDS)
def test_solver_alone(seed):
    S = 200
    q0, q1, E_true = pr.exact_samples(seed, S)
    E = torch.zeros(S, 10, 9, dtype=torch.float64, device=DEV)
    count = torch.full((S,), -1, dtype=torch.int32, device=DEV)
    a, b = dev(q0).contiguous(), dev(q1).contiguous()
    p = lambda x: C.c_void_p(x.data_ptr())
    st = _lib.load().fm_debug_pose_solve(p(a), p(b), S, p(E), p(count), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    E, count = E.cpu().numpy(), count.cpu().numpy()
    assert count.min() >= 0 and count.max() <= 10
    live = np.arange(10)[None] < count[:, None]
    E3 = E.reshape(S, 10, 3, 3)
    Et = np.swapaxes(E3, 2, 3)
    assert np.abs(np.linalg.norm(E, axis=2)[live] - 1).max() <= 1e-12
    h0, h1 = np.concatenate([q0, np.ones((S, 5, 1))], 2), np.concatenate([q1, np.ones((S, 5, 1))], 2)
    epi = np.abs(np.einsum("hpi,hcij,hpj->hcp", h1, E3, h0)).max(2)
    cubic = np.linalg.norm(2 * E3 @ Et @ E3 - np.trace(E3 @ Et, axis1=2, axis2=3)[..., None, None] * E3, axis=(2, 3))
    print(f"seed {seed}: {int(count.sum())} candidates, largest |q1 E q0| {epi[live].max():.2e}, largest cubic residual {cubic[live].max():.2e}")
    assert epi[live].max() <= 1e-9 and cubic[live].max() <= 1e-9
    Er, cr = pr.solve5(q0, q1, "numpy")
    ref_found, found = pr.found_true(Er, cr, E_true), pr.found_true(E, count, E_true)
    print(f"  true E found: restatement {int(ref_found.sum())}, kernel {int(found.sum())}, kernel misses of the restatement's "
          f"{int((ref_found & ~found).sum())}")
    assert ref_found.sum() >= 0.98 * S
    assert (ref_found & ~found).sum() <= 0.03 * ref_found.sum()
    z = np.where(live, E[:, :, 7] / np.where(live, E[:, :, 8], 1.0), 0.0)                 # z = E21 / E22
    assert np.all(np.diff(z, axis=1)[live[:, 1:]] >= 0)


# ---- segment and tile edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m_b", [0, 4, 5, 6, 63, 64, 65, 300])
def test_one_pair_of_every_size(m_b):
    sc = pr.scene(seed=30 + m_b, n=max(m_b, 1), outliers=0.2)
    k0, k1, bids, K0, K1, _ = pr.batch([dict(sc, k0=sc["k0"][:m_b], k1=sc["k1"][:m_b])])
    for samples in (1, 63, 64, 65, 256):
        out = call(k0, k1, bids, K0, K1, samples=samples, seed=3)
        check_bookkeeping(out, k0, k1, bids, K0, K1)
        ref = pr.estimate(k0, k1, K0[0], K1[0], seed=3, samples=samples)
        assert bool(out["ok"][0]) == ref["ok"], samples
        assert int(out["per_pair"][0, 1]) == ref["inliers"] and int(out["per_pair"][0, 2]) == ref["votes"], samples
        if m_b >= 64 and samples >= 63:
            assert ref["ok"]


@functools.lru_cache(maxsize=None)
def four_pairs():
    sizes = (37, 0, 130, 4)
    scenes = []
    for b, m in enumerate(sizes):
        sc = pr.scene(seed=50 + b, n=max(m, 1), outliers=0.25)
        scenes.append(dict(sc, k0=sc["k0"][:m], k1=sc["k1"][:m]))
    return pr.batch(scenes)


def test_four_pairs_of_different_sizes():
    k0, k1, bids, K0, K1, _ = four_pairs()
    out = call(k0, k1, bids, K0, K1, samples=65, seed=1)
    check_bookkeeping(out, k0, k1, bids, K0, K1)
    assert list(out["ok"]) == [True, False, True, False]
    for b in (0, 2):                                         # a pair of a batch is the pair alone, with its own stream of draws
        ref = pr.estimate(k0[bids == b], k1[bids == b], K0[b], K1[b], seed=1, b=b, samples=65)
        assert int(out["per_pair"][b, 1]) == ref["inliers"] and int(out["per_pair"][b, 2]) == ref["votes"]
        assert min(np.abs(out["E"][b].ravel() - ref["E"]).max(), np.abs(out["E"][b].ravel() + ref["E"]).max()) <= 1e-9


def test_keypoint_stride_count_and_foreign_ids():
    k0, k1, bids, K0, K1, _ = four_pairs()
    base = call(k0, k1, bids, K0, K1, samples=64, seed=2)
    # [M, 3] keypoints (mkpts*_f): the third column is not looked at
    junk = np.full((len(k0), 1), 7.5, np.float32)
    assert same_bits(call(np.hstack([k0, junk]), np.hstack([k1, junk]), bids, K0, K1, samples=64, seed=2), base)
    # a count shorter than the tensors: the rows behind it do not exist
    cut = len(k0) - 12
    short = call(k0, k1, bids, K0, K1, samples=64, seed=2, count=torch.tensor([cut], dtype=torch.int32, device=DEV))
    alone = call(k0[:cut], k1[:cut], bids[:cut], K0, K1, samples=64, seed=2)
    assert not short["inliers"][cut:].any()
    short["inliers"] = short["inliers"][:cut]
    assert same_bits(short, alone)
    check_bookkeeping(alone, k0[:cut], k1[:cut], bids[:cut], K0, K1)
    # ids outside [0, N) belong to no pair
    pad = np.tile(k0[:3], (1, 1))
    wide = call(np.vstack([pad, k0, pad]), np.vstack([pad, k1, pad]), np.concatenate([[-2, -1, -1], bids, [4, 4, 9]]), K0, K1,
                samples=64, seed=2)
    assert not wide["inliers"][:3].any() and not wide["inliers"][-3:].any()
    wide["inliers"] = wide["inliers"][3:-3]
    assert same_bits(wide, base)


def test_unsorted_list_with_a_count():
    """the rows behind the count do not exist, wherever a sort would put them; an int64 count is converted"""
    k0, k1, bids, K0, K1, _ = four_pairs()
    perm = np.argsort(pr.synth.hash_u64(9, 2, len(bids)), kind="stable")
    s0, s1, sb = k0[perm], k1[perm], bids[perm]
    cut = len(sb) - 20
    assert (sb[cut:] < sb[:cut].max()).any()                 # a plain sort of all rows would pull some of them forward
    out = call(s0, s1, sb, K0, K1, samples=64, seed=2, sorted_bids=False, count=torch.tensor([cut], dtype=torch.int64))
    order = np.argsort(sb[:cut], kind="stable")
    ref = call(s0[:cut][order], s1[:cut][order], sb[:cut][order], K0, K1, samples=64, seed=2)
    assert not out["inliers"][cut:].any()
    assert np.array_equal(out["inliers"][:cut][order], ref["inliers"])
    out["inliers"] = ref["inliers"]
    assert same_bits(out, ref)


def test_unsorted_list():
    k0, k1, bids, K0, K1, _ = four_pairs()
    perm = np.argsort(pr.synth.hash_u64(9, 1, len(bids)), kind="stable")
    s0, s1, sb = k0[perm], k1[perm], bids[perm]
    assert (np.diff(sb) < 0).any()
    out = call(s0, s1, sb, K0, K1, samples=64, seed=2, sorted_bids=False)
    order = np.argsort(sb, kind="stable")
    ref = call(s0[order], s1[order], sb[order], K0, K1, samples=64, seed=2)
    assert np.array_equal(out["inliers"][order], ref["inliers"])
    out["inliers"] = ref["inliers"]
    assert same_bits(out, ref)
    check_bookkeeping(ref, s0[order], s1[order], sb[order], K0, K1)


# ---- scenes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.NOISE_FREE)
def test_noise_free_scene(name):
    sc = scene(name)
    k0, k1, bids, K0, K1, _ = pr.batch([sc])
    out = call(k0, k1, bids, K0, K1, samples=256, seed=0)
    check_bookkeeping(out, k0, k1, bids, K0, K1)
    assert out["ok"][0]
    q0, q1 = pr.normalise(k0, K0[0]), pr.normalise(k1, K1[0])
    thr2 = pr.threshold2(K0[0], K1[0])
    truth = pr.sampson(sc["E"].ravel(), q0, q1) < thr2
    assert not pr.in_band(sc["E"], q0, q1, thr2).any()
    assert np.array_equal(out["inliers"], truth)
    assert truth.sum() >= (~sc["outlier"]).sum()
    ref = reference(name, 0, 256)
    assert np.array_equal(ref["mask"], truth)
    # the same samples, the same tie rules: the same candidate, to the rounding of two root finders
    r_err, t_ang = pr.rotation_angle_deg(out["R"][0], sc["R"]), pr.vector_angle_deg(out["t"][0], sc["t"])
    r_ref, t_ref = pr.rotation_angle_deg(ref["R"], sc["R"]), pr.vector_angle_deg(ref["t"], sc["t"])
    print(f"{name}: R_err {r_err:.3e} (restatement {r_ref:.3e}), t angle {t_ang:.3e} ({t_ref:.3e}) degrees")
    assert min(np.abs(out["E"][0].ravel() - ref["E"]).max(), np.abs(out["E"][0].ravel() + ref["E"]).max()) <= 1e-9
    assert abs(r_err - r_ref) <= 1e-6 and abs(t_ang - t_ref) <= 1e-6
    # against the ground truth itself (float32 keypoints: the restatement's own error is 1e-4 degrees at most here)
    assert r_err < 0.01 and t_ang < 0.1
    if name in pr.BACKWARD:              # a baseline towards -x: the pose is a -t decomposition, and that one
        Rd, td = pr.decompose(out["E"][0])[pr.BACKWARD[name]]
        assert np.abs(Rd - out["R"][0]).max() <= 1e-12 and np.abs(td - out["t"][0]).max() <= 1e-12


# per scene: what the restatement's own results spread over eight seeds (tools/pose_accuracy.py, profiles/pose_accuracy.txt):
# inliers, rotation error and translation angle in degrees
ALLOW = {"noisy64": (5, 0.3371, 2.4675), "noisy300": (10, 0.5009, 1.6504)}


@pytest.mark.parametrize("name", ["noisy64", "noisy300"])
def test_noisy_scene(name):
    sc = scene(name)
    k0, k1, bids, K0, K1, _ = pr.batch([sc])
    short, floor_r, floor_t = ALLOW[name]
    for seed in (0, 1):
        out = call(k0, k1, bids, K0, K1, samples=256, seed=seed)
        check_bookkeeping(out, k0, k1, bids, K0, K1)
        ref = reference(name, seed, 256)
        assert out["ok"][0] and ref["ok"]
        r_err, t_ang = pr.rotation_angle_deg(out["R"][0], sc["R"]), pr.vector_angle_deg(out["t"][0], sc["t"])
        r_ref, t_ref = pr.rotation_angle_deg(ref["R"], sc["R"]), pr.vector_angle_deg(ref["t"], sc["t"])
        same = min(np.abs(out["E"][0].ravel() - ref["E"]).max(), np.abs(out["E"][0].ravel() + ref["E"]).max())
        print(f"{name} seed {seed}: inliers {int(out['per_pair'][0, 1])} (restatement {ref['inliers']}), R_err {r_err:.4f} ({r_ref:.4f}), "
              f"t angle {t_ang:.4f} ({t_ref:.4f}), max |E - E_ref| {same:.2e}")
        assert int(out["per_pair"][0, 1]) >= ref["inliers"] - short
        assert r_err <= 2 * r_ref + floor_r and t_ang <= 2 * t_ref + floor_t


# ---- determinism, the drop-in -----------------------------------------------------------------------------------------------
def test_same_bits_every_time():
    k0, k1, bids, K0, K1, T = four_pairs()
    first = call(k0, k1, bids, K0, K1, samples=128, seed=5)
    assert same_bits(call(k0, k1, bids, K0, K1, samples=128, seed=5), first)
    post.epipolar_errors(dev(k0), dev(k1), dev(bids), dev(T.astype(np.float32)), dev(K0), dev(K1))      # an unrelated call
    sc = scene("noisy64")
    call(*pr.batch([sc])[:5], samples=64, seed=1)                                                       # ... and another shape
    assert same_bits(call(k0, k1, bids, K0, K1, samples=128, seed=5), first)
    assert not same_bits(call(k0, k1, bids, K0, K1, samples=128, seed=6), first)


def test_compute_pose_errors_is_the_drop_in():
    scenes = [scene("clean30"), dict(scene("clean"), k0=scene("clean")["k0"][:3], k1=scene("clean")["k1"][:3]), scene("clean60")]
    k0, k1, bids, K0, K1, T = pr.batch(scenes)
    junk = np.zeros((len(k0), 1), np.float32)
    data = {"m_bids": dev(bids), "mkpts0_f": dev(np.hstack([k0, junk])), "mkpts1_f": dev(np.hstack([k1, junk])), "K0": dev(K0),
            "K1": dev(K1), "T_0to1": dev(T.astype(np.float32))}
    post.compute_pose_errors(data, samples=256, seed=0)
    assert len(data["R_errs"]) == len(data["t_errs"]) == len(data["inliers"]) == 3
    T32 = T.astype(np.float32)
    for b, sc in enumerate(scenes):
        ref = pr.estimate(sc["k0"], sc["k1"], sc["K"], sc["K"], seed=0, b=b, samples=256)
        if not ref["ok"]:
            assert b == 1 and data["R_errs"][b] == np.inf and data["t_errs"][b] == np.inf and len(data["inliers"][b]) == 0
            continue
        t_err, R_err = post.relative_pose_error(T32[b], ref["R"], ref["t"])
        # the same candidate (1e-9 apart at most): angles within 1e-6 degrees, distances within 1e-8
        assert abs(data["R_errs"][b] - R_err) <= 1e-6 and abs(data["t_errs"][b] - t_err) <= 1e-8, b
        assert np.array_equal(data["inliers"][b], ref["mask"])
    # one pair through the reference's positional signature
    sc = scenes[0]
    R, t, mask = post.estimate_pose(sc["k0"], sc["k1"], sc["K"], sc["K"], 0.5, 0.99999, samples=256, seed=0)
    ref = pr.estimate(sc["k0"], sc["k1"], sc["K"], sc["K"], seed=0, b=0, samples=256)
    assert np.abs(R - ref["R"]).max() <= 1e-8 and np.abs(t - ref["t"]).max() <= 1e-8 and np.array_equal(mask, ref["mask"])
    assert post.estimate_pose(dev(sc["k0"][:4]), dev(sc["k1"][:4]), sc["K"], sc["K"], 0.5) is None
