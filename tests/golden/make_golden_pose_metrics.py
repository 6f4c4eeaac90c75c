#!/usr/bin/env python3
"""Writes tests/golden/pose_metrics.npz from the REFERENCE's own utils/metrics.py (:12-29 relative_pose_error, :162-182
error_auc, :185-196 epidist_prec, :199-219 aggregate_metrics).

    python tests/golden/make_golden_pose_metrics.py PATH_TO_THE_REFERENCE_TREE

Needs no GPU.  utils/metrics.py imports cv2, loguru and kornia, which the four functions do not use (loguru: one log line):
stand-in modules in sys.modules serve the imports.  Everything executed is the reference's unmodified code.

    T [P, 4, 4], R [P, 3, 3], t [P, 3]      seeded poses and estimates (synth's hashes)
    t_err, R_err [P]                         relative_pose_error(T[p], R[p], t[p])
    auc_in_{k} / auc_{k} [3]                 error lists (empty tail, all large, ties, values on a threshold) -> auc@5/10/20
    epi_{k}_{j}, prec_thr, prec_{k} [2]      ragged lists of epipolar errors (an empty pair included) -> precisions
    agg_R, agg_t, agg_ids, agg_epi_{j}, agg_out [4]   a metrics dict with repeated identifiers -> auc@5/10/20, prec@5e-04
Data only."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from featurematching_amd import synth          # noqa: E402


def reference_metrics(ref_root):
    log = types.SimpleNamespace(info=lambda *a, **k: None, warning=print)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.modules.setdefault("loguru", types.SimpleNamespace(logger=log))
    kornia = types.ModuleType("kornia")
    for name in ("kornia.geometry", "kornia.geometry.epipolar", "kornia.geometry.conversions"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules.setdefault("kornia", kornia)
    sys.modules["kornia.geometry.epipolar"].numeric = None
    sys.modules["kornia.geometry.conversions"].convert_points_to_homogeneous = None
    sys.path.insert(0, ref_root)
    from utils import metrics
    return metrics


def rot(w):
    th = np.linalg.norm(w)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def main(ref_root):
    m = reference_metrics(ref_root)
    out = {}
    P = 12
    u = synth.uniform(91, 1, P * 12).reshape(P, 12)
    T = np.tile(np.eye(4), (P, 1, 1))
    R = np.zeros((P, 3, 3))
    t = np.zeros((P, 3))
    for p in range(P):
        T[p, :3, :3] = rot(0.4 * (2 * u[p, :3] - 1))
        T[p, :3, 3] = 2 * u[p, 3:6] - 1
        R[p] = T[p, :3, :3] @ rot((0.001 if p < 3 else 0.3) * (2 * u[p, 6:9] - 1))
        t[p] = T[p, :3, 3] + (0.0 if p == 0 else 0.2) * (2 * u[p, 9:12] - 1)
    R[1] = T[1, :3, :3]                                  # the clip: cos just above 1
    errs = [m.relative_pose_error(T[p], R[p], t[p], ignore_gt_t_thr=0.0) for p in range(P)]
    out.update(T=T, R=R, t=t, t_err=np.array([e[0] for e in errs]), R_err=np.array([e[1] for e in errs]))
    v = synth.uniform(92, 1, 40) * 30
    lists = {"a": v, "b": v[:1], "c": np.array([25.0, 31.0, np.inf]), "d": np.array([5.0, 5.0, 10.0, 20.0, 0.0, 3.0]),
             "e": np.array([1.0, np.inf, 2.0, np.inf, 7.5])}
    for k, e in lists.items():
        out[f"auc_in_{k}"] = e
        out[f"auc_{k}"] = np.array(m.error_auc(list(e), [1, 2, 3], ret_dict=False), np.float64)
    w = synth.uniform(93, 1, 60) * 1e-3
    ragged = {"a": [w[:20], w[20:21], np.zeros(0), w[21:60]], "b": [np.zeros(0)], "c": [w[:5] * 0, w[5:9] + 1]}
    out["prec_thr"] = np.array([1e-4, 5e-4])
    for k, ls in ragged.items():
        for j, e in enumerate(ls):
            out[f"epi_{k}_{j}"] = e
        out[f"prec_{k}"] = np.array(m.epidist_prec(np.array(ls, dtype=object), list(out["prec_thr"]), ret_dict=False), np.float64)
    ids = np.array([3, 1, 3, 2, 1, 7, 8, 3])
    agg_R = np.array([1.0, 4.0, 12.0, 30.0, 2.0, np.inf, 0.5, 6.0])
    agg_t = np.array([0.5, 6.0, 1.0, 2.0, 3.0, np.inf, 0.7, 0.1])
    epi = [w[3 * i:3 * i + (i % 4)] for i in range(8)]
    res = m.aggregate_metrics({"identifiers": [f"pair{i}" for i in ids], "R_errs": list(agg_R), "t_errs": list(agg_t),
                               "epi_errs": epi}, epi_err_thr=5e-4)
    out.update(agg_ids=ids, agg_R=agg_R, agg_t=agg_t)
    for j, e in enumerate(epi):
        out[f"agg_epi_{j}"] = e
    assert list(res) == ["auc@5", "auc@10", "auc@20", "prec@5e-04"], list(res)
    out["agg_out"] = np.array(list(res.values()), np.float64)
    path = os.path.join(ROOT, "tests", "golden", "pose_metrics.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in ("t_err", "R_err", "auc_a", "auc_c", "prec_a", "agg_out"):
        print(k, out[k])


if __name__ == "__main__":
    main(sys.argv[1])
