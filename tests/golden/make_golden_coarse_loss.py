#!/usr/bin/env python3
"""Writes tests/golden/coarse_loss_small.npz from the REFERENCE's own Loss.compute_coarse_loss (losses/loss.py:27-67).

    python tests/golden/make_golden_coarse_loss.py PATH_TO_THE_REFERENCE_TREE

Needs no GPU.  losses/loss.py imports loguru, which only its fine loss uses: a stand-in module in sys.modules serves the
import.  Everything else executed is the reference's unmodified code, fed conf_matrix = the dual softmax of
coarse_matching_new.py:64-68 (oracle.matcher_ref.conf_matrix, pinned against the reference by tests/test_oracle.py) and
the dense conf_matrix_gt of supervision_new.py:32-33 (zeros, ones at the supervised entries).

Per case (a: (12,16)x(12,16) C 64 N 2, b: (15,17)x(11,13) C 128 N 2, both synth.coarse_descriptors(19, ..) 'borderline'
as in the dense-gradient test of test_gpu_parity.py; k0: case a with an empty supervision) and per loss (focal with
dense supervision, focal with sparse supervision, cross entropy; alpha 0.25, gamma 2, pos_weight 1, neg_weight 1):
    {case}_ids            int64 [K, 3]: every third match of the reference matcher + 20 random triples + 5 repeats
    {case}_{loss}_loss32  the reference's loss on float32 inputs (its only mode in practice)
    {case}_{loss}_loss64  ... on float64 inputs (clamp bounds are then the doubles 1e-6 and 1 - 1e-6)
    {case}_{loss}_g0/_g1  float64 autograd's gradient w.r.t. the descriptors, every 4th row, stored as float32
                          (the whole arrays would exceed the size limit of a committed fixture)
    {case}_desc_sums      float64 [2]: sums of the two descriptor arrays (synth regenerates them; this pins them)
Data only."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from featurematching_amd import synth          # noqa: E402
from oracle import matcher_ref as orc          # noqa: E402

CASES = {"a": ((12, 16), (12, 16), 64), "b": ((15, 17), (11, 13), 128), "k0": ((12, 16), (12, 16), 64)}
LOSSES = {"focal": ("focal", False), "focal_sparse": ("focal", True), "xent": ("cross_entropy", False)}
ROW_STEP = 4


def descriptors(hw0, hw1, c):
    l, s = hw0[0] * hw0[1], hw1[0] * hw1[1]
    f0, f1 = synth.coarse_descriptors(19, 2, max(l, s), c, "borderline")
    return np.ascontiguousarray(f0[:, :l]), np.ascontiguousarray(f1[:, :s])


def supervision(f0, f1, hw0, hw1, n_random=20, n_repeat=5, seed=31):
    m = orc.coarse_match(torch.as_tensor(f0), torch.as_tensor(f1), (hw0[0] * 8, hw0[1] * 8), hw0, hw1)
    ids = torch.stack([m['b_ids'][::3], m['i_ids'][::3], m['j_ids'][::3]], 1)
    g = torch.Generator().manual_seed(seed)
    rnd = torch.stack([torch.randint(f0.shape[0], (n_random,), generator=g), torch.randint(f0.shape[1], (n_random,), generator=g),
                       torch.randint(f1.shape[1], (n_random,), generator=g)], 1)
    ids = torch.cat([ids, rnd], 0)
    return torch.cat([ids, ids[:n_repeat]], 0).numpy().astype(np.int64)


def reference_loss(ref_root):
    sys.modules.setdefault("loguru", types.SimpleNamespace(logger=types.SimpleNamespace(warning=print)))
    sys.path.insert(0, ref_root)
    from losses.loss import Loss

    def make(coarse_type, sparse):
        cfg = {'module': {'loss': {'fine_correct_thr': 1.0, 'pos_weight': 1.0, 'neg_weight': 1.0, 'pose_loss_cal_flag': False,
                                   'coarse_type': coarse_type, 'focal_alpha': 0.25, 'focal_gamma': 2.0},
                          'match_coarse': {'sparse_spvs': sparse}}}
        return Loss(cfg)
    return make


def main(ref_root):
    make = reference_loss(ref_root)
    out = {}
    for case, (hw0, hw1, c) in CASES.items():
        f0, f1 = descriptors(hw0, hw1, c)
        ids = supervision(f0, f1, hw0, hw1) if case != "k0" else np.zeros((0, 3), np.int64)
        out[f"{case}_ids"] = ids
        out[f"{case}_desc_sums"] = np.array([f0.astype(np.float64).sum(), f1.astype(np.float64).sum()])
        for name, (coarse_type, sparse) in LOSSES.items():
            loss = make(coarse_type, sparse)
            for dt in (torch.float32, torch.float64):
                a0 = torch.as_tensor(f0, dtype=dt).requires_grad_(True)
                a1 = torch.as_tensor(f1, dtype=dt).requires_grad_(True)
                conf = orc.conf_matrix(a0, a1, 0.1)
                gt = torch.zeros_like(conf)                               # supervision_new.py:32-33
                gt[ids[:, 0], ids[:, 1], ids[:, 2]] = 1
                val = loss.compute_coarse_loss(conf, gt)
                if dt == torch.float32:
                    out[f"{case}_{name}_loss32"] = np.float32(val.item())
                else:
                    val.backward()
                    out[f"{case}_{name}_loss64"] = np.float64(val.item())
                    out[f"{case}_{name}_g0"] = a0.grad[:, ::ROW_STEP].numpy().astype(np.float32)
                    out[f"{case}_{name}_g1"] = a1.grad[:, ::ROW_STEP].numpy().astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "coarse_loss_small.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k, v in out.items():
        if "loss" in k:
            print(k, repr(v))


if __name__ == "__main__":
    main(sys.argv[1])
