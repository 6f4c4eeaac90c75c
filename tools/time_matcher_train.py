#!/usr/bin/env python3
"""One training step of the matcher - Matcher.training_step and backward() - on one 640x480 pair with 4000 seeded
correspondences, with the HIP training ops off (hip_train=False) and on, in ms by device events: the whole step, two
alternating rounds, and one more step split per stage (an event at each stage's entry and exit; the backward as one
piece).  The batch - images, correspondences - is built once, before anything is timed; every step gets a shallow copy
of the dict.  --hip-train-coarse adds a third matcher to every round: hip_train on with hip_train_coarse (the coarse
layers' tail through ops.coarse_tail).  Report only.

    python tools/time_matcher_train.py [--hip-train-coarse] [--out FILE]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from featurematching_amd import modules, synth  # noqa: E402
from featurematching_amd.matcher import Matcher  # noqa: E402
from timing import say, write_log  # noqa: E402

H, W, K = 480, 640, 4000
LOSS_CFG = {'fine_correct_thr': 1.0, 'pos_weight': 1.0, 'neg_weight': 1.0, 'pose_loss_cal_flag': False, 'coarse_type': 'focal',
            'focal_alpha': 0.25, 'focal_gamma': 2.0, 'coarse_weight': 1.0, 'fine_weight': 0.25}
CONFIG = {'module': {'loss': LOSS_CFG, 'match_coarse': {'sparse_spvs': False}}}
STAGES = ("backbone", "coarse", "coarse_matching", "fine_preprocess", "fine", "fine_matching")


def data(dev):
    img = lambda k: torch.as_tensor(synth.normal(11, k, (1, 3, H, W)), device=dev)
    pts = synth.uniform(11, 3, 2 * K).reshape(K, 2) * [W, H]
    kp0 = torch.as_tensor(pts, dtype=torch.float32, device=dev)[None]
    perm = torch.as_tensor(synth.permutation(11, 4, K), device=dev)
    return {'image0': img(1), 'image1': img(2), 'origin_kp0': kp0, 'origin_kp1': kp0[:, perm].contiguous()}


def step(m, loss, batch):
    def run():
        m.zero_grad(set_to_none=True)
        m.training_step(dict(batch), loss).backward()
    return run


def ms_of(fn, n=5):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def split(m, loss, batch):
    """one step with an event pair around every stage's forward"""
    marks, hooks = {}, []
    for name in STAGES:
        mod = getattr(m, name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        marks[name] = (e0, e1)
        hooks.append(mod.register_forward_pre_hook(lambda *_a, _e=e0: _e.record()))
        hooks.append(mod.register_forward_hook(lambda *_a, _e=e1: _e.record()))
    b0, b1, b2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    m.zero_grad(set_to_none=True)
    b0.record()
    out = m.training_step(dict(batch), loss)
    b1.record()
    out.backward()
    b2.record()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    parts = {name: e0.elapsed_time(e1) for name, (e0, e1) in marks.items()}
    parts["supervision, loss, between the stages"] = b0.elapsed_time(b1) - sum(parts.values())
    parts["backward"] = b1.elapsed_time(b2)
    return parts


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not torch.cuda.is_available():
        raise SystemExit("time_matcher_train.py measures on the GPU and found none")
    dev = torch.device("cuda:0")
    say(f"device: {torch.cuda.get_device_name(0)}   one training_step + backward, {W}x{H}, {K} correspondences, ms")
    loss = modules.Loss(CONFIG).train()
    batch = data(dev)                                  # built once, outside every timed region
    torch.cuda.synchronize()
    kinds = {"off": dict(hip_train=False), "on ": dict(hip_train=True)}
    if "--hip-train-coarse" in sys.argv:
        kinds["on, hip_train_coarse"] = dict(hip_train=True, hip_train_coarse=True)
    ms, runs = {}, {}
    for kind, kw in kinds.items():
        torch.manual_seed(3)
        runs[kind] = step(Matcher(**kw).to(dev).train(), loss, batch)
        runs[kind](); runs[kind]()
        ms[kind] = []
    for _ in range(2):
        for kind in kinds:
            ms[kind].append(ms_of(runs[kind]))
    for kind in kinds:
        say(f"hip_train {kind}  whole step {ms[kind][0]:8.2f} / {ms[kind][1]:8.2f} ms (round 1 / round 2)")
    for kind, kw in kinds.items():
        torch.manual_seed(3)
        m = Matcher(**kw).to(dev).train()
        step(m, loss, batch)()
        parts = split(m, loss, batch)
        say(f"hip_train {kind}  " + "   ".join(f"{k} {v:.2f}" for k, v in parts.items()))
    write_log(out)


if __name__ == "__main__":
    main()
