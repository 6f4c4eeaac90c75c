#!/usr/bin/env python3
"""What the comparisons of tests/test_gpu_matcher_train.py stand on, measured (report only; the batch, the matchers and
the float64 run are tests/matcher_train_ref.py's, images 1 x 3 x 96 x 128 with 300 correspondences):

  A  the fine context layers alone, on the windows and upstream gradients of a training step, against a float64 copy -
     the float32 torch layers, hip_attention alone and all three HIP switches - with FinePreprocess's own kaiming fan-out
     draw and with the fixtures' weights (synth.merge_weights): which side of an on / off comparison is the accurate one;
  B  hip_train on against off over a whole step at both draws, and each switch on its own at the module's own draw;
  C  how far two runs of the SAME path are apart: the default backbone (convolutions) in eval mode and over a training
     step, and the patch backbone with torch's deterministic algorithms.

    python tools/probe_matcher_train.py [--out FILE]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from featurematching_amd import synth  # noqa: E402
import matcher_train_ref as mref  # noqa: E402
from timing import say, write_log  # noqa: E402

GROUPS = ("backbone", "coarse.", "fine_preprocess", "fine.", "fine_matching", "image")


def apart(ga, gb):
    """name -> max|a - b| / max|a|"""
    return {k: (ga[k].double() - gb[k].double()).abs().max().item() / ga[k].abs().max().item() for k in ga}


def largest(d, n=4):
    return " | ".join(f"{k} {d[k]:.2e}" for k in sorted(d, key=d.get)[-n:])


def per_group(d):
    return "   ".join(f"{g.rstrip('.')} {max(v for k, v in d.items() if k.startswith(g)):.1e}" for g in GROUPS)


def part_a(fixture):
    m = mref.matcher(hip_train=False, patches=True, fixture_merge=fixture)
    names, tops, errs, top_x = mref.fine_layers_against_float64(m, mref.batch(62, grad=True))
    say(f"A  fine layers against float64, {'the fixtures weights' if fixture else 'the module own draw'}: windows max|x| {top_x:.1f}")
    say(f"   {'':28s} max|ref64|   torch float32 | hip_attention | all three switches")
    for i, (name, top) in enumerate(zip(names, tops)):
        say(f"   {name:28s} {top:.3e}    {errs[0][i]:.3e} | {errs[1][i]:.3e} | {errs[2][i]:.3e}")


def part_b(fixture):
    off = mref.matcher(hip_train=False, patches=True, fixture_merge=fixture)
    weights = {k: v.clone() for k, v in off.state_dict().items()}
    loss_off, g_off = mref.step(off, mref.batch(62, grad=True))
    off.load_state_dict(weights)
    _, g_again = mref.step(off, mref.batch(62, grad=True))
    tag = "the fixtures weights" if fixture else "the module own draw"
    say(f"B  whole step, {tag}: max|g - g_off| / max|g_off|, the four largest")
    say(f"   off again           {largest(apart(g_off, g_again))}")
    variants = [("hip_train=True", None)]
    if not fixture:
        variants += [(k, k) for k in ("hip_attention", "hip_tail", "hip_proj", "hip_merge")]
    for name, switch in variants:
        m = mref.matcher(hip_train=switch is None, patches=True, fixture_merge=fixture)
        m.load_state_dict(weights)
        if switch == "hip_merge":
            m.fine_preprocess.hip_merge = True
        elif switch is not None:
            for tf in (m.coarse, m.fine):
                setattr(tf, switch, True)
                for layer in tf.layers:
                    setattr(layer, switch, True)
        loss, g = mref.step(m, mref.batch(62, grad=True))
        say(f"   {name:19s} {largest(apart(g_off, g))}   (loss {loss.item():.9e} against {loss_off.item():.9e})")


def part_c():
    torch.use_deterministic_algorithms(False)
    m = mref.matcher(hip_train=False)
    weights = {k: v.clone() for k, v in m.state_dict().items()}
    runs = []
    for _ in range(3):
        m.load_state_dict(weights)
        runs.append(mref.step(m, mref.batch(62, grad=True))[1])
    say("C  the default backbone, two training steps of the same hip_train=False matcher (same weights, same batch), largest "
        "max|g_a - g_b| / max|g_a| per part:")
    say(f"   runs 1, 2   {per_group(apart(runs[0], runs[1]))}")
    say(f"   runs 2, 3   {per_group(apart(runs[1], runs[2]))}")
    m.load_state_dict(weights)
    m.eval()
    x = torch.cat([torch.as_tensor(synth.normal(64, k, (1, 3, mref.HC * 8, mref.WC * 8)), device=mref.DEV) for k in (1, 2)])
    with torch.no_grad():
        a, b = m.backbone(x), m.backbone(x)
    say("   the same eval-mode backbone called twice: " + ", ".join(
        f"{n} map {'the same bits' if torch.equal(u, v) else f'max|diff| {(u - v).abs().max().item():.1e}'}"
        for n, u, v in zip(("coarse", "fine"), a, b)))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if not torch.cuda.is_available():
        raise SystemExit("probe_matcher_train.py measures on the GPU and found none")
    say(f"device: {torch.cuda.get_device_name(0)}")
    torch.use_deterministic_algorithms(True, warn_only=True)       # A and B: the patch backbone, torch's scatter-adds in a fixed order
    for fixture in (False, True):
        part_a(fixture)
        say()
    for fixture in (False, True):
        part_b(fixture)
        say()
    part_c()
    write_log(out)


if __name__ == "__main__":
    main()
