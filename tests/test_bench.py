"""bench.py's plain run (set-up, warm-up, ONE timed region of exactly --steps steps, the result line) and --dump-outputs:
what the last timed step computed, written as .npy files a second build's run can be compared with."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_repetitions_of_the_timed_region_need_full():
    """a plain run times exactly --steps steps: --reps (the --full spread) is refused before any GPU work"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "10", "--reps", "3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--reps" in r.stderr and "--full" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    """`bench.py --steps 40 --warmup 8 --pairs 4 --dump-outputs DIR`: one JSON line with the headline fields and none of
    --full's; DIR holds the match list and fine keypoints of the last timed step (input set (40 - 1) % 4 = 3), in
    float32 / float64, and they are the oracle's answer for that input set."""
    from featurematching_amd import synth
    from oracle import matcher_ref as orc
    from helpers import compare_match_sets
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "8",
                        "--pairs", "4", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "image-pairs/s" and out["higher_is_better"] is True and out["dtype"]
    assert out["steps"] == 40 and out["warmup"] == 8 and out["ms_per_step"] > 0
    assert abs(out["value"] - 1e3 / out["ms_per_step"]) <= 1e-2 * out["value"]     # one pair per step
    for key in ("ms_per_step_spread", "verified", "roofline", "roofline_aux", "extra", "cpu_baseline"):
        assert key not in out, key

    got = {p[:-4]: np.load(out_dir / p) for p in os.listdir(out_dir)}
    names = {"b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f"}
    assert set(got) == names
    m = got["i_ids"].shape[0]
    assert m > 1000 and all(v.shape[0] == m and v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["mkpts0_f"].shape == (m, 3) and got["mkpts0_c"].shape == (m, 2)

    wl = dict(n=1, h=480, w=640, c=256, cf=64)               # bench.WORKLOADS["cfg2"], input set 3 of rank 0
    sh = synth.config_shapes(wl)
    seed = 1000 + 17 * 3
    f0, f1 = synth.coarse_descriptors(seed, 1, sh["l"], wl["c"], "peaky")
    ff0, ff1 = synth.fine_maps(seed, 1, wl["cf"], sh["hf"], sh["wf"])
    ref = orc.match_features(f0, f1, ff0, ff1, (wl["h"], wl["w"]), synth.mix_weights(seed, 25), w=5)
    ref = {k: v.numpy() for k, v in ref.items()}
    only_g, only_r, err = compare_match_sets(got, ref)
    assert all(abs(c - 0.2) < 2e-5 for _, c in only_g + only_r) and err <= 1e-5
    gk = {(int(b), int(i), int(j)): n for n, (b, i, j) in enumerate(zip(got["b_ids"], got["i_ids"], got["j_ids"]))}
    rk = {(int(b), int(i), int(j)): n for n, (b, i, j) in enumerate(zip(ref["b_ids"], ref["i_ids"], ref["j_ids"]))}
    common = [k for k in gk if k in rk]
    gi, ri = [gk[k] for k in common], [rk[k] for k in common]
    assert len(common) > 1000
    assert np.abs(got["mkpts0_f"][gi] - ref["mkpts0_f"][ri]).max() <= 1e-3
    assert np.abs(got["mkpts1_f"][gi] - ref["mkpts1_f"][ri]).max() <= 1e-3
