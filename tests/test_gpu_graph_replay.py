"""A replayed step is a function of its input buffers.

bench.py's timed step runs as a captured graph, replayed hundreds of times into the same workspace, on non-default
streams, with window and scratch buffers shared between the input sets of a stream.  include/fmatch.h promises what makes
that legal: the library keeps no state and asks nothing of a workspace's contents.  Here the small step of
tests/step_cases.py is captured on a side stream (one stream per capture, no fork inside it: the graph has no parallel
branch) after one eager warm-up step on that stream, and replayed over a schedule of input sets that are copied into the
static inputs on the same stream before each replay - the match count goes up, down and to zero.  After every replay the
outputs and `count` are cloned on the stream; the host waits once, at the end.  EVERY replay's clone must
  * equal, bit for bit over its first M rows, an eager step on fresh buffers with that input set, and
  * meet the oracle bars of step_cases.oracle_errors (ids and coarse keypoints equal, conf within 1e-5, fine keypoints
    within 1e-3 px).
The mode of a graph is the one the auto entry point learns on the graph's first input set (step_cases.learnt_mode), or
step_cases.GENERAL for the graphs that mix distributions and hold the empty set; before the capture every input set of
the schedule must be served by an eager call in that mode.

Each replay prints one RPL line (`pytest -s`); profiles/replay_tests_record.txt holds the lines of one run.
"""
import functools

import numpy as np
import pytest
import torch

import ctx_layers_ref as cr
import step_cases as sc
from featurematching_amd import _lib, ops, post

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PEAKY4 = [("peaky", s) for s in (7001, 7002, 7003, 7004, 7001, 7001)]
CASES = {
    "headline": dict(n=1, c=256, w=5, route="maps_fused", mode="learnt", sched=PEAKY4, m=(49, 44, 50, 45, 49, 49)),
    "windows": dict(n=1, c=64, w=7, route="windows", mode="learnt", sched=PEAKY4, m=(49, 44, 50, 45, 49, 49)),
    "nhwc": dict(n=2, c=64, w=5, route="maps_nhwc", mode="learnt",
                 sched=[("borderline", 7001), ("borderline", 7003), ("borderline", 7001)], m=(87, 94, 87)),
    "any_data": dict(n=1, c=64, w=5, route="maps_fused", mode="general",
                     sched=[("peaky", 7001), ("mixed", 7003), ("empty", 7001), ("borderline", 7002), ("empty", 7001),
                            ("peaky", 7001)], m=(49, 34, 0, 40, 0, 49)),
    "any_data_batch": dict(n=2, c=256, w=7, route="windows", mode="general",
                           sched=[("mixed", 7001), ("empty", 7001), ("peaky", 7003)], m=(73, 0, 95)),
    "stats": dict(n=2, c=64, w=5, route="coarse_stats", mode="learnt",
                  sched=[("borderline", 7001), ("borderline", 7003), ("borderline", 7001)], m=(87, 94, 87)),
}


def _set(cs, which):
    return sc.input_set(which[0], which[1], cs['n'], cs['c'], cs['w'])


def _enqueue(d, route, mode, bufs):
    if route == "coarse_stats":
        return sc.coarse(d, mode, stats=True)
    return sc.step(d, route, mode, bufs)


def _stat_slices(buf, ws):
    """the row and column statistics (stabilisers, denominators: four [N, L] float32 arrays) of a stats=True coarse call,
    read out of `ws` (the call's workspace or a clone of it) as tests/test_gpu_coarse_edges.py reads them"""
    nr, sr, qr, nc, sc_, qc = buf.softmax_stats()
    n, l, s = buf._shape[:3]
    assert qr >= l and qc >= s

    def read(p, pitch, k):
        o = p.value - buf.workspace.data_ptr()
        return ws[o:o + n * pitch * 4].view(torch.float32).view(n, pitch)[:, :k].cpu().numpy()
    return dict(nm_r=read(nr, qr, l), sum_r=read(sr, qr, l), nm_c=read(nc, qc, s), sum_c=read(sc_, qc, s))


_EAGER = {}


def _eager(cs, which, mode):
    """(M, numpy outputs) of one eager step on fresh buffers on the default stream; computed once per (set, route, mode).
    read_count raises when the mode does not serve the set: the schedule must then take another seed."""
    key = (which, cs['n'], cs['c'], cs['w'], cs['route'], tuple(sorted(mode.items(), key=str)))
    if key not in _EAGER:
        s = _set(cs, which)
        d = sc.to_device(s, cs['route'], DEV)
        res = _enqueue(d, cs['route'], mode, sc.Bufs(cs['n'], cs['w'], DEV))
        buf = res[0] if isinstance(res, tuple) else res
        m = buf.read_count()                     # raises on a status: the set is not served by this mode
        torch.cuda.synchronize()
        out = sc.host(sc.outputs(res))
        if cs['route'] == "coarse_stats":
            out.update(_stat_slices(buf, buf.workspace))
        _EAGER[key] = (m, out)
    return _EAGER[key]


def _mode_of(cs):
    if cs['mode'] == "general":
        return dict(sc.GENERAL)
    d = sc.to_device(_set(cs, cs['sched'][0]), cs['route'], DEV)
    return sc.learnt_mode(d, stats=cs['route'] == "coarse_stats")


class Replayed:
    """one captured step: static inputs, the graph, its result tensors; `replay(which)` loads an input set, replays and
    clones on the current stream"""

    def __init__(self, name, cs, side, bufs=None, behind=None):
        self.name, self.cs, self.side = name, cs, side
        self.mode = _mode_of(cs)
        for which in dict.fromkeys(cs['sched']):             # served by an eager call in that mode, before the capture
            _eager(cs, which, self.mode)
        self.sets = {which: sc.to_device(_set(cs, which), cs['route'], DEV) for which in dict.fromkeys(cs['sched'])}
        self.static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.sets[cs['sched'][0]].items()}
        self.bufs = bufs or sc.Bufs(cs['n'], cs['w'], DEV)
        self.behind = behind
        torch.cuda.synchronize()
        with torch.cuda.stream(side):                        # the kernels' dynamic-LDS attributes are set at a first launch
            self._enqueue()
        side.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.res, self.extra = self._enqueue()
        self.clones = []

    def _enqueue(self):
        res = _enqueue(self.static, self.cs['route'], self.mode, self.bufs)
        return res, (self.behind(res) if self.behind else None)

    def replay(self, which):
        sc.load(self.static, self.sets[which])
        self.graph.replay()
        cl = sc.clones(self.res)
        if self.cs['route'] == "coarse_stats":
            cl['workspace'] = self.res.workspace.clone()
        if self.extra is not None:
            cl['extra'] = [t.clone() for t in self.extra]
        self.clones.append((which, cl))

    def check(self):
        """every replay against the eager step and the oracle; returns the failures"""
        failures = []
        for k, (which, cl) in enumerate(self.clones):
            tag = f"{self.name} replay {k} {which[0]}{which[1]}"
            m_e, eager = _eager(self.cs, which, self.mode)
            extra, ws = cl.pop('extra', None), cl.pop('workspace', None)
            got = sc.host(cl)
            m, status = int(got['count'][0]), int(got['count'][1])
            if ws is not None:
                got.update(_stat_slices(self.res, ws))
            bad = []
            if status & ~_lib.FM_DEV_ALL_DENSE:
                bad.append(f"status word {status:#x}")
            if m != m_e or not np.array_equal(got['count'], eager['count']):
                bad.append(f"count {got['count'].tolist()}, eager {eager['count'].tolist()}")
            else:
                rows = [k for k in eager if k not in ("count", "nm_r", "sum_r", "nm_c", "sum_c")]
                bad += [f"{k}: bits differ from the eager step" for k in sc.bit_errors(got, eager, m, rows)]
                bad += [f"{k}: bits differ from the eager call" for k in ("nm_r", "sum_r", "nm_c", "sum_c")
                        if k in eager and sc.bit_errors(got, eager, None, [k])]
            bad += sc.oracle_errors(got, m, sc.oracle_of(_set(self.cs, which)))
            print(f"RPL {tag:44s} M {m:3d}  {'= eager bits, oracle bars hold' if not bad else 'FAILED: ' + '; '.join(bad)}")
            failures += [f"{tag}: {b}" for b in bad]
            cl['extra'] = extra
        return failures


@pytest.mark.parametrize("name", list(CASES))
def test_replay_over_a_schedule(name):
    cs = CASES[name]
    side = torch.cuda.Stream(DEV)
    g = Replayed(name, cs, side)
    with torch.cuda.stream(side):
        for which in cs['sched']:
            g.replay(which)
    side.synchronize()
    failures = g.check()
    ms = tuple(int(cl['count'][0]) for _, cl in g.clones)
    assert not failures, "\n".join(failures)
    assert ms == cs['m'], (ms, cs['m'])                  # the counts the schedule was written for (tests/test_step_cases.py)


SHARED = {
    "A": dict(n=1, c=64, w=7, route="windows", mode="learnt", sched=[("peaky", 7001)]),
    "B": dict(n=1, c=256, w=5, route="maps_fused", mode="learnt", sched=[("peaky", 7003)]),
    "C": dict(n=1, c=64, w=5, route="windows", mode="learnt", sched=[("borderline", 7002)]),
    "D": dict(n=1, c=64, w=7, route="maps_fused", mode="learnt", sched=[("peaky", 7004)]),
}


def test_two_graphs_share_window_and_scratch_buffers():
    """two input sets of one stream share win0 / win1 / scratch (bench.Pair(share=...)): the `windows` and the
    `maps_fused` route, captured into the same buffers and replayed A B A B B A"""
    side = torch.cuda.Stream(DEV)
    bufs = sc.Bufs(1, 7, DEV)
    gs = {k: Replayed(f"shared {k}", SHARED[k], side, bufs=bufs) for k in "AB"}
    with torch.cuda.stream(side):
        for k in "ABABBA":
            gs[k].replay(SHARED[k]['sched'][0])
    side.synchronize()
    failures = gs['A'].check() + gs['B'].check()
    assert not failures, "\n".join(failures)


def test_streams_side_by_side():
    """four graphs on two streams, two per stream sharing that stream's buffers, 24 rounds interleaved across the streams;
    the host waits only at the end and every replay is checked"""
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    bufs = [sc.Bufs(1, 7, DEV), sc.Bufs(1, 7, DEV)]
    gs = [Replayed(f"streams {k}", SHARED[k], streams[i // 2], bufs=bufs[i // 2]) for i, k in enumerate("ABCD")]
    torch.cuda.synchronize()
    for _ in range(24):
        for i in (0, 2, 1, 3):                               # stream 0, stream 1, stream 0, stream 1
            with torch.cuda.stream(gs[i].side):
                gs[i].replay(gs[i].cs['sched'][0])
    torch.cuda.synchronize()
    failures = [f for g in gs for f in g.check()]
    assert all(len(g.clones) == 24 for g in gs)
    assert not failures, "\n".join(failures)


POSE = dict(n=2, c=64, w=5, route="windows", mode="general", sched=[("peaky", 7001), ("peaky", 7003), ("empty", 7001)],
            m=(93, 95, 0))


@functools.lru_cache(maxsize=None)
def _pose_k():
    return torch.tensor([[100.0, 0.0, 64.0], [0.0, 100.0, 48.0], [0.0, 0.0, 1.0]]).repeat(2, 1, 1).to(DEV)


def _pose_behind(res):
    """post.estimate_poses on the step's device-side list: documented as not synchronising"""
    p = post.estimate_poses(res[1], res[2], res[0].b_ids, _pose_k(), _pose_k(), samples=256, count=res[0].count)
    return [p.R, p.t, p.E, p.inliers, p.per_pair]


def test_pose_behind_the_step():
    """estimate_poses(count=buf.count) captured behind the `windows` step: R, t, E, the inlier flags and per_pair of
    every replay equal the eager call's bits; the empty set leaves no pose and no inlier"""
    _pose_k()                                                # on the device before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    g = Replayed("pose", POSE, side, behind=_pose_behind)
    with torch.cuda.stream(side):
        for which in POSE['sched']:
            g.replay(which)
    side.synchronize()
    failures = g.check()
    for k, (which, cl) in enumerate(g.clones):
        d = sc.to_device(_set(POSE, which), "windows", DEV)
        res = sc.step(d, "windows", g.mode, sc.Bufs(2, 5, DEV))
        want = _pose_behind(res)
        torch.cuda.synchronize()
        m = int(cl['count'][0].item())
        names = ("R", "t", "E", "inliers", "per_pair")
        bad = [nm for nm, a, b in zip(names, cl['extra'], want)
               if not np.array_equal((a[:m] if nm == "inliers" else a).cpu().numpy().view(np.uint8),
                                     (b[:m] if nm == "inliers" else b).cpu().numpy().view(np.uint8))]
        per = cl['extra'][4].cpu().numpy()
        if m == 0 and (per[:, :3].any() or cl['extra'][3].any().item()):
            bad.append(f"empty set: per_pair {per.tolist()}")
        print(f"RPL pose replay {k} {which[0]}{which[1]:<30d} M {m:3d}  per_pair {per.tolist()}  "
              f"{'= eager bits' if not bad else 'FAILED: ' + ', '.join(bad)}")
        failures += [f"pose replay {k} {which}: {b} differs from the eager call" for b in bad]
    assert not failures, "\n".join(failures)
    assert tuple(int(cl['count'][0]) for _, cl in g.clones) == POSE['m']


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint8)


def test_coarse_context_layers_replayed():
    """ops.coarse_transformer at (2, 77, 45), four layers (its workspace is allocated inside the capture and replayed
    into): every replay's outputs equal the eager call's bits, also after the inputs changed in place"""
    w = cr.coarse_weights(4)
    packed = ops.pack_coarse_transformer({k: torch.as_tensor(v) for k, v in w.items()}, 4, DEV)
    sets = [cr.coarse_inputs(2, 77, 45), cr.coarse_inputs(2, 77, 45, gain=0.5, seed=93)]
    dsets = [[torch.as_tensor(a, device=DEV) for a in s] for s in sets]
    want = [ops.coarse_transformer(x0, x1, packed, cr.FOUR_LAYERS) for x0, x1 in dsets]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    s0, s1 = dsets[0][0].clone(), dsets[0][1].clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ops.coarse_transformer(s0, s1, packed, cr.FOUR_LAYERS)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = ops.coarse_transformer(s0, s1, packed, cr.FOUR_LAYERS)
    got = []
    with torch.cuda.stream(side):
        for k in (0, 1, 0):
            s0.copy_(dsets[k][0]); s1.copy_(dsets[k][1])
            g.replay()
            got.append((k, out[0].clone(), out[1].clone()))
    side.synchronize()
    for r, (k, o0, o1) in enumerate(got):
        same = np.array_equal(_bits(o0), _bits(want[k][0])) and np.array_equal(_bits(o1), _bits(want[k][1]))
        print(f"RPL coarse_transformer replay {r} input set {k}  {'= eager bits' if same else 'FAILED: bits differ'}")
        assert same, (r, k)
    assert not np.array_equal(_bits(want[0][0]), _bits(want[1][0]))


@pytest.mark.parametrize("w", [5, 7])
def test_fine_context_layers_replayed(w):
    """ops.fine_transformer (M = 37) with a two-element `status` zeroed inside the capture, replayed on mixed gains (some
    matches lower their scale), calm gains (none does: status [0, 0]) and mixed gains again: outputs and status equal
    the eager call's bits each time"""
    packed = ops.pack_fine_transformer({k: torch.as_tensor(v) for k, v in cr.fine_weights().items()}, DEV)
    sets = {"mixed": cr.fine_inputs(w, cr.fine_gains()), "calm": cr.fine_inputs(w, cr.fine_gains(calm=True))}
    dsets = {k: [torch.as_tensor(a, device=DEV) for a in v] for k, v in sets.items()}

    def call(x0, x1, status):
        status.zero_()
        return ops.fine_transformer(x0, x1, packed, status=status)
    want = {}
    for k, (x0, x1) in dsets.items():
        st = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        o0, o1 = call(x0, x1, st)
        torch.cuda.synchronize()
        want[k] = (o0, o1, st)
    side = torch.cuda.Stream(DEV)
    s0, s1 = dsets["mixed"][0].clone(), dsets["mixed"][1].clone()
    status = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        call(s0, s1, status)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = call(s0, s1, status)
    got = []
    with torch.cuda.stream(side):
        for k in ("mixed", "calm", "mixed"):
            s0.copy_(dsets[k][0]); s1.copy_(dsets[k][1])
            g.replay()
            got.append((k, out[0].clone(), out[1].clone(), status.clone()))
    side.synchronize()
    for r, (k, o0, o1, st) in enumerate(got):
        same = all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((o0, o1, st), want[k]))
        print(f"RPL fine_transformer W{w} replay {r} {k:5s} status {st.tolist()}  {'= eager bits' if same else 'FAILED: bits differ'}")
        assert same, (r, k, st.tolist(), want[k][2].tolist())
        if k == "calm":
            assert st.tolist() == [0, 0]
    assert want["mixed"][2].tolist()[0] == 0 and want["mixed"][2].tolist()[1] != 0      # the mixed gains do lower a scale
