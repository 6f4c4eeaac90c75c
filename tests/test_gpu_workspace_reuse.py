"""The same bits whatever the workspace held.

include/fmatch.h promises that the library keeps no state and asks nothing of a workspace's contents.  The suite's other
tests hand every call the block torch.empty has just given out - typically what the previous, identical call freed - or
one byte pattern (0xFF).  Here every Python-side workspace request (ops._aligned_workspace, patched for the duration of a
test; still one buffer of its own per request, kept alive by the caller as ever) is first filled
  * `zero`:     with zeros,
  * `ff`:       with 0xFF bytes,
  * `leftover`: not at all - the k-th request is served with the very buffer the k-th request of a run of the same entry
                point on a BIGGER, DIFFERENT problem left behind: counters with plausible values, candidate lists with
                valid ids, cell maps that point at real rows, partial sums of another problem.  Every request of the small
                run must be served this way from a recorded buffer that is large enough; none falls back to a fresh one.
Every output, and every gradient where the entry point has a backward, of the small problem must be the same bits under
all three and in an unpatched run.  The small problems come from the input builders of the tests that pin them to float64
(tests/reuse_cases.py), so the unpatched result is one the suite already holds to float64.

post.estimate_poses allocates its workspace itself (patched inside featurematching_amd.post for the test);
ops.fine_match_maps takes `scratch=` from the caller (filled by the test).  One RPL line per run (`pytest -s`).

These comparisons found fm_dual_softmax_backward_dense, fm_coarse_loss_backward and the supervised entries' own term adding
with float atomics in arrival order: two plain runs differed in the last bits of d_feat.  The sums are order-fixed now
(DESIGN.md section 6n), and the cases that reach them are held to the same bits as every other.
"""
import pytest
import torch

import reuse_cases as rc
from featurematching_amd import ops, post

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILLS = ("zero", "ff", "leftover")


class Workspaces:
    """stands in for ops._aligned_workspace: `record` keeps every buffer it hands out (unfilled, as ever), the fills hand
    out a buffer per request prepared as the fill says"""

    def __init__(self, how, recorded=None):
        self.how, self.recorded, self.kept, self.requests = how, recorded or [], [], 0

    def buffer(self, nbytes, device):
        k, self.requests = self.requests, self.requests + 1
        if self.how == "record":
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.kept.append(ws)
        elif self.how == "zero":
            ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        elif self.how == "ff":
            ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=device)
        else:
            assert k < len(self.recorded), f"request {k}: the bigger run made {len(self.recorded)} requests only"
            ws = self.recorded[k]
            assert ws.numel() >= nbytes, f"request {k}: {nbytes} bytes asked, the bigger run left {ws.numel()}"
        return ws

    def __call__(self, nbytes, device):
        ws = self.buffer(nbytes + 256, device)
        return ws, ops._aligned(ws)


class _PoseTorch:
    """featurematching_amd.post's `torch` for a test: its one uint8 torch.empty - the pose workspace - goes through a
    Workspaces object, everything else is torch"""

    def __init__(self, workspaces):
        self._ws = workspaces

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        if kw.get("dtype") is torch.uint8:
            return self._ws.buffer(int(size[0]), kw.get("device"))
        return torch.empty(*size, **kw)


def _patch(monkeypatch, ws):
    monkeypatch.setattr(ops, "_aligned_workspace", ws)
    monkeypatch.setattr(post, "torch", _PoseTorch(ws))


def _run(name, size, monkeypatch=None, ws=None, **replace):
    build, run, _ = rc.CASES[name]
    d = rc.to_device(build(size), DEV)
    d.update(replace)
    torch.cuda.synchronize()
    ops.MODE_MEMORY.clear()          # (the auto entry point's hint memory: every run starts from the same host state)
    if ws is not None:
        _patch(monkeypatch, ws)
    try:
        out = run(d)
        torch.cuda.synchronize()
    finally:
        if ws is not None:
            monkeypatch.undo()
    return out, d


WORKSPACE_CASES = [n for n in rc.CASES if n != "fine_match_maps"]


@pytest.mark.parametrize("name", WORKSPACE_CASES)
def test_same_bits_whatever_the_workspace_held(name, monkeypatch):
    base, _ = _run(name, "small")
    counter = Workspaces("record")
    again, _ = _run(name, "small", monkeypatch, counter)
    assert counter.requests > 0, "this case reaches no workspace"
    bad = rc.same_bits(again, base)
    print(f"RPL workspace {name:32s} {'again':8s} {counter.requests} request(s)  "
          f"{'= the bits of the first unpatched run' if not bad else 'FAILED: ' + ', '.join(rc.difference(again, base, bad))}")
    failures = [f"a second unpatched run: {k}" for k in rc.difference(again, base, bad)]
    for how in FILLS:
        recorded = None
        if how == "leftover":
            big = Workspaces("record")
            _run(name, "big", monkeypatch, big)
            recorded = big.kept
        ws = Workspaces(how, recorded)
        got, _ = _run(name, "small", monkeypatch, ws)
        assert ws.requests == counter.requests
        bad = rc.same_bits(got, base)
        print(f"RPL workspace {name:32s} {how:8s} {ws.requests} request(s)  "
              f"{'= the unpatched bits: ' + ', '.join(base) if not bad else 'FAILED: ' + ', '.join(rc.difference(got, base, bad))}")
        failures += [f"{how}: {k} (against the unpatched run)" for k in rc.difference(got, base, bad)]
    assert not failures, failures


def test_fine_match_maps_whatever_the_callers_scratch_held():
    """NCHW float32 maps: image 1's channels-last copy is made in the caller's scratch.  The same keypoints from a scratch
    of zeros, of 0xFF bytes, and from the one a call on set 7003 at twice the batch has just filled."""
    name = "fine_match_maps"
    base, d = _run(name, "small")
    _, big = _run(name, "big")
    assert big['scratch'].numel() >= 2 * d['scratch'].numel() and big['scratch'].any().item()
    fills = dict(zero=torch.zeros_like(d['scratch']), ff=torch.full_like(d['scratch'], 0xFF), leftover=big['scratch'])
    failures = []
    for how, scratch in fills.items():
        got, _ = _run(name, "small", scratch=scratch)
        bad = rc.same_bits(got, base)
        print(f"RPL workspace {name:32s} {how:8s} caller's scratch  "
              f"{'= the bits of a fresh scratch: ' + ', '.join(base) if not bad else 'FAILED: ' + ', '.join(bad)}")
        failures += [f"{how}: {k} differs" for k in bad]
    assert not failures, failures
