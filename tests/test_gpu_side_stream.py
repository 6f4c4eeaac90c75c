"""Every launch goes to the caller's stream.

Every Python wrapper takes torch.cuda.current_stream(device), and the suite calls them on the default stream, where a
launch, a hipMemsetAsync or a host read that goes to the null stream instead changes nothing.  Here every call runs on a
side stream `s` behind a delay:
  1. every input of the case is allocated as a device tensor of zeros, and the device is synchronised - zeros are valid
     input everywhere (floats, ids and counts alike), so misplaced work reads valid memory, computes a different answer
     and cannot index out of range;
  2. inside `with torch.cuda.stream(s)` a chain of large float32 matmuls on scratch tensors is enqueued (ordinary torch
     work, no spin kernel), an event `e` is recorded behind it, the real data is copy_'d into the inputs, and the call under
     test is made;
  3. `e.query()` is False just before the call - the delay is self-checking; make the chain longer if that ever fails -
     and, for the calls documented as not synchronising the host (coarse_match_async, gather_windows*, fine_match,
     fine_match_maps, fine_transformer with `status`, coarse_transformer, estimate_poses), still False when they return;
  4. after s.synchronize() every output equals the bits of the same call on the default stream with the real inputs.
Work that went to another stream ran before the copies, or before a memset of `s`, and gives other bits.
The cases that begin with the synchronous coarse call (dual_softmax_at, attach_conf_matrix_grad, coarse_loss) have lost
the delay once that call has read its count: behind it the descriptors are zeroed at once, a second delay is enqueued and
the real data copied behind it, so the training kernels these cases are about run behind pending work too.
One RPL line per run (`pytest -s`).

These comparisons found fm_dual_softmax_backward_dense, fm_coarse_loss_backward and the supervised entries' own term adding
with float atomics in arrival order: two plain runs differed in the last bits of d_feat.  The sums are order-fixed now
(DESIGN.md section 6n), and the cases that reach them are held to the same bits as every other.
"""
import pytest
import torch

import ctx_layers_ref as cr
import reuse_cases as rc
import step_cases as sc
from featurematching_amd import ops
from helpers import net_tail_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHAIN = 64              # matmuls of the delay, each 4096 x 4096 x 4096 in float32
_DELAY = {}


def _delay():
    """enqueue the chain on the current stream"""
    if not _DELAY:
        g = torch.Generator(device=DEV).manual_seed(3)
        _DELAY['a'] = torch.randn(4096, 4096, device=DEV, generator=g) / 64.0      # spectral norm ~ 2: the chain stays finite
        _DELAY['x'] = torch.randn(4096, 4096, device=DEV, generator=g)
        torch.cuda.synchronize()
    x = _DELAY['x']
    for _ in range(CHAIN):
        x = torch.mm(x, _DELAY['a']) * 0.5
    return x


def _zeros_like(d):
    return {k: (torch.zeros_like(v) if torch.is_tensor(v) else v) for k, v in d.items()}


def _behind_a_delay(name, real, run, no_sync, finish=None):
    """`run` on the default stream with the real inputs, then on a side stream behind the delay from inputs that are zero
    until the copies of that stream land; returns the names whose bits differ"""
    finish = finish or (lambda out: out)
    torch.cuda.synchronize()
    ops.MODE_MEMORY.clear()          # (the auto entry point's hint memory: both runs start from the same host state)
    want = run(real)
    torch.cuda.synchronize()
    want = finish(want)
    d = _zeros_like(real)
    side = torch.cuda.Stream(DEV)
    e = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        keep = _delay()
        e.record(side)
        for k, v in d.items():
            if torch.is_tensor(v):
                v.copy_(real[k])
        ops.MODE_MEMORY.clear()
        again = []

        def after_coarse(dd):
            """a case's coarse call has read the count on the host and drained the stream: descriptors back to zero at
            once, a second delay, the real data behind it - what the case launches next is behind pending work again"""
            for k in ("f0", "f1"):
                dd[k].zero_()
            again.append(_delay())
            again.append(torch.cuda.Event())
            again[1].record(side)
            for k in ("f0", "f1"):
                dd[k].copy_(real[k])
            again.append(again[1].query())
        if "f0" in d:
            d['after_coarse'] = after_coarse
        before = e.query()
        got = run(d)
        after = e.query()
    side.synchronize()
    del keep
    if again:
        assert not again[2], "the second delay had run out before the launches behind it: lengthen CHAIN"
        name = name + " (2 delays)"
    got = finish(got)
    bad = rc.same_bits(got, want)
    verdict = "= the default stream's bits: " + ", ".join(want) if not bad else "FAILED: " + ", ".join(rc.difference(got, want, bad))
    print(f"RPL side stream {name:34s} delay pending before the call: {not before}, when it returned: {not after}  {verdict}")
    assert not before, "the delay had run out before the call: lengthen CHAIN"
    if no_sync:
        assert not after, "the call is documented as not synchronising, and the delay had run out when it returned"
    return bad


@pytest.mark.parametrize("name", list(rc.CASES))
def test_workspace_entry_points_on_a_side_stream(name):
    build, run, no_sync = rc.CASES[name]
    bad = _behind_a_delay(name, rc.to_device(build("small"), DEV), run, no_sync)
    assert not bad, bad


STEP_SETS = {"maps_fused": ("peaky", 7001, 1, 256, 5), "maps_nhwc": ("borderline", 7001, 2, 64, 5),
             "windows": ("peaky", 7002, 1, 64, 7)}


@pytest.mark.parametrize("route", sc.ROUTES)
def test_step_on_a_side_stream(route):
    """coarse_match_async and the fine half of each route: no host synchronisation, the first M rows and the count equal
    the default stream's"""
    s = sc.input_set(*STEP_SETS[route])
    real = sc.to_device(s, route, DEV)
    mode = sc.learnt_mode(real)
    bufs = sc.Bufs(s['n'], s['w'], DEV)

    def run(d):
        return sc.outputs(sc.step(d, route, mode, bufs))

    def finish(out):
        m = int(out['count'][0].item())
        assert m == sc.oracle_of(s)['i_ids'].shape[0]
        return {k: (v if k == "count" else v[:m]).clone() for k, v in out.items()}
    bad = _behind_a_delay(f"step {route}", real, run, True, finish)
    assert not bad, bad


def test_matcher_forward_features_on_a_side_stream():
    """Matcher().eval().forward_features on the net_tail_small inputs: context layers, coarse matching, crop + merge, fine
    layers and fine matching, with its host reads of the count and of the fine kernel's range report"""
    from featurematching_amd.matcher import Matcher
    inp = net_tail_inputs()
    m = Matcher().to(DEV).eval()
    t = lambda d: {k: torch.as_tensor(v) for k, v in d.items()}
    m.coarse.load_state_dict(t(inp['w_coarse']))
    m.fine.load_state_dict(t(inp['w_fine']))
    m.fine_preprocess.load_state_dict(t(inp['w_prep']))
    w0, b0, w1, b1 = inp['mix']
    with torch.no_grad():
        m.fine_matching.mix_feat_0.weight.copy_(torch.as_tensor(w0).view(1, -1)); m.fine_matching.mix_feat_0.bias.fill_(float(b0))
        m.fine_matching.mix_feat_1.weight.copy_(torch.as_tensor(w1).view(1, -1)); m.fine_matching.mix_feat_1.bias.fill_(float(b1))
    real = {k: torch.as_tensor(inp[k], device=DEV) for k in ("feat_c0", "feat_c1", "feat_f0", "feat_f1")}

    def run(d):
        data = {'bs': 2, 'hw0_i': inp['hw_i'], 'hw1_i': inp['hw_i']}
        with torch.no_grad():
            m.forward_features(d['feat_c0'], d['feat_c1'], d['feat_f0'], d['feat_f1'], data)
        return {k: v for k, v in data.items() if torch.is_tensor(v)}
    bad = _behind_a_delay("Matcher.forward_features", real, run, False)
    assert not bad, bad


def test_context_layers_packed_and_run_on_a_side_stream():
    """pack_coarse_transformer / pack_fine_transformer followed by their transformer call, both on the side stream: the
    weights are zero until that stream's copies land, so a pack kernel on another stream packs zeros"""
    wc = {k: torch.as_tensor(v, device=DEV) for k, v in cr.coarse_weights(4).items()}
    x0, x1 = cr.coarse_inputs(2, 77, 45)
    real = dict(wc, x0=torch.as_tensor(x0, device=DEV), x1=torch.as_tensor(x1, device=DEV))

    def run_coarse(d):
        packed = ops.pack_coarse_transformer({k: v for k, v in d.items() if k not in ("x0", "x1")}, 4, DEV)
        o0, o1 = ops.coarse_transformer(d['x0'], d['x1'], packed, cr.FOUR_LAYERS)
        return dict(packed=packed, out0=o0, out1=o1)
    bad = _behind_a_delay("pack + coarse_transformer", real, run_coarse, False)

    wf = {k: torch.as_tensor(v, device=DEV) for k, v in cr.fine_weights().items()}
    for w in (5, 7):
        f0, f1 = cr.fine_inputs(w)
        real = dict(wf, x0=torch.as_tensor(f0, device=DEV), x1=torch.as_tensor(f1, device=DEV),
                    status=torch.zeros(2, dtype=torch.int32, device=DEV))

        def run_fine(d):
            packed = ops.pack_fine_transformer({k: v for k, v in d.items() if k not in ("x0", "x1", "status")}, DEV)
            d['status'].zero_()
            o0, o1 = ops.fine_transformer(d['x0'], d['x1'], packed, status=d['status'])
            return dict(packed=packed, out0=o0, out1=o1, status=d['status'])
        bad += _behind_a_delay(f"pack + fine_transformer W{w}", real, run_fine, False)
    assert not bad, bad


def test_transformer_calls_do_not_synchronise():
    """coarse_transformer and fine_transformer with `status` from weights packed beforehand: the delay is still pending
    when they return"""
    packed_c = ops.pack_coarse_transformer({k: torch.as_tensor(v) for k, v in cr.coarse_weights(4).items()}, 4, DEV)
    packed_f = ops.pack_fine_transformer({k: torch.as_tensor(v) for k, v in cr.fine_weights().items()}, DEV)
    x0, x1 = cr.coarse_inputs(2, 77, 45)
    real = dict(x0=torch.as_tensor(x0, device=DEV), x1=torch.as_tensor(x1, device=DEV))
    bad = _behind_a_delay("coarse_transformer", real,
                          lambda d: dict(zip(("out0", "out1"), ops.coarse_transformer(d['x0'], d['x1'], packed_c, cr.FOUR_LAYERS))), True)
    f0, f1 = cr.fine_inputs(7)
    real = dict(x0=torch.as_tensor(f0, device=DEV), x1=torch.as_tensor(f1, device=DEV),
                status=torch.zeros(2, dtype=torch.int32, device=DEV))

    def run_fine(d):
        d['status'].zero_()
        o0, o1 = ops.fine_transformer(d['x0'], d['x1'], packed_f, status=d['status'])
        return dict(out0=o0, out1=o1, status=d['status'])
    bad += _behind_a_delay("fine_transformer with status", real, run_fine, True)
    assert not bad, bad


def test_window_crops_do_not_synchronise():
    """gather_windows (list order, both layouts) and gather_windows_pair (cell order) behind a coarse call of the same
    stream"""
    s = sc.input_set("peaky", 7003, 1, 64, 7)
    real = sc.to_device(s, "windows", DEV)
    mode = sc.learnt_mode(real)

    def run(d):
        buf = sc.coarse(d, mode, cell_maps=True)
        w0 = ops.gather_windows(d['ff0'], buf.b_ids, buf.i_ids, 7, sc.STRIDE, sc.HW_C[1], count=buf.count)
        cl = ops.gather_windows(d['ff1'].contiguous(memory_format=torch.channels_last), buf.b_ids, buf.j_ids, 7, sc.STRIDE,
                                sc.HW_C[1], count=buf.count)
        p0, p1 = ops.gather_windows_pair(d['ff0'], d['ff1'], buf.b_ids, buf.i_ids, buf.j_ids, 7, sc.STRIDE, sc.HW_C, sc.HW_C,
                                         buf.cell_maps(), count=buf.count)
        out = dict(count=buf.count, list0=w0, list1_nhwc=cl, pair0=p0, pair1=p1)
        out['_keep'] = buf.workspace
        return out

    def finish(out):
        m = int(out['count'][0].item())
        return {k: (v if k == "count" else v[:m]).clone() for k, v in out.items() if k != "_keep"}
    bad = _behind_a_delay("gather_windows, gather_windows_pair", real, run, True, finish)
    assert not bad, bad
