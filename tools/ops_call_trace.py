"""Record what the Python layer asks of the C ABI: one line per C call (name, every integer / float argument, for a
pointer only whether it is NULL, what came back through out-parameters) and a SHA-256 of the deterministic outputs,
over a fixed seeded list of small scenarios run through the public functions of ops.py.  Two trees whose ops.py make
the same calls print the same text:  python tools/ops_call_trace.py [--root TREE] > trace.txt  (a GPU is needed)."""
import argparse
import ctypes as C
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--all-bits", action="store_true", help="a SHA also for the gradients that depend on the arrival order of "
                "float atomics (to show that two runs of ONE build differ there)")
sys.path.insert(0, os.path.abspath(ap.parse_args().root))
ALL_BITS = ap.parse_args().all_bits

import numpy as np  # noqa: E402
import torch  # noqa: E402
from featurematching_amd import _lib, ops, synth  # noqa: E402

REAL = _lib.load()


def show(a, kind, base):
    if hasattr(a, "_obj"):                                   # byref(out-parameter), shown after the call
        v = a._obj.value
        return f"->+{(v or base) - base}" if isinstance(a._obj, C.c_void_p) else f"->{v!r}"
    if kind is C.c_void_p or not isinstance(a, (int, float)):
        return "NULL" if a is None or getattr(a, "value", 1) in (None, 0) else "ptr"
    return repr(a)


class Recorder:
    def __getattr__(self, name):
        fn, kinds = getattr(REAL, name), _lib.ALL_SIGNATURES[name][1]

        def call(*args):
            st = fn(*args)
            base = args[0].value if args and isinstance(args[0], C.c_void_p) and args[0].value else 0
            print(name, *[show(a, k, base) for a, k in zip(args, kinds)], "=", repr(st), flush=True)
            return st
        return call


_lib.load = lambda path=None: Recorder()
DEV = torch.device("cuda:0")
HW, HWF, SCALE = (15, 20), (60, 80), 8.0


def sha(name, *ts):
    for t in ts:
        t = t.detach().cpu().contiguous()
        t = t.view(torch.int16) if t.dtype == torch.bfloat16 else t             # (numpy has no bfloat16: the same bytes)
        print(f"  {name} {tuple(t.shape)} {hashlib.sha256(t.numpy().tobytes()).hexdigest()}")


def lists(tag, d, count=None):
    print(f" [{tag}] M={d['b_ids'].shape[0]}")
    sha(tag, *[d[k] for k in ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c", "mconf")], *([count] if count is not None else []))


def desc(dist="peaky", c=256, seed=11, dtype=torch.float32):
    f0, f1 = synth.coarse_descriptors(seed, 2, 300, c, dist)
    return torch.as_tensor(f0, device=DEV).to(dtype), torch.as_tensor(f1, device=DEV).to(dtype)


def run_async(tag, f0, f1, hw1=HW, **kw):
    print(f"# coarse_match_async {tag}")
    buf = ops.coarse_match_async(f0, f1, HW, hw1, SCALE, **kw)
    try:
        lists(tag, buf.sliced(buf.read_count()), buf.count)
    except _lib.FMatchError as e:
        print(f" [{tag}] status {e.status}")
    if kw.get("cell_maps", True):
        buf.cell_maps()
    if kw.get("stats") or kw.get("conf_matrix"):
        buf.softmax_stats()
    return buf


f0, f1 = desc()
ff0, ff1 = (torch.as_tensor(a, device=DEV) for a in synth.fine_maps(11, 2, 64, *HWF))
run_async("plain", f0, f1)
for flag in ("conf_matrix", "stats", "dense", "exact_screening", "exact_step", "flat", "alone"):
    run_async(flag, f0, f1, **{flag: True})
run_async("no_cell_maps", f0, f1, cell_maps=False)
side = run_async("side_map", f0, f1, side_map=ff1)
sc = torch.tensor([[1.0, 1.5], [2.0, 0.5]], device=DEV)
run_async("scales", f0, f1, scale0=sc, scale1=sc.flip(0))
run_async("float16", f0.half(), f1.half())
run_async("bfloat16", f0.bfloat16(), f1.bfloat16())
run_async("mixed_dtypes", f0, f1.half())
run_async("cap_slots", f0, f1, cap=500, cand_slots=16)
g0, g1 = desc(c=100, seed=12)
run_async("c100_s192", g0, g1[:, :192].contiguous(), hw1=(12, 16), stats=True)

for tag, dist, kw in (("peaky", "peaky", {}), ("borderline_1", "borderline", {}), ("borderline_2", "borderline", {}),
                      ("mixed", "mixed", {}), ("thr005", "peaky", dict(thr=0.05)), ("stats", "peaky", dict(stats=True))):
    print(f"# coarse_match {tag}")
    a0, a1 = desc(dist)
    res = ops.coarse_match(a0, a1, HW, HW, SCALE, **kw)
    buf = res["_coarse_buffers"]
    lists(tag, res, buf.count)
    print(f" [{tag}] shape={buf._shape} hint={buf.hint} attempts={buf.attempts} info={buf.info}")
    buf.cell_maps()
b, i, j = res["b_ids"], res["i_ids"], res["j_ids"]                          # of the stats=True call on f0, f1
print("# dual_softmax_at, coarse_loss")
with torch.no_grad():
    ops.dual_softmax_at(f0, f1, b, i, j, buf)
    for kind, sparse in (("focal", False), ("cross_entropy", False), ("focal", True)):
        ops.coarse_loss(f0, f1, b, i, j, buf, coarse_type=kind, sparse_spvs=sparse)
print("# pack_*_transformer")
for d, n_layers in ((256, 2), (64, 2)):
    sd = {k: torch.as_tensor(v) for k, v in synth.transformer_weights(3, d, n_layers).items()}
    ops.pack_coarse_transformer(sd, n_layers, DEV) if d == 256 else ops.pack_fine_transformer(sd, DEV)
print("# gather_windows, gather_windows_grad, fine_match_maps")
maps = {"nchw_f32": ff0, "nhwc_f32": ff0.contiguous(memory_format=torch.channels_last), "nchw_f16": ff0.half(),
        "view": torch.cat([ff0, ff0], 3)[:, :, :, 10:90]}
for tag, m in maps.items():
    sha("crop_" + tag, ops.gather_windows(m, b, i, 7, 4, HW[1]))
sha("crop_cells", ops.gather_windows(ff0, b, i, 7, 4, HW[1], cells=buf.cell_maps()[0], h_c=HW[0]))
with torch.no_grad():
    sha("crop_grad_fwd", ops.gather_windows_grad(ff0, b, i, 7, 4, HW[1], HW[0]))
mix = synth.mix_weights(11, 49)
mix0, mix1 = (torch.as_tensor(np.append(mix[k], mix[k + 1]).astype(np.float32), device=DEV) for k in (0, 2))
k0, k1 = res["mkpts0_c"], res["mkpts1_c"]
cl = torch.channels_last
sha("fine_nchw", *ops.fine_match_maps(ff0, ff1, b, i, j, 7, 4, HW[1], HW[1], mix0, mix1, k0, k1, 2.0))
sha("fine_nhwc", *ops.fine_match_maps(ff0.contiguous(memory_format=cl), ff1.contiguous(memory_format=cl), b, i, j, 7, 4,
                                      HW[1], HW[1], mix0, mix1, k0, k1, 2.0))
m = side.read_count()
so = side.sliced(m)
sha("fine_prepared", *ops.fine_match_maps(ff0, ff1, so["b_ids"], so["i_ids"], so["j_ids"], 7, 4, HW[1], HW[1], mix0, mix1,
                                          so["mkpts0_c"], so["mkpts1_c"], 2.0, prepared=side.side_scratch))
print("# gather_merge_windows, gather_windows_pair, more gather_windows, gather_windows_backward, fine_match_maps float16")
gen = torch.Generator().manual_seed(11)
packed = ops.pack_merge_weights((torch.randn(64, 128, generator=gen) * 0.1).to(DEV))
ctx0, ctx1 = ((torch.randn(2, HW[0] * HW[1], 64, generator=gen) * 0.5).to(DEV) for _ in range(2))
cells0, cells1 = buf.cell_maps()
merge_maps = {"nchw_f32": ff0, "nhwc_f32": ff0.contiguous(memory_format=cl), "nhwc_f16": ff0.half().contiguous(memory_format=cl)}
for tag, m in merge_maps.items():
    for how, cm in (("list", None), ("cells", cells0)):
        sha(f"merge_{tag}_{how}", ops.gather_merge_windows(m, packed, ctx0, b, i, 7, 4, *HW, cells=cm))
sha("pair_plain", *ops.gather_windows_pair(ff0, ff1, b, i, j, 7, 4, HW, HW, (cells0, cells1)))
sha("pair_merge", *ops.gather_windows_pair(ff0, ff1, b, i, j, 7, 4, HW, HW, (cells0, cells1), packed_w=packed, ctx0=ctx0,
                                           ctx1=ctx1))
sha("pair_merge_nhwc", *ops.gather_windows_pair(ff0.contiguous(memory_format=cl), ff1.contiguous(memory_format=cl), b, i, j, 7,
                                                4, HW, HW, None, packed_w=packed, ctx0=ctx0, ctx1=ctx1))
sha("crop_nchw_bf16", ops.gather_windows(ff0.bfloat16(), b, i, 7, 4, HW[1]))
sha("crop_nhwc_f16", ops.gather_windows(ff0.half().contiguous(memory_format=cl), b, i, 7, 4, HW[1]))
d_win = torch.randn(b.shape[0], 49, 64, generator=gen).to(DEV)
for layout in (0, 1):
    sha(f"crop_backward_layout{layout}", ops.gather_windows_backward(d_win, b, i, (2, 64, *HWF), 7, 4, HW[1], HW[0], layout=layout))
sha("fine_nchw_f16", *ops.fine_match_maps(ff0.half(), ff1.half(), b, i, j, 7, 4, HW[1], HW[1], mix0, mix1, k0, k1, 2.0))


def train(tag, fn, a0=f0, a1=f1, bits=True):
    """fn(leaf0, leaf1) -> scalar, then .backward(); the SHA of the value and of the two gradients where their bits are
    the same every run (bits=False: the value's alone - the dense row / column sums the gradients are formed from are
    float atomics in arrival order)"""
    x0, x1 = (a.detach().clone().requires_grad_(True) for a in (a0, a1))
    val = fn(x0, x1)
    val.backward()
    sha(tag, val)
    if bits or ALL_BITS:
        sha(tag + ("" if bits else "_arrival_order"), x0.grad, x1.grad)
    else:
        print(f"  {tag} {tuple(x0.grad.shape)} {x0.grad.dtype} {tuple(x1.grad.shape)} {x1.grad.dtype} (no SHA)")


# the supervision is the stats=True call's own matches: mutual nearest neighbours, no two share a row or a column, so the
# sparse routes' float atomics meet no second addend and their outputs are the same bits every run
print("# training: dual_softmax_at, coarse_loss, attach_conf_matrix_grad, bfloat16, fine_loss - each with .backward()")
w = torch.linspace(0.5, 1.5, b.shape[0], device=DEV)
train("dsm_at", lambda x0, x1: (ops.dual_softmax_at(x0, x1, b, i, j, buf) * w).sum())
train("closs_focal", lambda x0, x1: ops.coarse_loss(x0, x1, b, i, j, buf), bits=False)
train("closs_xent", lambda x0, x1: ops.coarse_loss(x0, x1, b, i, j, buf, coarse_type="cross_entropy"), bits=False)
train("closs_focal_sparse", lambda x0, x1: ops.coarse_loss(x0, x1, b, i, j, buf, sparse_spvs=True))
train("closs_empty", lambda x0, x1: ops.coarse_loss(x0, x1, b[:0], i[:0], j[:0], buf), bits=False)
cbuf = ops.coarse_match_async(f0, f1, HW, HW, SCALE, conf_matrix=True)
cbuf.read_count()
gsel = torch.zeros_like(cbuf.conf_matrix)
gsel[b, i, j] = w
train("conf_grad_sparse", lambda x0, x1: (ops.attach_conf_matrix_grad(x0, x1, cbuf.conf_matrix, 0.1, cbuf) * gsel).sum())
gall = torch.rand(cbuf.conf_matrix.shape, generator=gen).to(DEV)
train("conf_grad_dense", lambda x0, x1: (ops.attach_conf_matrix_grad(x0, x1, cbuf.conf_matrix, 0.1, cbuf) * gall).sum(), bits=False)
train("dsm_at_bf16", lambda x0, x1: (ops.dual_softmax_at(x0, x1, b, i, j, buf) * w).sum(), f0.bfloat16(), f1.bfloat16())
e0, e1 = (torch.randn(b.shape[0], 3, generator=gen).to(DEV) for _ in range(2))
gt0, gt1 = (torch.randn(b.shape[0], 2, generator=gen).to(DEV) for _ in range(2))
train("fine_loss", lambda x0, x1: ops.fine_loss(x0, x1, gt0, gt1), e0, e1)
torch.cuda.synchronize()
print("# done")
