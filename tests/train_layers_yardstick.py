"""What the GPU tests of the four HIP training layers of the fine level share (tests/test_gpu_linear_attention.py,
test_gpu_encoder_tail.py, test_gpu_qkv_projection.py, test_gpu_window_merge.py, and the call counter of
test_gpu_matcher_train.py too); no tests here, nothing runs on a GPU by itself.  The one copy of: the error measure, the
acceptance bar of a layer against float64, the seeded LocalFeatureTransformer and one training step of it, the counter of
calls into ops, and the peak-memory probe.  Each test file keeps its own FLOOR: those are measured per layer."""
import torch

from featurematching_amd import ops, synth, transformer

DEV = "cuda:0"


def rel_err(x, ref):
    """max|x - ref| / max|ref| (0 for an all-zero reference that is met exactly)"""
    top = ref.abs().max().item()
    err = (x.double() - ref.double()).abs().max().item()
    return err / top if top > 0 else err


def hold(tag, names, hip, ref32, ref64, floor):
    """The bar of a layer: print every figure, then hold every tensor of `hip` to its shape, float32, finiteness and
        e_hip <= 4 e_ref + floor,   e_x = max|x - ref64| / max|ref64|
    with e_ref that of the float32 torch path.  The three tuples are of one length, `names` may go on beyond it."""
    assert len(hip) == len(ref32) == len(ref64) <= len(names), tag
    rows = []
    for name, h, r32, r64 in zip(names, hip, ref32, ref64):
        assert h.shape == r64.shape and h.dtype == torch.float32, (tag, name)
        finite = bool(torch.isfinite(h).all())
        e_hip, e_ref = rel_err(h, r64), rel_err(r32, r64)
        print(f"ACC  {tag:34s} {name:22s} max|ref64| {r64.abs().max().item():.3e}  e_ref {e_ref:.3e}  e_hip {e_hip:.3e}")
        rows.append((name, finite, e_hip, e_ref))
    for name, finite, e_hip, e_ref in rows:
        assert finite, (tag, name)
        assert e_hip <= 4 * e_ref + floor, (tag, name, e_hip, e_ref)


def module(cfg, dtype=torch.float32, **kw):
    m = transformer.LocalFeatureTransformer(cfg, **kw)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in
                       synth.transformer_weights(7, cfg['d_model'], len(cfg['layer_names'])).items()})
    return m.to(device=DEV, dtype=dtype).train()


def module_run(m, x0, x1, g0, g1, dtype, **kw):
    """one training step of m in `dtype`: (names, [both outputs, both input gradients, every parameter's gradient])"""
    a, b = (t.detach().to(dtype, copy=True).requires_grad_(True) for t in (x0, x1))
    o0, o1 = m(a, b, **kw)
    assert o0.grad_fn is not None and o1.grad_fn is not None
    torch.autograd.backward([o0, o1], [g0.to(dtype), g1.to(dtype)])
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert all(p is not None for p in grads.values()), [k for k, p in grads.items() if p is None]
    keys = sorted(grads)
    return ["out0", "out1", "d_feat0", "d_feat1"] + keys, [o0.detach(), o1.detach(), a.grad, b.grad] + [grads[k] for k in keys]


def count_calls(monkeypatch, *names):
    """name -> how often ops.<name> has been called since, for each of `names`"""
    calls = {k: 0 for k in names}
    for name in names:
        def counted(*a, _real=getattr(ops, name), _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls


def peak_above_inputs(fn, leaves, g, *args):
    """peak bytes allocated above what is there already by fn(*leaves, *args) and its backward from the upstream
    gradient(s) g to every leaf"""
    leaves = [t.detach().requires_grad_(True) for t in leaves]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(*leaves, *args)
    grads = torch.autograd.grad(out, leaves, g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out, grads
    return peak
