"""Helpers shared by the trainable-Matcher tests and tools/probe_matcher_train.py (no tests here, nothing runs on a GPU
by itself): the seeded batch, matchers with a reproducible backbone and the fixtures' FinePreprocess weights, one training
step with its gradients, and the fine context layers alone against a float64 copy on a step's own windows."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from featurematching_amd import modules, synth, transformer
from featurematching_amd.matcher import Matcher

import supervision_ref as sref

DEV = "cuda:0"
HC, WC, HF, WF, W = 12, 16, 48, 64, 7
LOSS_CFG = {'fine_correct_thr': 1.0, 'pos_weight': 1.0, 'neg_weight': 1.0, 'pose_loss_cal_flag': False, 'coarse_type': 'focal',
            'focal_alpha': 0.25, 'focal_gamma': 2.0, 'coarse_weight': 1.0, 'fine_weight': 0.25}
CONFIG = {'module': {'loss': LOSS_CFG, 'match_coarse': {'sparse_spvs': False}}}
OPS = ("window_merge", "linear_attention", "encoder_tail", "qkv_projection")


def batch(seed, grad=False):
    """one pair of seeded images and 300 correspondences"""
    img = lambda k: torch.as_tensor(synth.normal(seed, k, (1, 3, HC * 8, WC * 8)), device=DEV).requires_grad_(grad)
    return {'image0': img(20), 'image1': img(21),
            'origin_kp0': torch.as_tensor(sref.points(seed, 300, (HC, WC), 0), device=DEV)[None],
            'origin_kp1': torch.as_tensor(sref.points(seed, 300, (HC, WC), 1), device=DEV)[None]}


class PatchBackbone(nn.Module):
    """A feature extractor without convolutions - 8 x 8 and 2 x 2 pixel patches through one Linear each - for the tests
    that compare two runs: the convolutions of the default backbone are not run-to-run reproducible on the GPU (the same
    eval-mode module gives other bits on its second call), in either direction, and at default initialisation the
    fine-level gradients - residuals of cancelling terms, max|g| ~ 1e-7 - carry that to 9e-3 of their own maximum
    between two runs of the SAME path (measured: profiles/matcher_train_accuracy.txt)."""

    def __init__(self, d_coarse=256, d_fine=64):
        super().__init__()
        self.coarse, self.fine = nn.Linear(3 * 64, d_coarse), nn.Linear(3 * 4, d_fine)

    def forward(self, x):
        n, _, h, w = x.shape
        c = F.layer_norm(self.coarse(F.unfold(x, 8, stride=8).transpose(1, 2)), (self.coarse.out_features,))
        f = self.fine(F.unfold(x, 2, stride=2).transpose(1, 2))
        return (c.transpose(1, 2).reshape(n, -1, h // 8, w // 8).contiguous(),
                f.transpose(1, 2).reshape(n, -1, h // 2, w // 2).contiguous())


def matcher(seed=3, patches=False, fixture_merge=False, **kw):
    """fixture_merge: FinePreprocess's two Linear layers hold synth.merge_weights - torch's default range for a Linear,
    what the reference's fixtures under tests/golden were made with - in place of the module's kaiming fan-out draw"""
    torch.manual_seed(seed)
    if patches:
        kw['backbone'] = PatchBackbone()
    m = Matcher(**kw)
    if fixture_merge:
        names = ('down_proj.weight', 'down_proj.bias', 'merge_feat.weight', 'merge_feat.bias')
        weights = synth.merge_weights(seed, m.config['coarse']['d_model'], m.config['fine']['d_model'])
        m.fine_preprocess.load_state_dict({k: torch.as_tensor(v) for k, v in zip(names, weights)})
    return m.to(DEV).train()


def loss_module():
    return modules.Loss(CONFIG).train()


def step(m, data):
    """one training step and its backward: (loss, name -> gradient) over every parameter and both images"""
    m.zero_grad(set_to_none=True)
    loss = m.training_step(data, loss_module())
    loss.backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads.update({'image0': data['image0'].grad, 'image1': data['image1'].grad})
    return loss.detach(), grads




def fine_layers_against_float64(m, data, switches=({}, dict(hip_attention=True), dict(hip_attention=True, hip_tail=True, hip_proj=True))):
    """One training step of matcher m (as it is) to capture what its fine LocalFeatureTransformer is given - the windows and
    the gradients of its outputs - then those layers alone, from m's weights, on these tensors: a float64 copy as the
    reference and one float32 run per entry of `switches`.  Returns (names, max|ref64| per name, [errors per run]) with
    errors max|x - ref64| / max|ref64| over every parameter's gradient, both input gradients and the first output."""
    cap = {}
    pre = m.fine.register_forward_pre_hook(lambda mod, args: cap.__setitem__('in', [a.detach().clone() for a in args]))

    def keep(mod, args, out):
        for i, o in enumerate(out):
            o.register_hook(lambda g, i=i: cap.__setitem__(i, g.detach().clone()))
    post = m.fine.register_forward_hook(keep)
    step(m, data)
    pre.remove(), post.remove()
    (x0, x1), g0, g1 = cap['in'], cap[0], cap[1]
    weights = m.fine.state_dict()

    def run(dtype, **kw):
        tf = transformer.LocalFeatureTransformer(m.config['fine'], **kw)
        tf.load_state_dict(weights)
        tf = tf.to(device=x0.device, dtype=dtype).train()
        a, b = (v.to(dtype).clone().requires_grad_(True) for v in (x0, x1))
        o0, o1 = tf(a, b)
        torch.autograd.backward([o0, o1], [g0.to(dtype), g1.to(dtype)])
        res = {k: p.grad for k, p in tf.named_parameters()}
        res.update(d_win0=a.grad, d_win1=b.grad, out0=o0.detach())
        return res
    ref = run(torch.float64)
    names = list(ref)
    tops = [ref[k].abs().max().item() for k in names]
    errs = [[(r[k].double() - ref[k]).abs().max().item() / t for k, t in zip(names, tops)]
            for r in (run(torch.float32, **kw) for kw in switches)]
    return names, tops, errs, x0.abs().max().item()
