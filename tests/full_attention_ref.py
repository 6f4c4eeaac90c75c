"""Inputs shared by the full-attention tests and tests/golden/make_golden_full_attention.py: the seeded q, k, v and upstream
gradient of linear_attention_ref (regenerated, never stored) and three kinds of data that an online softmax can get wrong.
Nothing here runs on a GPU by itself; the yardstick is featurematching_amd.transformer.full_attention."""
import numpy as np

from linear_attention_ref import autograd, inputs  # noqa: F401  (shared as they are)
from train_layers_yardstick import rel_err  # noqa: F401  (the error measure of the GPU tests)

# the fixture's cases: name -> (N, L, S, H, D)
GOLDEN_CASES = {
    "window": (3, 25, 49, 8, 8),
    "long": (1, 17, 23, 8, 32),
}
GOLDEN_SEED = 83
KINDS = ("shifted", "ramp", "ramp_down")


def hard_inputs(kind, seed, dims):
    """(q, k, v, g) float32 numpy on which float32 transformer.full_attention stays finite under autograd (2e-5 of
    float64 on `shifted`, at most 7e-6 on the ramps, at (2, 130, 97, 8, 8 | 32)):
      shifted   channel 0 of every head of q and of k is 30: every scaled score gains 900 / sqrt(D) (159 at D = 32, 318 at
                D = 8) and exp overflows unless the row maximum is subtracted first
      ramp      q, k at scale 3 and k times linspace(0.1, 4, S) along the tokens: the row maximum keeps rising through a
                sweep over the keys and the early tiles are rescaled to nothing
      ramp_down the same with the linspace reversed: the maximum is in the first tile"""
    if kind == "shifted":
        q, k, v, g = inputs(seed, dims)
        q[..., 0] = 30.0
        k[..., 0] = 30.0
        return q, k, v, g
    q, k, v, g = inputs(seed, dims, 3.0)
    ramp = np.linspace(0.1, 4.0, dims[2], dtype=np.float32)
    if kind == "ramp_down":
        ramp = ramp[::-1].copy()
    elif kind != "ramp":
        raise KeyError(kind)
    return q, k * ramp[None, :, None, None], v, g
