"""Integrated gradients (Sundararajan et al. 2017, "Axiomatic Attribution for Deep Networks"):
average the input gradient over K points of the straight line from a baseline x0 to the state x
and scale it by x - x0.  The attributions of a state then sum, up to the error of the K-point
rule, to f(x) - f(x0) (completeness), which the raw input gradient and the perturbation map do
not offer.

This module states the whole rule in numpy and is the oracle of csrc/ba3c_intgrad.h: of
`ba3c_ig_states` bit for bit, of `ba3c_ig_accumulate` in float64.

Path states.  K steps, 1 <= K <= 256.  Path state j in [0, K) of a state is the midpoint-rule
point x0 + (2j+1)/(2K) (x - x0).  The network reads uint8 frames (its first kernel converts the
bytes itself), so the path has to be uint8 too: per byte, with d = x - x0 as a signed integer,
    p_j = x0 + floor(((2j+1) d + K) / (2K))
in integers (floor also for a negative numerator): the midpoint rounded half up.  The rounding
is part of the rule, not an error of the kernel: the gradients are taken at exactly these states,
and p_j never leaves [min(x0, x), max(x0, x)].  Path state n K + j belongs to source state n.

Baselines.  "zero": x0 = 0.  "blur": every history plane replaced by its Gaussian blur under
perturb.py's fixed-point blur A (sigma 3, radius 9, reflected edges; the whole frame, no mask),
the exact Q24 value rounded half up to a byte: x0 = (blur + 2^23) >> 24, which is what
perturb.py's blend gives under a full mask.

Attribution.  With g_j = Ba3cEngine.input_grads at path state j, the gradient per unit of the
float frames the network sees (state / 255, saliency.py's convention),
    attr[y, x, c] = (x - x0)[y, x, c] / 255 * (1 / K) sum_j g_j[y, x, c]
the sum in float64 in ascending j, the product (d / 255) * (sum / K) formed in float64 and
rounded once to float32.  sum(attr) approaches f(x) - f(x0) as K grows.
"""
import numpy as np

from .perturb import H, W, blur_q24

MAX_STEPS = 256
BASELINES = {"zero": 0, "blur": 1}      # ba3c_ig_states' `baseline`


def baseline_numpy(state, baseline):
    """state uint8 [..., 84, 84, 4] -> x0, uint8 of the same shape."""
    state = np.asarray(state)
    assert state.dtype == np.uint8 and state.shape[-3:] == (H, W, 4), state.shape
    if BASELINES[baseline] == 0:
        return np.zeros_like(state)
    return np.ascontiguousarray(((blur_q24(state) + (1 << 23)) >> 24).astype(np.uint8))


def path_bytes(x0, x, steps):
    """The byte rule: integer arrays x0, x of one shape -> int64 [steps, ...], the K path points."""
    assert 1 <= steps <= MAX_STEPS, steps
    x0, x = np.asarray(x0, np.int64), np.asarray(x, np.int64)
    t = (2 * np.arange(steps, dtype=np.int64) + 1).reshape((steps,) + (1,) * x.ndim)
    return x0 + (t * (x - x0) + steps) // (2 * steps)


def path_states(state, steps, baseline="blur"):
    """state uint8 [n, 84, 84, 4] -> uint8 [n * steps, 84, 84, 4], state-major, j minor."""
    state = np.asarray(state)
    p = path_bytes(baseline_numpy(state, baseline), state, steps)          # [K, n, ...]
    return np.ascontiguousarray(np.moveaxis(p, 0, 1).reshape((-1,) + state.shape[1:]).astype(np.uint8))


def attribution(state, grads, steps, baseline="blur"):
    """grads [n * steps, 84, 84, 4], the input gradients at path_states(state, steps, baseline)
    -> float32 [n, 84, 84, 4], the rule above."""
    state = np.asarray(state)
    g = np.asarray(grads, np.float64).reshape((state.shape[0], steps) + state.shape[1:])
    acc = np.zeros(state.shape, np.float64)
    for j in range(steps):
        acc += g[:, j]
    d = state.astype(np.int64) - baseline_numpy(state, baseline)
    return ((d / 255.0) * (acc / float(steps))).astype(np.float32)
