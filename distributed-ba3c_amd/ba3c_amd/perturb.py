"""Perturbation saliency (Greydanus et al. 2018, "Visualizing and Understanding Atari Agents"):
blur a small patch of the frames around every point of a coarse grid, run the policy on each
perturbed state, and score how far the value and the policy move.

This module states the whole rule in numpy, integer where the kernels are integer, and is the
oracle of csrc/ba3c_perturb.h (`ba3c_perturb_states`, `ba3c_perturb_scores`).

Centres.  (5i, 5j) for i, j in 0..16: 289 per state (the paper's stride 5).  Perturbed state
n * 289 + 17 i + j belongs to source state n.

Blur A.  A separable Gaussian, sigma 3, radius 9 (19 taps), over each of the four history planes
on its own.  WEIGHTS are integers in Q12 that sum to exactly 4096 (the centre tap absorbs the
rounding remainder); edges reflect symmetrically (d c b a | a b c d).  Neither pass is rounded, so
the blurred pixel is an exact Q24 integer <= 255 * 2^24 (it fits an unsigned 32-bit value), and
the order of the two passes does not matter.

Mask M.  m(dy, dx) = MASK_Q[|dy|] * MASK_Q[|dx|] in Q16, MASK_Q[t] = round(256 exp(-t^2 / 50))
(sigma 5, peak 256) for t <= 15 and 0 beyond.

Blend.  out = (p * 2^24 * (2^16 - m) + blur * m + 2^39) >> 40 in 64-bit integers: round half up,
a byte.  newest=False perturbs all four planes with the same mask, newest=True only the newest
plane (byte 3 of the pixel's dword, as env_render_push lays the history out).  A constant image
is reproduced exactly, and pixels farther than 15 from the centre in either axis are copies.

Scores, from the engine's float32 outputs in float64: S_v = 1/2 (V - V')^2 and
S_pi = 1/2 sum_a (p_a - p'_a)^2, summed over a = 0, 1, ... in that order.  The paper scores the
logits; the C ABI exposes probabilities, so S_pi is bounded by 1 and saturates where the paper's
score keeps growing.

Map.  The 17 x 17 grid is interpolated bilinearly to 84 x 84: pixel (y, x) sits at grid
coordinate (y / 5, x / 5) clamped to 16 (rows and columns 80..83 repeat the last cell), i.e. cell
y // 5 with weight (y % 5) / 5 towards the next; float64, rounded once to float32.
"""
import numpy as np

H = W = 84
STRIDE, GRID = 5, 17
NC = GRID * GRID                # centres per state
RADIUS, SIGMA = 9, 3.0          # the blur
MASK_RADIUS = 15                # the mask is zero beyond
WHICH = {"v": 0, "pi": 1}       # ba3c_perturb_scores' `which`


def _weights():
    t = np.arange(-RADIUS, RADIUS + 1)
    g = np.exp(-t * t / (2 * SIGMA * SIGMA))
    w = np.rint(4096 * g / g.sum()).astype(np.int64)
    w[RADIUS] += 4096 - w.sum()
    return w


WEIGHTS = _weights()                                                        # int64 [19], Q12
MASK_Q = np.rint(256 * np.exp(-np.arange(MASK_RADIUS + 1) ** 2 / 50.0)).astype(np.int64)   # [16]


def centres():
    """int64 [289, 2]: (y, x) of centre 17 i + j."""
    i, j = np.divmod(np.arange(NC), GRID)
    return np.stack([STRIDE * i, STRIDE * j], axis=1)


def reflect(i, n=H):
    """Symmetric reflection of indices -n..2n-1 into 0..n-1."""
    i = np.asarray(i)
    return np.where(i < 0, -1 - i, np.where(i >= n, 2 * n - 1 - i, i))


def blur_q24(state):
    """uint8 [..., 84, 84, C] -> the blurred planes as exact Q24 integers (int64, same shape)."""
    x = np.asarray(state).astype(np.int64)
    taps = np.arange(-RADIUS, RADIUS + 1)
    h = sum(w * x[..., :, reflect(np.arange(W) + t), :] for w, t in zip(WEIGHTS, taps))
    return sum(w * h[..., reflect(np.arange(H) + t), :, :] for w, t in zip(WEIGHTS, taps))


def mask_q16(cy, cx):
    """int64 [84, 84]: the mask of the centre (cy, cx)."""
    def axis(c):
        d = np.abs(np.arange(H) - c)
        return np.where(d <= MASK_RADIUS, MASK_Q[np.minimum(d, MASK_RADIUS)], 0)
    return np.outer(axis(cy), axis(cx))


def perturb_numpy(state, newest=False):
    """state uint8 [n, 84, 84, 4] -> uint8 [n * 289, 84, 84, 4], the rule above."""
    state = np.asarray(state)
    assert state.dtype == np.uint8 and state.shape[1:] == (H, W, 4), state.shape
    p24 = state.astype(np.int64) << 24
    blur = blur_q24(state)
    out = np.empty((state.shape[0], NC) + state.shape[1:], np.uint8)
    for k, (cy, cx) in enumerate(centres()):
        m = mask_q16(cy, cx)[None, :, :, None]
        out[:, k] = (p24 * (65536 - m) + blur * m + (1 << 39)) >> 40
    if newest:
        out[..., :3] = state[:, None, :, :, :3]
    return out.reshape((-1,) + state.shape[1:])


def scores_numpy(probs0, value0, probs, value, which):
    """The outputs of n source states (probs0 [n, A], value0 [n]) and of their n * 289 perturbed
    states -> float64 [n, 17, 17]: S_v (which = 0) or S_pi (which = 1)."""
    n = len(value0)
    if which == 0:
        d = np.asarray(value0, np.float64)[:, None] - np.asarray(value, np.float64).reshape(n, NC)
        return (0.5 * d * d).reshape(n, GRID, GRID)
    assert which == 1
    p0 = np.asarray(probs0, np.float64)
    d = p0[:, None, :] - np.asarray(probs, np.float64).reshape(n, NC, p0.shape[1])
    acc = np.zeros((n, NC))
    for a in range(p0.shape[1]):
        acc += d[:, :, a] * d[:, :, a]
    return (0.5 * acc).reshape(n, GRID, GRID)


def upsample_numpy(grid):
    """float64 [n, 17, 17] -> float32 [n, 84, 84], the bilinear map above."""
    g = np.asarray(grid, np.float64)
    c0 = np.minimum(np.arange(H) // STRIDE, GRID - 1)
    c1 = np.minimum(c0 + 1, GRID - 1)
    t = np.where(np.arange(H) < STRIDE * (GRID - 1), (np.arange(H) % STRIDE) / float(STRIDE), 0.0)
    ty, tx = t[:, None], t[None, :]
    top = (1 - tx) * g[:, c0][:, :, c0] + tx * g[:, c0][:, :, c1]
    bot = (1 - tx) * g[:, c1][:, :, c0] + tx * g[:, c1][:, :, c1]
    return ((1 - ty) * top + ty * bot).astype(np.float32)
