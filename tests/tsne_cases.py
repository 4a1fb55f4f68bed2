"""Inputs and a blocked oracle for the t-SNE iteration at sizes where ba3c_amd/tsne.py's own
helpers cost too much on the host: affinities_numpy bisects every row in Python, and step_numpy
forms [N, N, 2] float64 arrays (1 GB at N = 8192).  Nothing here is imported from anything compiled.

crafted_p makes a valid joint P without a bisection; crafted_state a (Y, U, G) that takes every
branch of the gains rule; step_numpy_chunked states step_numpy's rule in blocks of 256 rows.
tests/test_tsne_cases.py holds the three to tsne.py; tests/test_gpu_tsne.py uses them.
"""
import functools

import numpy as np

from ba3c_amd import tsne as T

CHUNK = 256
CENTRES = np.array([[0.0, 0.0], [24.0, 0.0], [0.0, 24.0]])
TOL_STEP = 4 * 8.579e-8      # tests/test_gpu_tsne.py's bound on a step (it asserts that the two agree)
# the crafted step cases of tests/test_gpu_tsne.py: every N at both exaggerations, the limit at one
STEP_N, LIMIT_N = (132, 260, 2049, 2052, 4098, 4100), T.MAX_N
STEP_CASES = [(n, exag) for n in STEP_N for exag in (12.0, 1.0)] + [(LIMIT_N, 12.0)]
GAINS = np.array([0.0101, 0.8, 1.0, 1.2, 2.6], np.float32)      # 0.0101 * 0.8 falls under the floor of 0.01


def crafted_points(n, seed=0):
    """z float64 [N, 2]: three unit Gaussian clusters, point i in cluster i % 3."""
    rs = np.random.RandomState(1000 + seed + n)
    return rs.standard_normal((n, 2)) + CENTRES[np.arange(n) % 3]


def crafted_p(n, seed=0):
    """-> (P float32 [N, N], z): w = exp(-|z_i - z_j|^2 / 2) with a zero diagonal, rows normalised,
    P = (w + w^T) / 2N.  Pairs of different clusters are 24 apart: exp(-288) / 2N is exactly 0 in
    float32, so P holds exact zeros off the diagonal (the kernel's p log(max(p, 1e-12) t) at p = 0)."""
    z = crafted_points(n, seed)
    n2 = (z * z).sum(axis=1)
    w = np.maximum(0.0, n2[:, None] + n2[None, :] - 2.0 * (z @ z.T))
    w *= -0.5
    np.exp(w, out=w)
    np.fill_diagonal(w, 0.0)
    w /= w.sum(axis=1, keepdims=True)
    return ((w + w.T) / (2.0 * n)).astype(np.float32), z


def crafted_state(n, z, seed=0):
    """-> (Y, U, G) float32 [N, 2]: Y = 0.5 z + noise of 0.1, U of both signs of order 0.05, G drawn
    from GAINS."""
    rs = np.random.RandomState(2000 + seed + n)
    y = (0.5 * z + 0.1 * rs.standard_normal((n, 2))).astype(np.float32)
    u = (0.05 * rs.standard_normal((n, 2))).astype(np.float32)
    return y, u, GAINS[rs.randint(0, len(GAINS), size=(n, 2))]


def crafted_dist(z):
    """z [N, 2] -> d float32 [N, N] = |z_i - z_j|^2, from the differences in blocks: symmetric bit for
    bit with a zero diagonal, which a Gram-matrix form would not promise."""
    z = np.asarray(z, np.float64)
    d = np.empty((z.shape[0],) * 2, np.float32)
    for i0 in range(0, z.shape[0], CHUNK):
        diff = z[i0:i0 + CHUNK, None, :] - z[None, :, :]
        d[i0:i0 + CHUNK] = (diff * diff).sum(axis=2)
    return d


def kl_grad_chunked(p, y):
    """tsne.kl_grad_numpy in blocks of CHUNK rows: -> (KL, a [N, 2], r [N, 2], Z, sum_ij |p_ij
    log(max(p_ij, 1e-12) / num_ij)|), all float64; the last is what kl_bound wants."""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    a, r, zrow, klrow, klabs = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n), np.zeros(n), np.zeros(n)
    for i0 in range(0, n, CHUNK):
        i1 = min(n, i0 + CHUNK)
        pc = np.asarray(p[i0:i1], np.float64)
        own = np.arange(i0, i1)[:, None] == np.arange(n)[None, :]
        diff = y[i0:i1, None, :] - y[None, :, :]
        num = 1.0 / (1.0 + (diff * diff).sum(axis=2))
        num[own] = 0.0
        zrow[i0:i1] = num.sum(axis=1)
        a[i0:i1] = ((pc * num)[:, :, None] * diff).sum(axis=1)
        r[i0:i1] = ((num * num)[:, :, None] * diff).sum(axis=1)
        # p_ii = 0: the own pair's term is 0 log(1e-12 / 1) = 0
        term = pc * np.log(np.maximum(pc, T.P_FLOOR) / np.where(own, 1.0, num))
        klrow[i0:i1], klabs[i0:i1] = term.sum(axis=1), np.abs(term).sum(axis=1)
    z = zrow.sum()
    return klrow.sum() + np.log(z), a, r, z, klabs.sum()


def kl_bound(passed):
    """The absolute error that the fp32 terms of csrc/ba3c_tsne.h's tsne_pair allow in a step's KL,
    from the oracle's own figures (passed = kl_grad_chunked(p, y)).  With u = 2^-24, the relative error
    of one rounding, and L = log(max(p, 1e-12) t), t = 1 + |y_i - y_j|^2:
      t:  dx, dy (1 each, squared: 2), dx dx and dy dy (1), their sum (1), 1 + (1): 5 u relative;
      the argument max(p, 1e-12) t: 1 more, so L is off by 6 u ABSOLUTE, the term p L by 6 u p;
      logf is the hardware's log2 (1 ulp = 2 u of |log2|, hence 2 u |L|) times ln 2 in two
      floats (1), p L (1), the fp32 sum of a lane load's four terms (3): 7 u |p L|;
      Z: q = rcp(t) is t's 5 u plus 1 ulp (2), the sum of four (3): 10 u relative, so log Z is off by
      10 u absolute (the float64 sums and the float64 log do not count).
    -> u (7 sum |p L| + 6 sum p + 10), sum p = 1.  Relative to the KL ITSELF the same error is large
    where the embedding fits: KL = sum p L + log Z is then the small difference of two numbers of the
    size of log(N^2) (0.22 from -14.8 and 15.0 at N = 4100), which is why the crafted cases take
    this bound and not a share of |KL|."""
    return 2.0 ** -24 * (7.0 * passed[4] + 6.0 + 10.0)


def step_numpy_chunked(p, y, vel, gains, exag, momentum, lr, passed=None):
    """tsne.step_numpy with the pass over the pairs in blocks: -> (Y, U, G float32 [N, 2], KL, grad
    float64 [N, 2]).  `passed`: a kl_grad_chunked(p, y) made earlier (it does not depend on exag)."""
    y, vel, gains = (np.asarray(v, np.float32) for v in (y, vel, gains))
    kl, a, r, z = (kl_grad_chunked(p, y) if passed is None else passed)[:4]
    grad = 4.0 * (float(exag) * a - r / z)
    flip = (grad > 0) != (vel > 0)
    g = np.maximum(np.where(flip, gains + np.float32(0.2), gains * np.float32(0.8)), np.float32(0.01))
    u = (float(momentum) * vel.astype(np.float64) - float(lr) * g.astype(np.float64) * grad).astype(np.float32)
    return y + u, u, g.astype(np.float32), kl, grad


@functools.lru_cache(maxsize=None)
def crafted_case(n):
    """-> (P, (Y, U, G), kl_grad_chunked(P, Y)) of the crafted step case at N = n, made once."""
    p, z = crafted_p(n)
    state = crafted_state(n, z)
    return p, state, kl_grad_chunked(p, state[0])


def unsure(grad, tol):
    """The entries of the oracle's gradient whose sign is within `tol` of the largest entry."""
    return np.abs(grad) <= tol * np.abs(grad).max()
