"""Exact t-SNE (van der Maaten & Hinton 2008) of a set of states' fc1 features: the picture of
Mnih et al. 2015, Fig. 4.  This module states the whole rule in numpy float64 and is the oracle of
csrc/ba3c_tsne.h; `embed` is the device path.

Input.  X [N, D] float32, 8 <= N <= 8192, 1 <= D <= 2048; perplexity u, 1 <= u <= (N - 1) / 3.

Distances.  The column means are taken in float64 and rounded once to float32; Xc = X - mean in
float32 is what both sides use.  d_ij = max(0, |xc_i|^2 + |xc_j|^2 - 2 xc_i . xc_j), d_ii = 0,
evaluated here in float64.

Conditional affinities.  Per row i the precision beta_i at which
    p_{j|i} = e_j / sum_k e_k,  e_j = exp(-beta_i (d_ij - min_{k != i} d_ik)),  j != i
has Shannon entropy H = log(sum e) + beta sum(d' e) / sum(e) = log(u), by bisection: beta = 1;
evaluate H; stop where |H - log u| <= 1e-5 or after 100 updates; H too large: beta_min = beta and
beta doubles (no upper bound yet) or moves half way to beta_max; else beta_max = beta and beta
halves or moves half way to beta_min.  All in float64.

Joint affinities.  P = (P_c + P_c^T) / (2N) as float32, zero on the diagonal.

One iteration (`step_numpy`), sums in float64 over j != i:
    num_ij = 1 / (1 + |y_i - y_j|^2),  Z = sum_ij num_ij,
    a_i = sum_j p_ij num_ij (y_i - y_j),  r_i = sum_j num_ij^2 (y_i - y_j),
    grad_i = 4 (exag a_i - r_i / Z),
    G = G + 0.2 where (grad > 0) != (U > 0), else G * 0.8 (float32), floored at 0.01,
    U = float32(momentum U - lr G grad) (the expression in float64),  Y = Y + U (float32),
    KL = sum_ij p_ij log(max(p_ij, 1e-12) / num_ij) + log Z      (P itself, never exag P)
KL and grad belong to the Y the iteration started from.

Schedule (`run_numpy`, `embed`).  lr = 200; exag = 12 and momentum = 0.5 for iterations 0 .. 249,
then 1 and 0.8; Y is never re-centred.  Y0 = float32(1e-4 RandomState(seed).standard_normal((N, 2))),
U0 = 0, G0 = 1; with init="pca" Y0 is ba3c_amd/pca.py's start (`initial_pca_numpy`).  The KL trace holds iteration t's KL for every t with (t + 1) % kl_every == 0.
"""
import ctypes

import numpy as np

MIN_N, MAX_N, MAX_D = 8, 8192, 2048
ENTROPY_TOL, MAX_BISECT = 1e-5, 100
EXAG, EXAG_ITERS, MOMENTUM = 12.0, 250, (0.5, 0.8)
P_FLOOR = 1e-12


def center_numpy(x):
    """X float32 [N, D] -> Xc float32: minus the float64 column means rounded to float32."""
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 2 and MIN_N <= x.shape[0] <= MAX_N and 1 <= x.shape[1] <= MAX_D, x.shape
    return x - x.astype(np.float64).mean(axis=0).astype(np.float32)


def sqdist_numpy(x):
    """X float32 [N, D] -> d float64 [N, N]."""
    xc = center_numpy(x).astype(np.float64)
    n2 = (xc * xc).sum(axis=1)
    d = np.maximum(0.0, n2[:, None] + n2[None, :] - 2.0 * (xc @ xc.T))
    np.fill_diagonal(d, 0.0)
    return d


def check_perplexity(n, u):
    u = float(u)
    assert np.isfinite(u) and 1.0 <= u <= (n - 1) / 3.0, "perplexity %r outside [1, (N-1)/3]" % u
    return u


def row_entropy(dm, beta):
    """dm: a row's d - min without its own entry.  -> (H, e, sum e)."""
    e = np.exp(-beta * dm)
    s = e.sum()
    return np.log(s) + beta * (dm * e).sum() / s, e, s


def conditional_row_numpy(row, i, target):
    """One row of the bisection: row float64 [N] = d_i., target = log u.  -> (beta_i, the
    conditional row p_.|i float64 [N], zero at i)."""
    others = np.arange(row.shape[0]) != i
    dm = row[others] - row[others].min()
    b, lo, hi = 1.0, -np.inf, np.inf
    for it in range(MAX_BISECT + 1):
        h, e, s = row_entropy(dm, b)
        if abs(h - target) <= ENTROPY_TOL or it == MAX_BISECT:
            break
        if h > target:
            lo = b
            b = b * 2.0 if hi == np.inf else 0.5 * (b + hi)
        else:
            hi = b
            b = b * 0.5 if lo == -np.inf else 0.5 * (b + lo)
    out = np.zeros(row.shape[0])
    out[others] = e / s
    return b, out


def conditional_numpy(dist, perplexity):
    """dist [N, N] -> (beta float64 [N], P_c float64 [N, N])."""
    dist = np.asarray(dist, np.float64)
    n = dist.shape[0]
    target = np.log(check_perplexity(n, perplexity))
    beta, pc = np.ones(n), np.zeros((n, n))
    for i in range(n):
        beta[i], pc[i] = conditional_row_numpy(dist[i], i, target)
    return beta, pc


def affinities_numpy(dist, perplexity):
    """dist [N, N] -> (P float32 [N, N], beta float64 [N])."""
    beta, pc = conditional_numpy(dist, perplexity)
    return ((pc + pc.T) / (2.0 * pc.shape[0])).astype(np.float32), beta


def kl_grad_numpy(p, y):
    """P [N, N], Y [N, 2] -> (KL, a [N, 2], r [N, 2], Z), all float64: the pass of one iteration."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    diff = y[:, None, :] - y[None, :, :]
    num = 1.0 / (1.0 + (diff * diff).sum(axis=2))
    np.fill_diagonal(num, 0.0)
    z = num.sum(axis=1).sum()
    a = ((p * num)[:, :, None] * diff).sum(axis=1)
    r = ((num * num)[:, :, None] * diff).sum(axis=1)
    off = ~np.eye(p.shape[0], dtype=bool)
    kl = (p[off] * np.log(np.maximum(p[off], P_FLOOR) / num[off])).sum() + np.log(z)
    return kl, a, r, z


def step_numpy(p, y, vel, gains, exag, momentum, lr):
    """One iteration.  -> (Y, U, G float32 [N, 2], KL, grad float64 [N, 2])."""
    y, vel, gains = (np.asarray(v, np.float32) for v in (y, vel, gains))
    kl, a, r, z = kl_grad_numpy(p, y)
    grad = 4.0 * (float(exag) * a - r / z)
    flip = (grad > 0) != (vel > 0)
    g = np.maximum(np.where(flip, gains + np.float32(0.2), gains * np.float32(0.8)), np.float32(0.01))
    u = (float(momentum) * vel.astype(np.float64) - float(lr) * g.astype(np.float64) * grad).astype(np.float32)
    return y + u, u, g.astype(np.float32), kl, grad


def schedule(t):
    """-> (exag, momentum) of iteration t."""
    return (EXAG, MOMENTUM[0]) if t < EXAG_ITERS else (1.0, MOMENTUM[1])


def initial_numpy(n, seed):
    y = (1e-4 * np.random.RandomState(seed).standard_normal((n, 2))).astype(np.float32)
    return y, np.zeros((n, 2), np.float32), np.ones((n, 2), np.float32)


def initial_pca_numpy(x, seed=0, sweeps=32):
    """The PCA start of ba3c_amd/pca.py: Y0 from the first two principal-component scores of X, the
    first at standard deviation 1e-4; `initial_numpy`'s draw where X has no variance."""
    from . import pca
    fit = pca.fit_numpy(x, min(2, x.shape[1]), sweeps, seed)
    n = x.shape[0]
    return pca.y0_numpy(fit["scores"], fit["eigvals"][0], seed), np.zeros((n, 2), np.float32), np.ones((n, 2), np.float32)


def run_numpy(p, iters=1000, lr=200.0, seed=0, kl_every=50, state=None):
    """The schedule from Y0 (or from `state` = (Y, U, G, first iteration)) -> (Y, U, G, KL trace)."""
    y, vel, gains, t0 = state if state is not None else initial_numpy(p.shape[0], seed) + (0,)
    trace = []
    for t in range(t0, iters):
        y, vel, gains, kl, _ = step_numpy(p, y, vel, gains, *schedule(t), lr)
        if (t + 1) % kl_every == 0:
            trace.append(kl)
    return y, vel, gains, np.asarray(trace, np.float64)


# ---- the device path -------------------------------------------------------------------------

def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _workspace(x_or_n, d=1):
    import torch

    from . import _lib
    n = x_or_n if isinstance(x_or_n, int) else x_or_n.shape[0]
    size = int(_lib.load().ba3c_tsne_workspace_size(n, d))
    assert size > 0, "N = %d or D = %d outside the embedding's range" % (n, d)
    return torch.empty(size, dtype=torch.uint8, device="cuda")


def sqdist(x, work=None):
    """x float32 device [N, D] -> d float32 device [N, N] (ba3c_tsne_sqdist)."""
    import torch

    from . import _lib
    assert x.dtype == torch.float32 and x.is_cuda and x.dim() == 2 and x.is_contiguous()
    n, d = x.shape
    work = _workspace(n, d) if work is None else work
    dist = torch.empty(n, n, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ba3c_tsne_sqdist(_stream(), _ptr(x), n, d, _ptr(work), _ptr(dist)))
    return dist


def affinities(dist, perplexity, work=None):
    """dist float32 device [N, N] -> (P float32 device [N, N], beta float64 device [N])."""
    import torch

    from . import _lib
    assert dist.dtype == torch.float32 and dist.is_cuda and dist.is_contiguous()
    n = dist.shape[0]
    work = _workspace(n) if work is None else work
    beta = torch.empty(n, dtype=torch.float64, device=dist.device)
    p = torch.empty(n, n, dtype=torch.float32, device=dist.device)
    _lib.check(_lib.load().ba3c_tsne_affinities(_stream(), _ptr(dist), n, float(perplexity), _ptr(work),
                                                _ptr(beta), _ptr(p)))
    return p, beta


def step(p, y, vel, gains, exag, momentum, lr, work, kl_out=None):
    """One iteration in place on y, vel, gains (float32 device [N, 2]); kl_out: a float64 device
    element that receives the iteration's KL, or None."""
    from . import _lib
    _lib.check(_lib.load().ba3c_tsne_step(_stream(), _ptr(p), p.shape[0], _ptr(y), _ptr(vel), _ptr(gains),
                                          float(exag), float(momentum), float(lr), _ptr(work), _ptr(kl_out)))


def embed(x, perplexity=30, iters=1000, lr=200, seed=0, kl_every=50, init="random", pca_out=None):
    """x float32 device [N, D] -> (Y float32 device [N, 2], KL trace float64 numpy).  Three launches
    make P, then every iteration is two launches on the current stream; the host reads nothing
    until the trace is copied back at the end.  init="pca": Y0 comes from `pca.fit` on the device
    (over the seed's draw, which stays where X has no variance); a dict passed as pca_out receives
    that fit."""
    import torch
    n, d = x.shape
    check_perplexity(n, perplexity)
    assert iters >= 1 and kl_every >= 1 and init in ("random", "pca"), init
    if init == "pca":
        from . import pca
        work = pca._workspace(n, d)                  # one buffer serves both kernel families
    else:
        work = _workspace(n, d)
    p, _ = affinities(sqdist(x.contiguous(), work), perplexity, work)
    y, vel, gains = (torch.from_numpy(v).to(x.device) for v in initial_numpy(n, seed))
    if init == "pca":
        fit = pca.fit(x.contiguous(), min(2, d), seed=seed, y0=y, work=work)
        if pca_out is not None:
            pca_out.update(fit)
    trace = torch.zeros(max(1, iters // kl_every), dtype=torch.float64, device=x.device)
    for t in range(iters):
        slot = trace[(t + 1) // kl_every - 1:] if (t + 1) % kl_every == 0 else None
        step(p, y, vel, gains, *schedule(t), lr, work, slot)
    return y, trace[:iters // kl_every].cpu().numpy()
