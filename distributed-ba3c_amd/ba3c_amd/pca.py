"""The leading principal components of a set of states' fc1 features: the standard start of a t-SNE
map (Kobak & Berens 2019) and the linear picture one looks at before trusting it.  This module
states the whole rule in numpy float64 and is the oracle of csrc/ba3c_pca.h; `scatter`,
`components`, `project` and `fit` are the device path.

Input.  X [N, D] float32, N and D as for t-SNE (8 <= N <= 8192, 1 <= D <= 2048); k components,
1 <= k <= m = min(8, D); `sweeps` in 1 .. 256 (default 32).

Centring and scatter.  Xc = tsne.center_numpy(X), the float32 Xc of the distances.
C = Xc^T Xc [D, D] in float64, not divided by N.

Block iteration.  Q0 = RandomState(seed).standard_normal((D, m)), drawn on the host by both sides;
Q = orth(Q0), then `sweeps` times Q = orth(C Q).  orth is modified Gram-Schmidt over the columns in
order: column j loses its projection r = q_i . z_j onto each earlier column i in turn
(z_j = z_j - r q_i, r from the current z_j), that pass over i = 0 .. j - 1 runs twice, and z_j is
divided by its norm.  A column whose norm after the two passes is 0, or at most 2^-40 of its norm
before them, becomes exactly zero instead: a rank-deficient C (N - 1 < m, dead ReLU columns) gives
zero columns and never a NaN.  A zero column stays zero and touches no other column.

Rayleigh-Ritz.  Z = C Q, G = Q^T Z, H = (G + G^T) / 2.  H [m, m] is diagonalised by cyclic Jacobi:
JACOBI_SWEEPS = 12 sweeps over the pairs (p, q), p < q, in the order (0, 1), (0, 2) .. (0, m - 1),
(1, 2) ..; a pair with h_pq = 0 is skipped, otherwise theta = (h_qq - h_pp) / (2 h_pq),
t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c, and columns then
rows p, q of H and columns p, q of W (W = I at the start) become (c a_p - s a_q, s a_p + c a_q).
The eigenvalues are H's diagonal, ordered descending by a stable sort; V = Q W in that order; each
vector is flipped so that its first component of largest magnitude is positive.

Outputs for the k leading pairs.  components float32 [k, D]; eigvals float64 [k];
ratio = eigvals / trace(C) (0 where the trace is 0); resid_j = |C v_j - l_j v_j| / l_1 (0 where
l_1 <= 0; the device forms C V as Z W), which tells the caller whether `sweeps` sufficed;
scores = Xc components^T, float32 [N, k], summed in float64 from the float32 components.

t-SNE start.  Y0 = float32(1e-4 * scores[:, :2] / sqrt(l_1 / N)): the first column has standard
deviation 1e-4.  With k = 1 (D = 1 allows no other) the second column is zero; with l_1 <= 0
(C = 0: all rows equal) Y0 is tsne.initial_numpy's draw.
"""
import ctypes

import numpy as np

from . import tsne

M, MAX_SWEEPS, JACOBI_SWEEPS = 8, 256, 12
ZERO_COLUMN = 2.0 ** -40
RESID_WARN = 1e-3


def width(d):
    return min(M, d)


def check(d, k, sweeps=1):
    assert 1 <= d <= tsne.MAX_D and 1 <= k <= width(d), "k = %r outside [1, min(8, D)]" % k
    assert 1 <= sweeps <= MAX_SWEEPS, "sweeps = %r outside [1, 256]" % sweeps


def scatter_numpy(x):
    """X float32 [N, D] -> C float64 [D, D]."""
    xc = tsne.center_numpy(x).astype(np.float64)
    return xc.T @ xc


def q0_numpy(d, seed=0):
    return np.random.RandomState(seed).standard_normal((d, width(d)))


def orth_numpy(z):
    q = np.array(z, np.float64)
    for j in range(q.shape[1]):
        before = np.sqrt(q[:, j] @ q[:, j])
        for _ in range(2):
            for i in range(j):
                q[:, j] -= (q[:, i] @ q[:, j]) * q[:, i]
        after = np.sqrt(q[:, j] @ q[:, j])
        q[:, j] = 0.0 if after == 0.0 or after <= ZERO_COLUMN * before else q[:, j] / after
    return q


def jacobi_numpy(h):
    """Symmetric H [m, m] -> (its diagonal after the sweeps, W)."""
    h = np.array(h, np.float64)
    m = h.shape[0]
    w = np.eye(m)
    rot = lambda a, b, c, s: (c * a - s * b, s * a + c * b)
    with np.errstate(over="ignore", divide="ignore"):
        for _ in range(JACOBI_SWEEPS):
            for p in range(m - 1):
                for q in range(p + 1, m):
                    if h[p, q] == 0.0:
                        continue
                    theta = (h[q, q] - h[p, p]) / (2.0 * h[p, q])
                    t = np.copysign(1.0, theta) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    h[:, p], h[:, q] = rot(h[:, p].copy(), h[:, q].copy(), c, s)
                    w[:, p], w[:, q] = rot(w[:, p].copy(), w[:, q].copy(), c, s)
                    h[p, :], h[q, :] = rot(h[p, :].copy(), h[q, :].copy(), c, s)
    return np.diag(h).copy(), w


def components_numpy(c, k=2, sweeps=32, seed=0, q0=None):
    """C [D, D] -> dict of components float32 [k, D], eigvals, ratio, resid float64 [k] and the
    float64 vectors v [D, k]."""
    c = np.asarray(c, np.float64)
    d = c.shape[0]
    check(d, k, sweeps)
    q = orth_numpy(q0_numpy(d, seed) if q0 is None else q0)
    for _ in range(sweeps):
        q = orth_numpy(c @ q)
    g = q.T @ (c @ q)
    eig, w = jacobi_numpy((g + g.T) / 2.0)
    order = np.argsort(-eig, kind="stable")[:k]
    v, eig = q @ w[:, order], eig[order]
    lead = v[np.abs(v).argmax(axis=0), np.arange(k)]
    v = v * np.where(lead < 0.0, -1.0, 1.0)
    trace = np.trace(c)
    resid = np.sqrt(((c @ v - eig * v) ** 2).sum(axis=0)) / eig[0] if eig[0] > 0.0 else np.zeros(k)
    return {"components": v.T.astype(np.float32), "eigvals": eig, "v": v, "resid": resid,
            "ratio": eig / trace if trace > 0.0 else np.zeros(k)}


def project_numpy(x, components):
    """-> scores float32 [N, k]."""
    xc = tsne.center_numpy(x).astype(np.float64)
    return (xc @ np.asarray(components, np.float32).astype(np.float64).T).astype(np.float32)


def y0_numpy(scores, l1, seed=0):
    """The t-SNE start from float32 scores [N, k] and l_1."""
    n = scores.shape[0]
    if not l1 > 0.0:
        return tsne.initial_numpy(n, seed)[0]
    y = np.zeros((n, 2), np.float32)
    cols = min(2, scores.shape[1])
    y[:, :cols] = (1e-4 * scores[:, :cols].astype(np.float64) / np.sqrt(l1 / n)).astype(np.float32)
    return y


def fit_numpy(x, k=2, sweeps=32, seed=0):
    out = components_numpy(scatter_numpy(x), k, sweeps, seed)
    out["scores"] = project_numpy(x, out["components"])
    return out


# ---- the device path -------------------------------------------------------------------------

def _workspace(n, d):
    import torch

    from . import _lib
    size = int(_lib.load().ba3c_pca_workspace_size(n, d))
    assert size > 0, "N = %d or D = %d outside the range" % (n, d)
    return torch.empty(size, dtype=torch.uint8, device="cuda")


def _checked(x):
    import torch
    assert x.dtype == torch.float32 and x.is_cuda and x.dim() == 2 and x.is_contiguous()
    return x.shape


def scatter(x, work=None):
    """x float32 device [N, D] -> C float64 device [D, D] (ba3c_pca_scatter)."""
    import torch

    from . import _lib
    n, d = _checked(x)
    work = _workspace(n, d) if work is None else work
    c = torch.empty(d, d, dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().ba3c_pca_scatter(tsne._stream(), tsne._ptr(x), n, d, tsne._ptr(work), tsne._ptr(c)))
    return c


def components(c, k=2, sweeps=32, seed=0, q0=None, work=None):
    """c float64 device [D, D] -> (components float32 [k, D], eigvals, ratio, resid float64 [k]),
    device tensors (ba3c_pca_components).  Q0 is drawn on the host, as the oracle draws it."""
    import torch

    from . import _lib
    d = c.shape[0]
    check(d, k, sweeps)
    assert c.dtype == torch.float64 and c.is_cuda and c.is_contiguous() and c.shape == (d, d)
    if not torch.is_tensor(q0):
        q0 = torch.from_numpy(np.ascontiguousarray(q0_numpy(d, seed) if q0 is None else q0, np.float64)).to(c.device)
    assert q0.dtype == torch.float64 and q0.is_cuda and q0.is_contiguous() and q0.shape == (d, width(d))
    work = _workspace(tsne.MIN_N, d) if work is None else work
    comps = torch.empty(k, d, dtype=torch.float32, device=c.device)
    eig, ratio, resid = (torch.empty(k, dtype=torch.float64, device=c.device) for _ in range(3))
    _lib.check(_lib.load().ba3c_pca_components(tsne._stream(), tsne._ptr(c), d, None, tsne._ptr(q0), k, sweeps,
                                               tsne._ptr(work), tsne._ptr(comps), tsne._ptr(eig), tsne._ptr(ratio),
                                               tsne._ptr(resid)))
    return comps, eig, ratio, resid


def project(x, comps, eigvals, y0=None, work=None):
    """x float32 device [N, D], comps float32 device [k, D] -> scores float32 device [N, k]; y0
    (float32 device [N, 2], filled with the fall-back draw) is overwritten where eigvals[0] > 0."""
    import torch

    from . import _lib
    n, d = _checked(x)
    k = comps.shape[0]
    assert comps.dtype == torch.float32 and comps.is_contiguous() and comps.shape == (k, d)
    work = _workspace(n, d) if work is None else work
    scores = torch.empty(n, k, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ba3c_pca_project(tsne._stream(), tsne._ptr(x), n, d, tsne._ptr(comps), k,
                                            tsne._ptr(eigvals), tsne._ptr(work), tsne._ptr(scores), tsne._ptr(y0)))
    return scores


def fit(x, k=2, sweeps=32, seed=0, y0=None, work=None):
    """x float32 device [N, D] -> dict of scores, components, eigvals, ratio, resid: device tensors,
    the host reads nothing.  y0: see `project`."""
    n, d = _checked(x)
    work = _workspace(n, d) if work is None else work
    comps, eig, ratio, resid = components(scatter(x, work), k, sweeps, seed, work=work)
    return {"scores": project(x, comps, eig, y0, work), "components": comps, "eigvals": eig, "ratio": ratio,
            "resid": resid}
