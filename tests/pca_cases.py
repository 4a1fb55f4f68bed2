"""Inputs of tests/test_pca_rules.py and tests/test_gpu_pca.py and the float64 references they share.
crafted(n, d): scatter eigenvalues 64 * 4^-i, i < min(n - 1, d): an orthonormal, column-centred
U [n, r] times the scales times r rows of a rotation, plus a mean offset, rounded to float32.
relu_like(n, d): the same through a ReLU (more than half exact zeros) with four all-zero columns.
"""
import functools

import numpy as np

from ba3c_amd import pca as P
from ba3c_amd import tsne as T

# the tile edges 64 | 65 and 128 | 129 | 130 of D, the K-step seams of N, rank below m, D = 1
SHAPES = [(8, 1), (8, 33), (9, 8), (65, 33), (129, 64), (257, 130)]
CPU_ONLY_SHAPES = [(64, 200)]
RELU_SHAPE = (130, 40)
K = 4


def crafted(n, d):
    rs = np.random.RandomState(3000 + 7 * n + d)
    r = min(n - 1, d)
    a = rs.standard_normal((n, r))
    u, _ = np.linalg.qr(a - a.mean(axis=0))
    rot, _ = np.linalg.qr(rs.standard_normal((d, d)))
    return ((u * np.sqrt(64.0 * 4.0 ** -np.arange(r))) @ rot[:r] + rs.standard_normal(d)).astype(np.float32)


def relu_like(n, d):
    rs = np.random.RandomState(4000 + 7 * n + d)
    r = min(n - 1, d)
    u, _ = np.linalg.qr(rs.standard_normal((n, r)))
    rot, _ = np.linalg.qr(rs.standard_normal((d, d)))
    x = np.maximum(0.0, (u * np.sqrt(64.0 * 4.0 ** -np.arange(r))) @ rot[:r] - 0.05).astype(np.float32)
    x[:, [1, 5, d - 2, d - 1]] = 0
    return x


@functools.lru_cache(maxsize=None)
def case(n, d, relu=False):
    """-> dict, made once: x, xc (float64), C, eigh's eigenvalues and vectors (descending, after the
    sign rule), k = min(K, m), the oracle's fit, and the entrywise scatter bound."""
    x = relu_like(n, d) if relu else crafted(n, d)
    xc = T.center_numpy(x).astype(np.float64)
    c = xc.T @ xc
    lam, vec = np.linalg.eigh(c)
    lam, vec = lam[::-1], vec[:, ::-1]
    vec = vec * np.where(vec[np.abs(vec).argmax(axis=0), np.arange(d)] < 0.0, -1.0, 1.0)
    k = min(K, P.width(d))
    return {"x": x, "xc": xc, "c": c, "lam": lam, "vec": vec, "k": k, "fit": P.fit_numpy(x, k),
            "dc": 3.0 * 2.0 ** -22 * (np.abs(xc).T @ np.abs(xc))}


def gaps(lam, k):
    """The distance of each of the k leading eigenvalues to its nearest other eigenvalue."""
    lam = np.asarray(lam, np.float64)
    return np.array([np.abs(np.delete(lam, j) - lam[j]).min() if lam.size > 1 else lam[0] for j in range(k)])


def off_axis(v, ref):
    """|v - (ref . v) ref| per column: the part of v outside ref's direction."""
    return np.sqrt(((v - (ref * v).sum(axis=0) * ref) ** 2).sum(axis=0))
