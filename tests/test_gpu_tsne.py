"""The t-SNE kernels on the MI355X, each stage against ba3c_amd/tsne.py on the same inputs (so the
errors of a stage do not reach the next one), the embedding end to end, and Ba3cEngine.features.

The bounds are four times the worst figure measured over the cases of each test (DESIGN.md
section 23.1 lists the figures); every test prints its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch

from ba3c_amd import tsne as T
from test_gpu_parity import case, dev, engine

pytestmark = pytest.mark.gpu
TOL_D = 4 * 2.208e-7      # |d - d64| / (|xc_i|^2 + |xc_j|^2); the split's model allows 3 * 2^-22 = 7e-7 per product
TOL_P = 4 * 9.025e-8      # |P - P64| / max P64
TOL_STEP = 4 * 8.579e-8   # normwise, per array of the step (and the KL, relative)
KL_MARGIN = 0.207         # the spread of the oracle's final KL over the seeds 0 .. 4 of Y0 on test_end_to_end's P


def clusters(n, d, sep=4.0, seed=0):
    """Three Gaussian clusters whose centres are `sep` standard deviations apart along three axes of
    a shifted frame (the centring has work to do), rows 1 and n - 2 exact copies of rows 0 and n - 1."""
    rs = np.random.RandomState(seed + n + d)
    x = rs.normal(size=(n, d)) + 3.0
    x[:, 0] += sep * (np.arange(n) % 3)
    x = x.astype(np.float32)
    x[1], x[n - 2] = x[0], x[n - 1]
    return x


@functools.lru_cache(maxsize=None)
def oracle_p(n, u):
    d = T.sqdist_numpy(clusters(n, 16)).astype(np.float32)
    return (d,) + T.affinities_numpy(d, u)


@functools.lru_cache(maxsize=None)
def oracle_state(n):
    """(P, (Y, U, G) after 30 iterations of run_numpy)."""
    p = oracle_p(n, 5 if n < 100 else 30)[1]
    return p, T.run_numpy(p, iters=30)[:3]


@pytest.mark.parametrize("n,d", [(8, 1), (65, 33), (129, 128), (257, 512)])
def test_distances(n, d):
    x = clusters(n, d)
    got = T.sqdist(dev(x)).cpu().numpy()
    ref, n2 = T.sqdist_numpy(x), (T.center_numpy(x).astype(np.float64) ** 2).sum(axis=1)
    err = np.abs(got - ref) / np.maximum(n2[:, None] + n2[None, :], 1e-300)
    print("sqdist n=%d d=%d: worst %.3e of |xc_i|^2 + |xc_j|^2" % (n, d, err.max()))
    assert np.array_equal(x[0], x[1]) and np.array_equal(x[n - 1], x[n - 2])     # d = 0 off the diagonal occurs
    assert not got.diagonal().any() and np.array_equal(got, got.T) and got.min() >= 0
    assert err.max() <= TOL_D


@pytest.mark.parametrize("n,u", [(8, 2), (65, 5), (257, 30), (1000, 50)])
def test_affinities(n, u):
    d, ref, _ = oracle_p(n, u)
    p, beta = T.affinities(dev(d), u)
    p, beta = p.cpu().numpy(), beta.cpu().numpy()
    dm = np.where(np.eye(n, dtype=bool), np.inf, d.astype(np.float64))
    e = np.exp(-beta[:, None] * (dm - dm.min(axis=1, keepdims=True)))
    pc = e / e.sum(axis=1, keepdims=True)
    perp = np.exp(-(pc * np.log(np.where(pc > 0, pc, 1.0))).sum(axis=1))
    err = np.abs(p - ref).max() / ref.max()
    print("affinities n=%d u=%g: perplexity off by %.3e, P off by %.3e of max P" % (n, u, np.abs(perp / u - 1).max(), err))
    assert np.abs(perp / u - 1).max() <= 1e-4
    assert np.array_equal(p, p.T) and not p.diagonal().any() and p.min() >= 0
    assert err <= TOL_P


@pytest.mark.parametrize("exag", [12.0, 1.0])
@pytest.mark.parametrize("n", [65, 128, 257])          # 128: the 16-byte lane loads of a row of P
def test_one_step(n, exag):
    p, (y0, u0, g0) = oracle_state(n)
    y1, u1, g1, kl, grad = T.step_numpy(p, y0, u0, g0, exag, 0.5, 200.0)
    unsure = np.abs(grad) <= TOL_STEP * np.abs(grad).max()      # the sign of grad is within the noise
    assert unsure.mean() < 0.01
    y, u, g = dev(y0), dev(u0), dev(g0)
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    T.step(dev(p), y, u, g, exag, 0.5, 200.0, T._workspace(n), out)
    y, u, g, out = (t.cpu().numpy() for t in (y, u, g, out))
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    print("step n=%d exag=%g: Y %.3e U %.3e KL %.3e, %d of %d gains unsure"
          % (n, exag, rel(y, y1), rel(u, u1), abs(out[0] - kl) / abs(kl), unsure.sum(), unsure.size))
    assert np.array_equal(g[~unsure], g1[~unsure]) and out[1] == 0
    assert rel(u, u1) <= TOL_STEP and rel(y, y1) <= TOL_STEP and abs(out[0] - kl) <= TOL_STEP * abs(kl)


def test_end_to_end():
    x = np.random.RandomState(7).normal(size=(192, 128)).astype(np.float32)
    x[:, 0] += 10.0 * (np.arange(192) // 64)
    y, trace = T.embed(dev(x), perplexity=20, iters=500, kl_every=50)
    y = y.cpu().numpy().astype(np.float64)
    p, _ = T.affinities_numpy(T.sqdist_numpy(x), 20)
    ref = T.run_numpy(p, iters=500)[3][-1]
    d = ((y[:, None] - y[None]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    near = np.argsort(d, axis=1)[:, :5]
    print("end to end: final KL %.4f, the oracle's %.4f" % (trace[-1], ref))
    assert np.array_equal(near // 64, np.repeat(np.arange(192)[:, None] // 64, 5, axis=1))
    assert trace.shape == (10,) and np.isfinite(trace).all() and trace[-1] <= ref + KL_MARGIN


@pytest.mark.parametrize("B", [3, 5])
def test_features_are_the_forward_workspace(B):
    params, state, _, _, _ = case(90 + B, B)
    eng = engine(max_batch=4)
    eng.load_params(params)
    got = eng.features(dev(state))
    assert got.shape == (B, 128) and got.dtype == torch.float32 and got.any()
    for first in range(0, B, 4):
        b = min(4, B - first)
        eng.forward(dev(state[first:first + b]))
        assert torch.equal(got[first:first + b].reshape(-1), eng.workspace_tensor("h", b, train=False))
