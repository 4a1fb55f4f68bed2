"""The t-SNE rule of ba3c_amd/tsne.py on its own: the perplexity of every conditional row, the
properties of the joint P, and step_numpy's gradient against the finite difference of its own KL."""
import numpy as np
import pytest

from ba3c_amd import tsne as T


@pytest.mark.parametrize("n,u", [(8, 2), (50, 10)])
def test_affinities_have_the_perplexity_and_p_is_a_joint_distribution(n, u):
    d = T.sqdist_numpy(np.random.RandomState(n).normal(size=(n, 7)).astype(np.float32))
    assert np.array_equal(d, d.T) and not d.diagonal().any() and d.min() >= 0
    beta, pc = T.conditional_numpy(d, u)
    h = -(pc * np.log(np.where(pc > 0, pc, 1.0))).sum(axis=1)
    assert np.abs(np.exp(h) / u - 1).max() <= 1e-4 and (beta > 0).all()
    p, beta2 = T.affinities_numpy(d, u)
    assert p.dtype == np.float32 and np.array_equal(beta, beta2)
    assert np.array_equal(p, p.T) and p.min() >= 0 and not p.diagonal().any()
    assert abs(p.astype(np.float64).sum() - 1) <= 1e-6


def test_the_gradient_is_the_finite_difference_of_the_kl():
    n, rs = 12, np.random.RandomState(3)
    p, _ = T.affinities_numpy(T.sqdist_numpy(rs.normal(size=(n, 4)).astype(np.float32)), 3)
    y = rs.normal(size=(n, 2)).astype(np.float32)
    zeros = np.zeros((n, 2), np.float32)
    _, _, _, kl, grad = T.step_numpy(p, y, zeros, zeros + 1, 1.0, 0.5, 200.0)
    assert kl == T.kl_grad_numpy(p, y)[0] and kl > 0
    fd, eps = np.zeros((n, 2)), 1e-5
    for i in range(n):
        for c in range(2):
            e = np.zeros((n, 2))
            e[i, c] = eps
            fd[i, c] = (T.kl_grad_numpy(p, y + e)[0] - T.kl_grad_numpy(p, y - e)[0]) / (2 * eps)
    assert np.abs(grad - fd).max() <= 1e-5 * np.abs(fd).max()


def test_the_schedule_and_the_trace():
    assert T.schedule(249) == (12.0, 0.5) and T.schedule(250) == (1.0, 0.8)
    p, _ = T.affinities_numpy(T.sqdist_numpy(np.random.RandomState(0).normal(size=(9, 3)).astype(np.float32)), 2)
    y, u, g, trace = T.run_numpy(p, iters=7, kl_every=3)
    assert trace.shape == (2,) and y.dtype == u.dtype == g.dtype == np.float32 and g.min() >= 0.01
    y2, u2, g2, trace2 = T.run_numpy(p, iters=7, kl_every=3, state=T.run_numpy(p, iters=4, kl_every=3)[:3] + (4,))
    assert np.array_equal(y, y2) and np.array_equal(g, g2) and trace2[-1] == trace[-1]
