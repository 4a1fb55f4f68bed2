"""tests/tsne_cases.py against ba3c_amd/tsne.py: the blocked oracle is step_numpy, the crafted P is a
joint distribution with exact zeros, and the oracle's own gradient is clear of zero at every size
tests/test_gpu_tsne.py steps (the share of unsure gains it tolerates must hold without a device)."""
import numpy as np
import pytest

import tsne_cases as C
from ba3c_amd import tsne as T


def oracle_made_p(n):
    rs = np.random.RandomState(n)
    x = rs.normal(size=(n, 6)).astype(np.float32)
    x[:, 0] += 4.0 * (np.arange(n) % 3)
    return T.affinities_numpy(T.sqdist_numpy(x), 20)[0]


@pytest.mark.parametrize("made", ["crafted", "oracle"])
@pytest.mark.parametrize("exag,momentum", [(12.0, 0.5), (1.0, 0.8), (12.0, 0.0)])
def test_the_chunked_step_is_step_numpy(made, exag, momentum):
    n = 257                                        # two blocks, the second of one row
    p, z = C.crafted_p(n)
    if made == "oracle":
        p = oracle_made_p(n)
    y, u, g = C.crafted_state(n, z)
    ref = T.step_numpy(p, y, u, g, exag, momentum, 200.0)
    got = C.step_numpy_chunked(p, y, u, g, exag, momentum, 200.0)
    for a, b in zip(got[:3], ref[:3]):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert abs(got[3] - ref[3]) <= 1e-13 * abs(ref[3])
    assert np.abs(got[4] - ref[4]).max() <= 1e-13 * np.abs(ref[4]).max()
    passed = C.kl_grad_chunked(p, y)
    again = C.step_numpy_chunked(p, y, u, g, exag, momentum, 200.0, passed)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    # every branch of the gains rule occurs: raised, lowered, and lowered to the floor
    assert (ref[2] > g).any() and ((ref[2] < g) & (ref[2] > 0.01)).any() and (ref[2] == np.float32(0.01)).any()


@pytest.mark.parametrize("n", [132, 257, 2052])
def test_the_crafted_p_is_a_joint_distribution_with_exact_zeros(n):
    p, z = C.crafted_p(n)
    assert p.dtype == np.float32 and p.shape == (n, n) and z.shape == (n, 2)
    assert np.array_equal(p, p.T) and p.min() >= 0 and not p.diagonal().any()
    assert abs(p.astype(np.float64).sum() - 1) <= 1e-6
    off = ~np.eye(n, dtype=bool)
    assert (p[off] == 0).any() and (p[off] > 0).any()
    assert (p.max(axis=1) > 0).all()               # no row is empty


@pytest.mark.parametrize("n", C.STEP_N + (C.LIMIT_N,))
def test_the_oracle_gradient_is_clear_of_zero(n):
    p, (y, u, g), passed = C.crafted_case(n)
    for exag in [e for m, e in C.STEP_CASES if m == n]:
        grad = C.step_numpy_chunked(p, y, u, g, exag, 0.5, 200.0, passed)[4]
        unsure = C.unsure(grad, C.TOL_STEP)
        print("n=%d exag=%g: %d of %d unsure" % (n, exag, unsure.sum(), unsure.size))
        assert unsure.mean() < 0.01
