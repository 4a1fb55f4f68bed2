"""csrc/ba3c_pca.h against ba3c_amd/pca.py and numpy.linalg.eigh, each stage from the oracle's own
inputs (tests/pca_cases.py).  Every bound is computed from the float64 reference alone; run with -s
for the measured figures.

The components are float32, so where the issue's float64 bound on a vector (64 D 2^-53 l_1 / gap_j)
meets them it carries the rounding of that format, 2^-24, on top; the eigenvalues and residuals are
float64 and are held to the backward error itself."""
import numpy as np
import pytest
import torch

import pca_cases as PC
from ba3c_amd import pca as P
from ba3c_amd import tsne as T

pytestmark = pytest.mark.gpu

CASES = [(n, d, False) for n, d in PC.SHAPES] + [PC.RELU_SHAPE + (True,)]
# (33, 8): the smallest N of two row chunks (a chunk is 32 rows while 32-row chunks stay under 256
# workgroups); (289, 520): 45 tile pairs, 5 chunks of two K-steps each
SCATTER_CASES = CASES + [(33, 8, False), (289, 520, False)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(fit):
    return {k: v.cpu().numpy() for k, v in fit.items()}


@pytest.mark.parametrize("n,d,relu", SCATTER_CASES)
def test_scatter(n, d, relu):
    """|C - C64|_ij <= 3 * 2^-22 sum_n |xc_ni| |xc_nj| (the split's per-product model); C symmetric
    bit for bit; scatter(X 2^s) == scatter(X) 2^2s bit for bit at s = +40 and -40."""
    cs = PC.case(n, d, relu)
    got = P.scatter(dev(cs["x"])).cpu().numpy()
    worst = (np.abs(got - cs["c"]) / np.maximum(cs["dc"], 1e-300)).max()
    print("scatter n=%d d=%d relu=%d: worst %.3f of the model bound" % (n, d, relu, worst))
    assert got.dtype == np.float64 and np.array_equal(got, got.T)
    assert (np.abs(got - cs["c"]) <= cs["dc"]).all()
    for s in (40, -40):
        scaled = P.scatter(dev(cs["x"] * np.float32(2.0 ** s))).cpu().numpy()
        assert np.array_equal(scaled, got * 4.0 ** s), s


@pytest.mark.parametrize("n,d,relu", CASES)
def test_components_from_the_oracles_scatter(n, d, relu):
    """Both sides in float64 on one C from one Q0: only the summation order differs."""
    cs = PC.case(n, d, relu)
    k, ref, back = cs["k"], cs["fit"], 64 * d * 2.0 ** -53
    comps, eig, ratio, resid = (v.cpu().numpy() for v in P.components(dev(cs["c"]), k))
    v = comps.T.astype(np.float64)
    off, bound = PC.off_axis(v, ref["v"]), back * cs["lam"][0] / PC.gaps(cs["lam"], k)
    print("components n=%d d=%d relu=%d: eigenvalues %.2e of l_1, vectors %s (float32: 6e-8), resid %s" %
          (n, d, relu, np.abs(eig - ref["eigvals"]).max() / cs["lam"][0], off, resid))
    assert np.abs(eig - ref["eigvals"]).max() <= back * cs["lam"][0]
    assert (off <= bound + 2.0 ** -24).all() and (np.abs(v - ref["v"]) <= bound + 2.0 ** -24 * np.abs(ref["v"])).all()
    assert ((v * ref["v"]).sum(axis=0) > 0).all()
    assert resid.max() <= back and np.abs(ratio - ref["ratio"]).max() <= back


def test_rank_deficiency():
    """(8, 33) has rank 7 < m = 8: the eighth eigenvalue is 0 within the backward error and every
    output is finite."""
    cs = PC.case(8, 33)
    out = [v.cpu().numpy() for v in P.components(dev(cs["c"]), 8)]
    print("rank 7 of 8: eigenvalues", out[1])
    assert all(np.isfinite(v).all() for v in out)
    assert abs(out[1][7]) <= 64 * 33 * 2.0 ** -53 * cs["lam"][0] and out[3][7] <= 64 * 33 * 2.0 ** -53


@pytest.mark.parametrize("n,d,relu", CASES)
def test_fit_end_to_end(n, d, relu):
    """fit(x) against eigh of the float64 C: each vector within 2 |dC|_F / gap_j, dC the scatter's
    entrywise model bound."""
    cs = PC.case(n, d, relu)
    k = cs["k"]
    x = dev(cs["x"])
    fit = host(P.fit(x, k))
    bound = 2.0 * np.linalg.norm(cs["dc"]) / PC.gaps(cs["lam"], k)
    off = PC.off_axis(fit["components"].T.astype(np.float64), cs["vec"][:, :k])
    print("fit n=%d d=%d relu=%d: vectors %s of %s, eigenvalues %.2e of l_1, resid %.1e" %
          (n, d, relu, off, bound, np.abs(fit["eigvals"] - cs["lam"][:k]).max() / cs["lam"][0], fit["resid"].max()))
    assert (off <= bound).all() and ((fit["components"].T * cs["vec"][:, :k]).sum(axis=0) > 0).all()
    assert np.abs(fit["eigvals"] - cs["lam"][:k]).max() <= np.linalg.norm(cs["dc"])        # Weyl
    again = host(P.fit(x, k))
    assert all(np.array_equal(fit[key], again[key]) for key in fit)


@pytest.mark.parametrize("n,d,relu", CASES)
def test_projection_from_the_oracles_components(n, d, relu):
    """Scores within 4 * 2^-24 sum_d |xc_id| |v_dj| of float64; Y0's first column at standard
    deviation 1e-4 to 1e-6 relative, its second zero for k = 1."""
    cs = PC.case(n, d, relu)
    ref = cs["fit"]
    comps64 = ref["components"].astype(np.float64)
    y0 = dev(T.initial_numpy(n, 0)[0])
    scores = P.project(dev(cs["x"]), dev(ref["components"]), dev(ref["eigvals"]), y0).cpu().numpy()
    bound = 4 * 2.0 ** -24 * (np.abs(cs["xc"]) @ np.abs(comps64).T)
    worst = (np.abs(scores - cs["xc"] @ comps64.T) / np.maximum(bound, 1e-300)).max()
    y0 = y0.cpu().numpy()
    sd = np.std(y0[:, 0].astype(np.float64))
    print("project n=%d d=%d relu=%d: worst %.3f of the bound, sd(Y0[:, 0]) = 1e-4 (1 %+.1e)" % (n, d, relu, worst, sd / 1e-4 - 1))
    assert (np.abs(scores - cs["xc"] @ comps64.T) <= bound).all()
    assert abs(sd / 1e-4 - 1) <= 1e-6 and np.array_equal(y0, P.y0_numpy(scores, ref["eigvals"][0]))
    assert cs["k"] > 1 or not y0[:, 1].any()


def test_identical_rows():
    """l_1 = 0: C = 0, every output finite, and Y0 keeps the seed's draw."""
    x = np.tile(np.random.RandomState(3).normal(size=(1, 16)).astype(np.float32) + 3.0, (64, 1))
    draw = T.initial_numpy(64, 5)[0]
    y0 = dev(draw)
    fit = host(P.fit(dev(x), 2, y0=y0))
    assert all(np.isfinite(v).all() for v in fit.values())
    assert not fit["eigvals"].any() and not fit["scores"].any() and not fit["resid"].any() and not fit["ratio"].any()
    assert np.array_equal(y0.cpu().numpy(), draw)


@pytest.mark.parametrize("init", ["random", "pca"])
def test_embed_start(init):
    """embed(init=..., iters=2) is bit-equal to the launches of P, the start (for "pca": pca.fit's Y0
    over the seed's draw) and two hand-issued steps; "random" issues exactly the parent's calls."""
    cs = PC.case(129, 64)
    x = dev(cs["x"])
    got, trace = T.embed(x, perplexity=10, iters=2, seed=1, init=init)
    work = T._workspace(129, 64)
    p, _ = T.affinities(T.sqdist(x, work), 10, work)
    y, vel, gains = (dev(v) for v in T.initial_numpy(129, 1))
    if init == "pca":
        P.fit(x, 2, seed=1, y0=y)
        ref = T.initial_pca_numpy(cs["x"], 1)[0]
        rel = np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max()
        # a vector off by e moves a row's score by e |xc_i|: test_fit_end_to_end's bound on the second
        # vector, in units of the largest score, plus 1e-6 for the float32 roundings and l_1's own error
        bound = (2.0 * np.linalg.norm(cs["dc"]) / PC.gaps(cs["lam"], 2).min() * np.sqrt((cs["xc"] ** 2).sum(axis=1).max())
                 / np.abs(cs["fit"]["scores"]).max() + 1e-6)
        print("Y0 against initial_pca_numpy: %.2e of its largest entry (bound %.2e)" % (rel, bound))
        assert rel <= bound
    for t in range(2):
        T.step(p, y, vel, gains, *T.schedule(t), 200, work)
    assert trace.size == 0 and np.array_equal(got.cpu().numpy(), y.cpu().numpy())
