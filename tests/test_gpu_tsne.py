"""The t-SNE kernels on the MI355X, each stage against ba3c_amd/tsne.py on the same inputs (so the
errors of a stage do not reach the next one), the embedding end to end, and Ba3cEngine.features.

The bounds are four times the worst figure measured over the cases of test_distances,
test_affinities and test_one_step (DESIGN.md section 23.1 lists the figures); the cases below
test_features_are_the_forward_workspace are held to the same bounds and did not set them: every
instantiation and row split of tsne_pairs_kernel up to the limit N = 8192 on the crafted inputs of
tests/tsne_cases.py, the update rule's edges, and the distances' and affinities' input edges.  Every
test prints its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch

import tsne_cases as C
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
    assert abs(p.sum(dtype=np.float64) - 1) <= 1e-6
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


# ---- every variant of the iteration, the update rule's edges, the input edges of P's launches --------

assert C.TOL_STEP == TOL_STEP                      # tests/test_tsne_cases.py holds the oracle to this bound
SENTINEL = -123.25


def run_step(p, state, exag, momentum, with_kl, lr=200.0):
    """One device step from `state` (numpy) -> (Y, U, G, the two-element KL buffer), numpy.  The
    buffer starts as two sentinels; only with_kl hands its first element to the step."""
    y, u, g = (dev(v) for v in state)
    out = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda")
    T.step(p if torch.is_tensor(p) else dev(p), y, u, g, exag, momentum, lr, T._workspace(y.shape[0]),
           out if with_kl else None)
    return tuple(t.cpu().numpy() for t in (y, u, g, out))


def check_step(label, got, ref, with_kl, kl_bound=None):
    """What test_one_step asserts, of a run_step against a step_numpy: the gains equal wherever the
    oracle's gradient is clear of zero, Y, U and the KL within TOL_STEP, the KL's neighbour (and
    without a KL the whole buffer) untouched.  kl_bound: an absolute bound on the KL's error that
    replaces TOL_STEP |KL| (test_step_variants).  -> the unsure entries."""
    (y, u, g, out), (y1, u1, g1, kl, grad) = got, ref
    unsure = C.unsure(grad, TOL_STEP)
    assert unsure.mean() < 0.01
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    kl_bound = TOL_STEP * abs(kl) if kl_bound is None else kl_bound
    print("step %s: Y %.3e U %.3e KL %s, %d of %d gains unsure"
          % (label, rel(y, y1), rel(u, u1), "%.3e (%.3f of its bound, KL = %.4f)"
             % (abs(out[0] - kl) / abs(kl), abs(out[0] - kl) / kl_bound, kl) if with_kl else "none",
             unsure.sum(), unsure.size))
    assert np.array_equal(g[~unsure], g1[~unsure]) and out[1] == SENTINEL
    assert rel(u, u1) <= TOL_STEP and rel(y, y1) <= TOL_STEP
    if with_kl:
        assert abs(out[0] - kl) <= kl_bound
    else:
        assert out[0] == SENTINEL
    return unsure


@pytest.mark.parametrize("n,exag,with_kl", [(n, exag, with_kl) for n, exag in C.STEP_CASES
                                             for with_kl in (True, False) if with_kl or n != C.LIMIT_N])
def test_step_variants(n, exag, with_kl):
    """The four instantiations of tsne_pairs_kernel at 1, 2 and 4 rows per wave, against
    step_numpy_chunked on tests/tsne_cases.py's crafted P and state.  132: 16-byte loads, half the
    lanes idle; 260: a second, partial pass of them; 2049: scalar, 2 rows, the last wave owns one row
    and breaks; 2052: 16-byte, 2 rows, the last workgroup half empty; 4098: scalar, 4 rows, a break
    after two; 4100: 16-byte, 4 rows; 8192: the limit, 64 KB of LDS (with a KL only: its host oracle
    is the slow part).

    Y, U and the gains are held to TOL_STEP.  The KL is not held to TOL_STEP |KL| here: the crafted
    state fits its P, so KL = sum p log(p / num) + log Z is 0.21 to 0.23, the difference of two
    numbers of the size of log N^2 (-14.8 and 15.0 at N = 4100), and the device's is low by 3.3e-7
    ABSOLUTE at N = 132 and 260 and by 6.6e-7 at every N >= 2049: 1.4e-6 to 3.2e-6 of the KL, where
    TOL_STEP is 3.4e-7.  The error is logf's, which is the hardware's log2 times ln 2: the figures are
    ln 2 times half an ulp of a log2 in [-16, -8) and in [-32, -16), on terms that all have one
    sign.  The KL is held to tsne_cases.kl_bound instead, u (7 sum |p L| + 6 sum p + 10) with
    u = 2^-24, counted from tsne_pair's fp32 operations in kl_bound's docstring and computed from
    the oracle alone (4.2e-6 to 7.8e-6; the measured error is a tenth of it).  DESIGN.md section 23.1."""
    p, state, passed = C.crafted_case(n)
    ref = C.step_numpy_chunked(p, *state, exag, 0.5, 200.0, passed)
    check_step("n=%d exag=%g" % (n, exag), run_step(p, state, exag, 0.5, with_kl), ref, with_kl, C.kl_bound(passed))


@pytest.mark.parametrize("exag", [12.0, 1.0])
@pytest.mark.parametrize("n", [65, 128, 257])
def test_one_step_without_kl(n, exag):
    """test_one_step's cases through the two instantiations without the KL terms."""
    p, state = oracle_state(n)
    ref = T.step_numpy(p, *state, exag, 0.5, 200.0)
    check_step("n=%d exag=%g (oracle-made P)" % (n, exag), run_step(p, state, exag, 0.5, False), ref, False)


@pytest.mark.parametrize("edge", ["first", "momentum0", "floor"])
@pytest.mark.parametrize("n", [65, 128])               # scalar, 16-byte
def test_update_rule_edges(n, edge):
    """first: iteration 0 (U = 0, so grad alone decides a gain's direction; Y of order 1e-4).
    momentum0: U is -lr G grad alone.  floor: every gain is 0.0101, and each one that is lowered
    (0.0101 * 0.8) must come out as exactly float32(0.01), each raised one as 0.0101f + 0.2f."""
    p, state = oracle_state(n)
    momentum = 0.0 if edge == "momentum0" else 0.5
    if edge == "first":
        state = T.initial_numpy(n, 0)
    elif edge == "floor":
        state = state[:2] + (np.full((n, 2), 0.0101, np.float32),)
    ref = T.step_numpy(p, *state, 12.0, momentum, 200.0)
    got = run_step(p, state, 12.0, momentum, True)
    unsure = check_step("n=%d %s" % (n, edge), got, ref, True)
    if edge == "first":
        assert not state[1].any() and np.array_equal(ref[2] > 1, ref[4] > 0)
    if edge == "floor":
        lowered = (ref[2] == np.float32(0.01)) & ~unsure
        raised = (ref[2] == np.float32(0.0101) + np.float32(0.2)) & ~unsure
        print("floor n=%d: %d gains lowered to the floor, %d raised" % (n, lowered.sum(), raised.sum()))
        assert lowered.any() and raised.any() and (lowered | raised | unsure).all()
        assert (got[2][lowered] == np.float32(0.01)).all() and (got[2][raised] == ref[2][raised]).all()


@pytest.mark.parametrize("n", [260, 2052])
def test_step_is_deterministic(n):
    """No atomics, and every workgroup sums Z in the same order: two calls from the same state are
    equal bit for bit."""
    p, state, _ = C.crafted_case(n)
    pd = dev(p)
    a, b = run_step(pd, state, 12.0, 0.5, True), run_step(pd, state, 12.0, 0.5, True)
    same = [np.array_equal(x, y) for x, y in zip(a, b)]
    print("determinism n=%d: Y, U, G, KL equal: %s" % (n, same))
    assert all(same) and np.isfinite(a[3][0]) and a[3][0] != SENTINEL


# ---- the distances' input edges ----------------------------------------------------------------

@pytest.mark.parametrize("s", [40, -40])
def test_distances_scale_by_powers_of_two_exactly(s):
    """sqdist(X 2^s) == sqdist(X) 2^(2s) bit for bit.  Every operation commutes with the scaling as
    long as nothing leaves float32's normal range, and with |x| <= 20 and s = +-40 nothing does
    (squares are within 2^+-90): the float64 column sums and their rounding to float32 scale by
    2^s, so Xc does, the float64 row norms and their float32 rounding scale by 2^2s, the largest
    |xc| moves amax_exp's k by exactly -s (|k| <= 100 is not reached: k is -29 or 51), so the
    scaled values xc 2^k, their fp16 hi / lo planes and the fp32 accumulators are the SAME numbers,
    and the two multiplications by 2^-k and the epilogue's (n_i + n_j) - 2 g are exact scalings of
    the unscaled run's."""
    x = clusters(129, 33)
    xs = x * np.float32(2.0 ** s)
    assert xs.dtype == np.float32 and np.array_equal(xs.astype(np.float64), x.astype(np.float64) * 2.0 ** s)
    base = T.sqdist(dev(x)).cpu().numpy()
    got = T.sqdist(dev(xs)).cpu().numpy()
    want = base * np.float32(2.0 ** (2 * s))
    off = ~np.eye(129, dtype=bool)
    print("sqdist of X 2^%d: %d of %d entries differ from the scaled run, smallest d > 0 %.3e, largest %.3e"
          % (s, (got != want).sum(), got.size, want[off & (base > 0)].min(), want.max()))
    assert np.isfinite(got).all() and want[off & (base > 0)].min() > 1e-37      # nothing went subnormal
    assert np.array_equal(got, want)


def test_distances_of_identical_rows_are_zero():
    """rowmax = 0, so kexp = 0: every product and every norm is exactly 0."""
    x = np.tile(np.random.RandomState(3).normal(size=(1, 16)).astype(np.float32) + 3.0, (64, 1))
    got = T.sqdist(dev(x)).cpu().numpy()
    print("sqdist of 64 identical rows: largest |d| %.3e" % np.abs(got).max())
    assert got.shape == (64, 64) and not got.any()


def relu_features(n, d):
    """What Ba3cEngine.features returns looks like this: most entries exactly 0, some columns all 0."""
    x = np.maximum(0, clusters(n, d) - 3.5).astype(np.float32)
    x[:, [1, 5, d - 2, d - 1]] = 0
    return x


@pytest.mark.parametrize("n,d", [(64, 32), (130, 40)])     # one full tile and K-step; a partial tile and 8-float load
def test_distances_of_relu_features(n, d):
    x = relu_features(n, d)
    got = T.sqdist(dev(x)).cpu().numpy()
    ref, n2 = T.sqdist_numpy(x), (T.center_numpy(x).astype(np.float64) ** 2).sum(axis=1)
    err = np.abs(got - ref) / np.maximum(n2[:, None] + n2[None, :], 1e-300)
    print("sqdist of ReLU features n=%d d=%d (%.0f %% zeros): worst %.3e of |xc_i|^2 + |xc_j|^2"
          % (n, d, 100 * (x == 0).mean(), err.max()))
    assert (x == 0).mean() > 0.5 and not x[:, d - 1].any() and n2.min() > 0
    assert not got.diagonal().any() and np.array_equal(got, got.T) and got.min() >= 0
    assert err.max() <= TOL_D


# ---- the affinities' input edges ---------------------------------------------------------------

COPIES = np.arange(5, 65, 5)                           # 12 rows of duplicated(): more than any u <= 11


def duplicated():
    """clusters(65, 16) with the rows COPIES exact copies of one another."""
    x = clusters(65, 16)
    x[COPIES] = x[COPIES[0]]
    return x


def device_affinities(d, u):
    p, beta = T.affinities(dev(d), u)
    return p.cpu().numpy(), beta.cpu().numpy()


def check_p(p):
    assert np.array_equal(p, p.T) and not p.diagonal().any() and p.min() >= 0
    assert abs(p.sum(dtype=np.float64) - 1) <= 1e-6


def test_affinities_of_more_duplicates_than_the_perplexity():
    """A row with 11 neighbours at distance 0 has entropy >= log 11 > log 3 at every beta: both
    sides double beta 100 times and stop at 2^100, where the row is uniform over its copies.  So does
    a row whose nearest neighbours are the 12 copies, all at one distance (rows 14 and 23 of this X):
    the rows that saturate are the oracle's, and every other row has the perplexity."""
    u, d = 3, T.sqdist_numpy(duplicated())
    d[np.ix_(COPIES, COPIES)] = 0.0                # what the exact rule gives; a Gram matrix in float64 need not
    d = d.astype(np.float32)
    ref, beta_ref = T.affinities_numpy(d, u)
    p, beta = device_affinities(d, u)
    sat = beta_ref == 2.0 ** 100
    rest = np.flatnonzero(~sat)
    dm = np.where(np.eye(65, dtype=bool), np.inf, d.astype(np.float64))
    e = np.exp(-beta[:, None] * (dm - dm.min(axis=1, keepdims=True)))
    pc = e / e.sum(axis=1, keepdims=True)
    perp = np.exp(-(pc * np.log(np.where(pc > 0, pc, 1.0))).sum(axis=1))
    err = np.abs(p - ref).max() / ref.max()
    print("affinities with 12 copies, u=3: beta of the copies 2^%g, %d rows saturate (the oracle: %d), perplexity "
          "of the rest off by %.3e, P off by %.3e of max P"
          % (np.log2(beta[COPIES]).max(), (beta == 2.0 ** 100).sum(), sat.sum(), np.abs(perp[rest] / u - 1).max(), err))
    assert sat[COPIES].all() and len(rest) >= 40 and np.array_equal(beta[sat], beta_ref[sat])
    assert np.abs(beta[rest] / beta_ref[rest] - 1).max() <= 1e-9
    assert np.abs(perp[rest] / u - 1).max() <= 1e-4
    check_p(p)
    assert err <= TOL_P


def test_affinities_of_all_zero_distances():
    n, u = 64, 5
    d = np.zeros((n, n), np.float32)
    ref, _ = T.affinities_numpy(d, u)
    p, beta = device_affinities(d, u)
    err = np.abs(p - ref).max() / ref.max()
    print("affinities of d = 0: P off by %.3e of max P, beta 2^%g" % (err, np.log2(beta).max()))
    off = ~np.eye(n, dtype=bool)
    assert (beta == 2.0 ** 100).all() and np.abs(ref[off] * (n * (n - 1)) - 1).max() <= 1e-6
    check_p(p)
    assert err <= TOL_P


def test_affinities_at_the_limit_on_a_subset():
    """N = 8192 (32 KB of LDS per row, 128 x 128 tile pairs): the device on all of d, the oracle's
    bisection on 16 rows S that are one another's nearest neighbours: the first and last rows, both
    sides of the tile seam 63 | 64, and rows of row 8191's tile."""
    n, u = C.LIMIT_N, 50
    S = np.array([0, 1, 2, 3, 62, 63, 64, 65, 66, 8128, 8129, 8130, 8160, 8189, 8190, 8191])
    z = C.crafted_points(n)
    z[S] = z[0] + 0.02 * np.random.RandomState(5).standard_normal((len(S), 2))
    d = C.crafted_dist(z)
    rows = [T.conditional_row_numpy(d[i].astype(np.float64), i, np.log(float(u))) for i in S]
    beta_ref, pc = np.array([b for b, _ in rows]), np.stack([r for _, r in rows])
    ref = ((pc[:, S] + pc[:, S].T) / (2.0 * n)).astype(np.float32)
    scale = pc.max() / (2.0 * n)                    # max P of what the oracle evaluated
    p, beta = T.affinities(dev(d), u)
    sym = torch.equal(p, p.T) and not p.diagonal().any().item() and p.min().item() >= 0
    total = p.sum(dtype=torch.float64).item()
    Sd = torch.as_tensor(S, device="cuda")
    got, beta = p[Sd][:, Sd].cpu().numpy(), beta[Sd].cpu().numpy()
    err = np.abs(got - ref).max() / scale
    print("affinities n=%d u=%d on 16 rows: beta off by %.3e, P off by %.3e of max P (largest P[S, S] %.3f of it), "
          "sum P - 1 = %.3e" % (n, u, np.abs(beta / beta_ref - 1).max(), err, ref.max() / scale, total - 1))
    assert ref.max() >= 0.5 * scale                 # the subset holds entries of the size of the largest
    assert sym and abs(total - 1) <= 1e-6
    assert np.abs(beta / beta_ref - 1).max() <= 1e-9
    assert err <= TOL_P


def test_chained_launches_with_duplicates():
    """affinities(sqdist(X)) on the device where X holds 12 copies of a row and u = 3.  The device's
    distance between two copies is rounding noise, not 0, so nothing compares bit for bit with the
    oracle; what must hold is that P is a finite joint distribution."""
    x = duplicated()
    d = T.sqdist(dev(x))
    p, beta = T.affinities(d, 3)
    d, p, beta = d.cpu().numpy(), p.cpu().numpy(), beta.cpu().numpy()
    n2 = (T.center_numpy(x).astype(np.float64) ** 2).sum(axis=1)[COPIES[0]]
    print("chained, 12 copies: largest device distance between copies %.3e of 2 |xc|^2, their beta up to %.3e"
          % (d[np.ix_(COPIES, COPIES)].max() / (2 * n2), beta[COPIES].max()))
    assert np.isfinite(p).all() and np.isfinite(beta).all() and (beta > 0).all()
    check_p(p)


# ---- embed()'s KL slots ------------------------------------------------------------------------

def test_embed_slots():
    """embed(iters=7, kl_every=3) is the three launches of P and seven steps of which t = 2 and t = 5
    alone receive a KL element, the first and the second of the trace; iters < kl_every gives an
    empty trace.  Both bit for bit."""
    n, dd, u = 132, 8, 20
    x = dev(clusters(n, dd))
    work = T._workspace(n, dd)
    p, _ = T.affinities(T.sqdist(x, work), u, work)

    def by_hand(iters, slots):
        y, vel, gains = (dev(v) for v in T.initial_numpy(n, 0))
        kl = torch.full((len(slots) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
        for t in range(iters):
            T.step(p, y, vel, gains, *T.schedule(t), 200.0, work, kl[slots.index(t):] if t in slots else None)
        return y, kl.cpu().numpy()

    y7, kl7 = by_hand(7, [2, 5])
    y, trace = T.embed(x, perplexity=u, iters=7, kl_every=3)
    print("embed 7 / 3: trace %s, by hand %s" % (trace, kl7[:2]))
    assert trace.shape == (2,) and trace.dtype == np.float64 and np.array_equal(trace, kl7[:2])
    assert kl7[2] == SENTINEL and np.isfinite(trace).all() and trace[0] != trace[1]
    assert torch.equal(y, y7)
    y2, _ = by_hand(2, [])
    y, trace = T.embed(x, perplexity=u, iters=2, kl_every=3)
    assert trace.shape == (0,) and torch.equal(y, y2) and not torch.equal(y2, y7)
