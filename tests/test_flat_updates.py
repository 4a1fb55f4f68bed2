"""The recipe of tests/flat_updates.py pinned on the oracle alone (no GPU): what the deals
contain, that every case stays finite, and that the float32 oracle's own distance to the
float64 one (the yardstick the GPU tests scale their bound from) stays under 1e-6.  That cap
is a condition on the inputs: a geometry that breaks it needs other inputs, not another cap.

Measured yardsticks, worst over the four geometries, both hyper-parameter sets and the four
deals (clip 1.3e-7: it does not depend on the optimizer), and of the unfused-scale deals:
    optimizer   parameters   slot 0     slot 1      scaled: parameters   slot 0     slot 1
    adam        2.5e-7       1.8e-7     2.9e-7              2.8e-7       9.7e-8     9.9e-8
    rms         2.2e-7       3.1e-7     2.5e-7              1.8e-7       1.2e-7     1.9e-7
    gd          1.3e-7       -          -                   4.2e-8       -          -
    momentum    1.6e-7       3.0e-7     -                   9.8e-8       5.7e-8     -
    adagrad     1.9e-7       2.9e-7     -                   1.9e-7       7.9e-8     -
    adadelta    2.7e-7       3.0e-7     6.0e-7              2.7e-7       1.1e-7     6.2e-7
"""
import numpy as np
import pytest

import flat_updates as U

GEOMS = sorted(U.GEOMETRIES)


def test_geometries_are_what_their_names_say():
    t = {g: dict(U.tensors(g)) for g in GEOMS}
    c = {g: U.chunk_count(t[g].values()) for g in GEOMS}
    assert t["odd"]["fc1_0/W"] == 57600 == 14 * U.UPD_CHUNK + 256
    assert (t["odd"]["fc-pi/W"], t["odd"]["fc-pi/b"], t["odd"]["fc-v/b"]) == (1116, 31, 1)
    assert t["bench"]["fc1_0/W"] == 200 * U.UPD_CHUNK       # three 64-lane passes and 8
    assert len(t["legacy"]) == 16 and t["legacy"]["fc1_2/b"] == 64
    assert c == {"odd": 52, "bench": 237, "legacy": 142, "over": 438}
    # fc1 of `over`: 100 chunks each, a second lane pass that is not full
    assert t["over"]["fc1_3/W"] == 100 * U.UPD_CHUNK
    U.check_cu_sides(256, c)                                # MI355X: 256 CUs
    with pytest.raises(AssertionError):
        U.check_cu_sides(1024, c)


def test_default_set_is_make_optimizers():
    from ba3c_amd.optimizer import make_optimizer
    for opt in U.OPTS:
        h = make_optimizer(opt, 1e-3, beta1=0.8, beta2=0.75, epsilon=1e-8)._hparams()
        for k, v in U.HP[opt][0].items():
            assert h[k] == v, (opt, k)
        z = U.initial_slots(opt, 3)
        assert sum(x is not None for x in z) == U.N_SLOTS[opt]
    second = {"adam": dict(lr=1e-3, beta1=0.8, beta2=0.75, epsilon=1e-3),
              "rms": dict(lr=7e-4, decay=0.99, momentum=0.5, epsilon=1e-6),
              "gd": dict(lr=1e-2), "momentum": dict(lr=1e-3, momentum=0.5),
              "adagrad": dict(lr=1e-2), "adadelta": dict(lr=0.5, rho=0.9, epsilon=1e-6)}
    for opt, want in second.items():
        got = {k: v for k, v in U.HP[opt][1].items() if v != 0.0}
        assert got == want, opt


@pytest.mark.parametrize("geom", GEOMS)
def test_deals_hold_both_branches_a_zero_and_a_tail_only_tensor(geom):
    names = [n for n, _ in U.tensors(geom)]
    numels = [n for _, n in U.tensors(geom)]
    seen = [set() for _ in names]
    for step in range(U.NSTEPS):
        kinds = U.deal(geom, step)
        g = U.dealt_gradients(geom, step)
        cap = []
        for i, (k, gi) in enumerate(zip(kinds, g)):
            assert gi.dtype == np.float32 and gi.shape == (numels[i],)
            sq = gi.astype(np.float64) ** 2
            # g^2 and sum g^2 inside normal float32 range
            assert sq[sq > 0].min(initial=1.0) > 1.2e-38 and sq.sum() < 3e38, (step, names[i])
            c64, c32 = U.took_cap(gi, np.float64), U.took_cap(gi, np.float32)
            if k == 5:      # at the threshold: either branch, the same result to rounding
                assert U.norm_err(U.clip32(gi), U.clip64(gi)) < U.YARDSTICK_CAP
            else:           # the float64 reference and the float32 oracle took the same branch
                assert c64 == c32, (step, names[i], k)
            cap.append(c64)
            if step < 3:
                seen[i].add(k)
        if step < 3:
            assert set(kinds) == {0, 1, 2, 3}
            assert any(cap) and not all(cap)
            assert all(c for c, k in zip(cap, kinds) if k in (0, 2))
            assert any(not np.any(x) for x in g)
            assert any(np.count_nonzero(x) == 1 and x[-1] == 7 for x in g)
        else:
            # the largest tensor's clipped branch: its factor depends on every chunk's partial
            big = int(np.argmax(numels))
            assert set(kinds) == {4, 5} and kinds[big] == 4 and not cap[big]
    for i, s in enumerate(seen):    # the largest tensor and the 1-element fc-v/b included
        assert {0, 1} <= s and s & {2, 3}, (names[i], s)
    for step in range(2):
        assert set(U.deal_scale(geom, step)) == {0, 1, 4}


def test_gradient_kinds():
    rs = np.random.RandomState(0)
    n = 5000
    assert U.took_cap(U.gradient(0, n, rs), np.float64)
    assert not U.took_cap(U.gradient(1, n, rs), np.float64)
    assert not np.any(U.clip64(U.gradient(2, n, rs)))
    g3 = U.gradient(3, n, rs)
    assert np.count_nonzero(g3) == 1 and g3[-1] == 7
    e = np.frexp(U.gradient(4, n, rs))[1]
    assert e.min() < -15 and e.max() > 8
    g5 = U.gradient(5, n, rs).astype(np.float64)
    assert abs(np.sqrt((g5 ** 2).sum()) / n / 0.1 - 1) < 1e-6


def test_measures_bite():
    """A 10 % error in the clip factor, a dropped momentum term and a one-ulp nudge of an
    unchanged parameter are all far outside what the measures let through."""
    rs = np.random.RandomState(1)
    n = 3000
    g = U.gradient(0, n, rs)
    assert U.norm_err(U.clip32(g) * np.float32(0.9), U.clip64(g)) > 0.09
    p = rs.normal(0, 0.05, n).astype(np.float32)
    hp = U.HP["rms"][1]
    s0, s1 = U.initial_slots("rms", n)
    s1 = s1 + np.float32(0.01)
    r64, y = U.reference_update("rms", hp, g, p, s0, s1)
    assert max(y.values()) < U.YARDSTICK_CAP
    wrong = U.apply32("rms", p, U.clip32(g), s0, s1, dict(hp, momentum=0.0))
    e = U.update_errs(wrong, r64, p)
    assert e["p"] > 0.1 and e["s1"] > 0.1 and e["s0"] < U.YARDSTICK_CAP
    z = np.zeros(n, np.float32)
    r64, _ = U.reference_update("gd", U.HP["gd"][0], z, p, None, None)
    assert U.param_err(p, r64[0], p) == 0.0
    assert U.param_err(np.nextafter(p, np.float32(1)), r64[0], p) == float("inf")
    assert U.norm_err(np.full(4, 1e-45, np.float32), np.zeros(4)) == float("inf")


def _run_pair(geom, opt, hp, steps, scale=None):
    """The float32 oracle stepped through the deals -> worst yardstick per measure."""
    ts = U.tensors(geom)
    p = U.initial_params(geom)
    sl = [U.initial_slots(opt, n) for _, n in ts]
    worst = {}
    for step in range(steps):
        kinds = None if scale is None else U.deal_scale(geom, step)
        g = U.dealt_gradients(geom, step, kinds)
        pw = U.adam_powers(hp, step) if opt == "adam" else None
        for i in range(len(ts)):
            r64, y = U.reference_update(opt, hp, g[i], p[i], sl[i][0], sl[i][1], pw, scale)
            assert all(x is None or np.isfinite(x).all() for x in r64), (geom, opt, step, ts[i][0])
            for k, v in y.items():
                worst[k] = max(worst.get(k, 0.0), v)
            if scale is None:
                worst["clip"] = max(worst.get("clip", 0.0), U.norm_err(U.clip32(g[i]), U.clip64(g[i])))
                gc = U.clip32(g[i])
            else:
                gc = (g[i] * np.float32(scale)).astype(np.float32)
            p[i], s0, s1 = U.apply32(opt, p[i], gc, sl[i][0], sl[i][1], hp, pw)
            sl[i] = (s0, s1)
            assert np.isfinite(p[i]).all()
    return worst


@pytest.mark.parametrize("opt,k", U.PAIRS)
@pytest.mark.parametrize("geom", GEOMS)
def test_finite_and_yardstick_under_the_cap(geom, opt, k):
    worst = _run_pair(geom, opt, U.HP[opt][k], U.NSTEPS)
    print("yardstick", geom, opt, k, {m: "%.2e" % v for m, v in sorted(worst.items())})
    assert set(worst) == {"clip", "p"} | {"s%d" % i for i in range(U.N_SLOTS[opt])}
    for m, v in worst.items():
        assert v < U.YARDSTICK_CAP, (m, v)


@pytest.mark.parametrize("opt,k", U.PAIRS)
@pytest.mark.parametrize("geom", ["odd", "over"])
def test_unfused_scale_yardstick_under_the_cap(geom, opt, k):
    worst = _run_pair(geom, opt, U.HP[opt][k], 2, scale=np.float32(1.0) / np.float32(3.0))
    print("yardstick-scale", geom, opt, k, {m: "%.2e" % v for m, v in sorted(worst.items())})
    for m, v in worst.items():
        assert v < U.YARDSTICK_CAP, (m, v)


def test_adam_powers_are_the_float32_chain():
    hp = U.HP["adam"][1]
    b1 = np.float32(0.8)
    assert U.adam_powers(hp, 0) == (np.float32(0.8), np.float32(0.75))
    assert U.adam_powers(hp, 2)[0] == np.float32(np.float32(b1 * b1) * b1)
