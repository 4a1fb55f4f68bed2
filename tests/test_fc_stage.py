"""tests/fc_stage.py pinned to the oracle, its checkers shown to reject the errors they exist
for, and the coverage of the geometry table of tests/test_gpu_fc_shapes.py checked against
restatements of the two dispatch rules it is built around."""
import numpy as np
import pytest

import fc_stage as S
from oracle import ba3c_oracle as O
from test_gpu_parity import as64, case

ORACLE_TOL = 1e-10               # float64 rounding (test_oracle.py's bound for the torch restatement)
NAMES = sorted(S.GEOMETRIES, key=lambda n: int(n[1:]))


def _close(a, b):
    return S.normwise(a, b) < ORACLE_TOL


@pytest.mark.parametrize("name", NAMES)
def test_helper_equals_the_oracle(name):
    g, B = S.GEOMETRIES[name], 7
    params, state, action, R, cfg = case(200 + int(name[1:]), B, wscale=2.0, **g)
    p64 = as64(params)
    t, osc, grads = O.loss_and_grads(p64, state, action, R.astype(np.float64), cfg)
    a3 = t["a3"].reshape(B, 1600)
    fw = S.fc1_forward(p64, cfg, a3)
    assert _close(fw["h_pre"], t["h_pre"]) and _close(fw["h"], t["h"])
    assert np.all(fw["mag"] >= np.abs(fw["h_pre"]) * (1 - 1e-12))
    hd = S.heads_forward(p64, fw["h"], explore_factor=1.7)
    t17 = O.get_nn_prediction(p64, state, cfg, explore_factor=1.7)
    assert _close(hd["policy"], t["policy"]) and _close(hd["logits"], t["logits"])
    assert _close(hd["logitsT"], t17["logitsT"]) and _close(hd["pred_value"], t["pred_value"])
    lb = S.loss_backward(p64, fw["h"], action, R, entropy_beta=0.01)
    from ba3c_amd._lib import SCALAR_NAMES
    for i, n in enumerate(SCALAR_NAMES[:7]):
        assert abs(lb["scalars"][i] - float(osc[n])) <= ORACLE_TOL * max(1.0, abs(float(osc[n]))), n
    assert _close(lb["dz"], t["dz"]) and _close(lb["dV"], t["dV"])
    dh, dh_mag = S.head_dh(p64, cfg, lb["dz"], lb["dV"], fw["h"])
    assert _close(dh, t["dh"]) and np.all(dh_mag >= np.abs(dh) * (1 - 1e-12))
    dy3, dy3_mag = S.fc1_dgrad(p64, cfg, dh, a3)
    assert _close(dy3.reshape(B, 5, 5, 64), t["da3"])
    assert np.all(dy3_mag >= np.abs(dy3) * (1 - 1e-12))
    got = dict(S.fc1_wgrad(cfg, a3, dh))
    got.update(S.head_wgrad(fw["h"], lb["dz"], lb["dV"]))
    want = {k: v for k, v in grads.items() if not k.startswith("conv")}
    assert sorted(got) == sorted(want)
    for k, (grad, mag) in got.items():
        assert grad.shape == mag.shape == params[k].shape, k
        assert _close(grad, want[k]), k
        assert np.all(mag >= np.abs(grad) * (1 - 1e-12)), k
        if not (g["A"] == 1 and k.startswith("fc-pi")):       # one action: a constant softmax
            assert np.abs(want[k]).max() > 0, k


_G3 = {}


def _g3_products():
    """The helper's exact h, dY3 and fc1 gradient for g3 at B = 33 as (exact, mag, K), each 2-d."""
    # (a float64 forward of 33 images: computed once, shared by the tests below, never changed)
    if not _G3:
        g, B = S.GEOMETRIES["g3"], 33
        params, state, action, R, cfg = case(233, B, wscale=2.0, **g)
        p64 = as64(params)
        a3 = O.get_nn_prediction(p64, state, cfg)["a3"].reshape(B, 1600)
        fw = S.fc1_forward(p64, cfg, a3)
        lb = S.loss_backward(p64, fw["h"], action, R)
        dh, _ = S.head_dh(p64, cfg, lb["dz"], lb["dV"], fw["h"])
        dy3, dy3_mag = S.fc1_dgrad(p64, cfg, dh, a3)
        gw, gw_mag = S.fc1_wgrad(cfg, a3, dh)["fc1_0/W"]
        # the valid columns of dY3 and rows of the gradient: the conv3 units that fire for some
        # sample (the others are exactly zero in both, whatever is done to them)
        live = (a3 > 0).any(axis=0)
        dy3, dy3_mag = dy3[:, live], dy3_mag[:, live]
        _G3.update(h=(fw["h"], fw["mag"], 1600), dy3=(dy3, dy3_mag, g["F"]),
                   fc1_grad=(gw.reshape(1600, -1)[live], gw_mag.reshape(1600, -1)[live], B))
    return _G3


def _corrupt(kind, x, mag):
    y = x.copy()
    if kind == "stale_column":                                # the last column computed as column n - 5
        y[:, -1] = x[:, -5]
    elif kind == "zero_tail":                                 # a tail tile never written
        y[:, -4:] = 0
    elif kind == "tail_element":                              # one element off by 2^-9 of its scale
        i = np.flatnonzero(mag[:, -1] > 0)[-1]               # (dY3: the last sample that fires there)
        y[i, -1] += 2.0 ** -9 * mag[i, -1]
    else:                                                     # rows B - 1 and B - 2 exchanged
        y[[-1, -2]] = x[[-2, -1]]
    assert not np.array_equal(x, y)
    return y


@pytest.mark.parametrize("product", ["h", "dy3", "fc1_grad"])
def test_within_model_accepts_float32_rounding(product):
    exact, mag, K = _g3_products()[product]
    assert S.within_model(exact.astype(np.float32), exact, mag, K)
    assert S.model_ratio(exact.astype(np.float32), exact, mag, K) > 0


@pytest.mark.parametrize("kind", ["stale_column", "zero_tail", "tail_element", "swapped_rows"])
@pytest.mark.parametrize("product", ["h", "dy3", "fc1_grad"])
def test_within_model_rejects(product, kind):
    exact, mag, K = _g3_products()[product]
    bad = _corrupt(kind, exact, mag).astype(np.float32)
    print("%s %s: max |err| / bound %.3g" % (product, kind, S.model_ratio(bad, exact, mag, K)))
    assert not S.within_model(bad, exact, mag, K)


def test_within_model_rejects_a_nan():
    exact, mag, K = _g3_products()["h"]
    bad = exact.copy()
    bad[3, -1] = np.nan
    assert not S.within_model(bad, exact, mag, K)


def test_tail_element_corruption_is_a_few_gamma():
    """2^-9 of the magnitude sum is about 3.4 x the bound's coefficient at K = 1600: the
    element-wise check resolves errors of that size, far below any normwise tolerance."""
    assert 3.3 < 2.0 ** -9 / (S.gamma(6 * 1600 + S.P_MAX) + S.DROPPED) < 3.5


def test_bound_is_the_stated_formula():
    mag = np.array([[2.0, 0.0]])
    n = 6 * 68 + 64
    want = (n * 2.0 ** -24 / (1 - n * 2.0 ** -24) + 2.0 ** -23 + 2.0 ** -23) * mag + 68 * 2.0 ** -126
    assert np.array_equal(S.bound(mag, 68, extra=2.0 ** -23), want)


def test_geometry_table_covers_every_form_exit_and_tail():
    gs = list(S.GEOMETRIES.values())
    assert len(gs) == 13
    assert {S.heads_form(g["F"], g["A"]) for g in gs} == S.ALL_HEADS_FORMS
    assert len(S.ALL_HEADS_FORMS) == 7
    assert {S.reduce_exit(g["A"]) for g in gs} == {4, 8, 16, 64}
    assert {1, 4, 8, 9, 16, 17, 31} <= {g["A"] for g in gs}
    assert {4, 36} <= {g["F"] % 64 for g in gs}
    assert any(g["F"] % 128 == 4 for g in gs)
    assert any((g["F"] // S.n_splits(g)) % 32 for g in gs)
    assert any(g["F"] % 32 for g in gs)                       # FcDgrad's K tail (GEMM_BK = 32)
    assert any(g.get("legacy") and S.n_splits(g) > 1 for g in gs)
    assert any(g["C"] == 12 for g in gs)
    for g in gs:
        assert S.create_rule_ok(g["F"], S.n_splits(g), g["A"]), g


def test_dispatch_restatements_at_their_thresholds():
    assert [S.heads_form(F, 6) for F in (4, 64, 68, 128, 132, 256, 260, 512, 516)] == \
        [(1, 0), (1, 0), (2, 0), (2, 0), (4, 0), (4, 0), (8, 0), (8, 0), (0, 0)]
    assert [S.heads_form(F, 4) for F in (64, 68, 128, 132, 256, 260, 512, 516)] == \
        [(1, 0), (2, 4), (2, 4), (4, 0), (4, 0), (8, 4), (8, 4), (0, 0)]
    assert [S.reduce_exit(A) for A in (1, 4, 5, 8, 9, 16, 17, 31)] == [4, 4, 8, 8, 16, 16, 64, 64]
    assert not S.create_rule_ok(66, 1, 4) and not S.create_rule_ok(72, 4, 4)
    assert not S.create_rule_ok(68, 1, 32) and not S.create_rule_ok(68, 1, 0)
