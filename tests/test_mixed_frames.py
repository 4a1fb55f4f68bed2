"""What the mixed-scale GPU tests (test_gpu_mixed_scale.py) rest on, pinned on the reference alone.

B=16 mixed_frames images (two of each kind), layer_scaled weights, mixed_returns: the fp64
oracle against its own fp32 evaluation.  The inputs must really separate the exponents (bright
against dim images by >= 2^7, a black image exactly zero everywhere), must not be dominated by
numerically ambiguous pooling windows (the cap of _check_against_oracle: a condition, not a
measurement), and a plain fp32 evaluation must sit well inside FWD_TOL / GRAD_TOL per image —
otherwise a per-image bound would test the inputs, not the kernels.
"""
import numpy as np
import pytest

from oracle import ba3c_oracle as O
from mixed_frames import (KINDS, LAYER_SCALES, mixed_frames, mixed_returns, return_classes,
                          scaled_params)

FWD_TOL = 1e-5      # test_gpu_parity's (that module needs torch; the GPU tests import its own)
GRAD_TOL = 1e-4
B = 16
CFG = dict(fc_neurons=512, fc_splits=1)
MAPS = ("p0", "p1", "p2", "a3", "h")


def per_image_rel(got, ref):
    """max|got_i - ref_i| / max|ref_i| per image (the absolute error where ref_i is all zero)."""
    got = np.asarray(got, np.float64).reshape(len(ref), -1)
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    err, den = np.abs(got - ref).max(axis=1), np.abs(ref).max(axis=1)
    return np.where(den > 0, err / np.where(den > 0, den, 1.0), err)


@pytest.fixture(scope="module")
def ev():
    p32 = scaled_params(5)
    p64 = {k: v.astype(np.float64) for k, v in p32.items()}
    state, kinds = mixed_frames(B, 5)
    rs = np.random.RandomState(5)
    action = rs.randint(0, 4, size=B).astype(np.int64)
    f64 = O.get_nn_prediction(p64, state, CFG)
    f32 = O.get_nn_prediction(p32, state, CFG)
    R = mixed_returns(f64["pred_value"], 5)
    # the checked side's (fp32) own decisions drive the reference's backward, as on the GPU
    t32, _, g32 = O.loss_and_grads_chunked(p32, state, action, R, CFG, chunk=B)
    forced = {"c0": t32["own_c0"], "c1": t32["own_c1"], "c2": t32["own_c2"], "a3_mask": t32["a3_pos"]}
    t64, _, g64 = O.loss_and_grads_chunked(p64, state, action, R.astype(np.float64), CFG,
                                           forced=forced, chunk=B)
    return dict(kinds=kinds, f64=f64, f32=f32, t64=t64, t32=t32, g64=g64, g32=g32, R=R,
                p32=p32, p64=p64, state=state, action=action)


def test_kinds_alternate_and_cover_every_return_class():
    state, kinds = mixed_frames(48, 3)
    assert state.dtype == np.uint8 and state.shape == (48, 84, 84, 4)
    assert np.array_equal(kinds, np.arange(48) % 8) and len(KINDS) == 8
    assert state[2].max() == 0 and np.count_nonzero(state[3]) == 1 and state[3].max() == 255
    assert state[1].max() == 1 and state[5].max() == 15 and np.all(state[6] == 255)
    assert 0 < state[7].max() <= 3 and state[4].max() == 200
    assert {(k, c) for k, c in zip(kinds[:24], return_classes(24))} == \
        {(k, c) for k in range(8) for c in range(3)}
    s12, _ = mixed_frames(8, 3, C=12)
    assert s12.shape == (8, 84, 84, 12) and np.count_nonzero(s12[3]) == 1


def test_layer_scales_put_the_conv_weights_in_distinct_binades():
    p = scaled_params(5)
    binades = [int(np.floor(np.log2(np.abs(p[k]).max()))) for k in LAYER_SCALES]
    assert len(set(binades)) == 4, binades
    assert abs(float(np.prod(list(LAYER_SCALES.values()))) - 1.0) < 1e-12
    assert np.all(p["fc-pi/b"] != 0) and p["fc-v/b"][0] != 0


def test_returns_span_the_advantage_classes(ev):
    adv = np.abs(ev["f64"]["pred_value"] - ev["R"].astype(np.float64))
    scale = np.maximum(1.0, np.abs(ev["f64"]["pred_value"]))
    cls = return_classes(B)
    assert np.all(adv[cls == 0] <= 2.0 ** -24 * scale[cls == 0])
    assert np.all(np.abs(adv[cls == 1] - 1.0) < 1e-5 * scale[cls == 1])
    assert np.all(np.abs(adv[cls == 2] - 1e3) < 1e-3)


def test_bright_and_dim_images_are_binades_apart(ev):
    m = np.abs(ev["f64"]["p0"]).reshape(B, -1).max(axis=1)
    k = ev["kinds"]
    assert m[k == 0].min() >= 2.0 ** 7 * m[k == 1].max(), (m[k == 0], m[k == 1])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_black_image_is_exactly_zero_in_every_layer(ev, dt):
    f, z = ev[dt], ev["kinds"] == 2
    for n in MAPS + ("a0", "a1", "a2"):
        assert not np.any(f[n][z]), n
    for layer in range(3):
        assert np.all(ev["t" + dt[1:]]["own_c%d" % layer][z] == 255)


def test_ambiguous_window_shares_stay_under_the_cap(ev):
    for name in ("near_c0", "near_c1", "near_c2", "near_a3"):
        for k in range(8):
            share = float(np.mean(ev["t64"][name][ev["kinds"] == k]))
            assert share < 1e-2, (name, KINDS[k], share)


def test_fp32_decisions_differ_only_in_ambiguous_windows(ev):
    t64, t32 = ev["t64"], ev["t32"]
    for layer in range(3):
        bad = (t64["own_c%d" % layer] != t32["own_c%d" % layer]) & ~t64["near_c%d" % layer]
        assert not bad.any(), (layer, np.argwhere(bad)[:4])
    bad = (t64["a3_pos"] != t32["a3_pos"]) & ~t64["near_a3"]
    assert not bad.any(), np.argwhere(bad)[:4]


def test_zero_advantage_images_are_ill_conditioned_in_any_fp32_forward(ev):
    """Why the GPU test compares the backward maps of the R = float32(V) images with the
    oracle's heads evaluated on the GPU's own FC output: their advantage is a few ulps of V,
    so the head gradient is linear in the forward's own rounding of V.  The plain fp32
    evaluation misses GRAD_TOL per image there, and only there (measured: up to 5e-4 against
    <= 4.5e-6 on every other image)."""
    B_, st, ac, R = B, ev["state"], ev["action"], ev["R"]
    t32, _, _ = O.loss_and_grads(ev["p32"], st, ac, R, CFG)
    forced = {"c%d" % l: np.where(t32["p%d" % l] > 0, t32["c%d" % l], 255) for l in range(3)}
    forced["a3_mask"] = t32["a3"] > 0
    t64, _, _ = O.loss_and_grads(ev["p64"], st, ac, R.astype(np.float64), CFG, forced=forced)
    floor = return_classes(B_) == 0
    worst_floor = 0.0
    for n in ("dh", "dp2", "dp1", "dp0"):
        e = per_image_rel(t32[n], t64[n])
        assert e[~floor].max() <= GRAD_TOL / 10, (n, e[~floor].max())
        worst_floor = max(worst_floor, float(e[floor].max()))
    assert worst_floor > GRAD_TOL, worst_floor


def test_fp32_reference_sits_well_inside_the_per_image_bounds(ev):
    worst = {}
    for n in MAPS:
        e = per_image_rel(ev["f32"][n], ev["f64"][n])
        worst[n] = float(e.max())
        assert e.max() <= FWD_TOL / 5, (n, KINDS[int(ev["kinds"][e.argmax()])], e.max())
    for k, g in ev["g64"].items():
        e = float(np.abs(ev["g32"][k].astype(np.float64) - g).max() / np.abs(g).max())
        worst[k] = e
        assert e <= GRAD_TOL / 20, (k, e)
    print("fp32 reference, worst per-image / per-tensor relative error:", worst)
