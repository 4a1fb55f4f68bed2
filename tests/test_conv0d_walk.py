"""tests/conv0d_walk.py on the host: the walk schedule of conv0's input-gradient kernel, the deal
of scale classes over it, and the checks of tests/test_gpu_conv0d_walk.py shown to reject a wrong
walk (a numpy mirror that quantises a band at the previous image's exponent) which the per-image
normwise check on a same-binade batch lets through."""
import numpy as np
import pytest

import conv0d_walk as W
from oracle import ba3c_oracle as O

GRAD_TOL = 1e-4                  # test_gpu_parity's
CUS = (64, 104, 256, 304)


def rel(a, b):                   # test_gpu_parity.rel
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("cus", CUS)
def test_every_band_is_visited_once_and_the_iteration_counts_are_right(cus):
    for B in (1, 3, W.smallest_batch(cus, 2), W.smallest_batch(cus, 3), W.smallest_batch(cus, 3) + 5):
        v = W.walk(B, cus)
        grid, bands = min(21 * B, 2 * cus), 21 * B
        assert len(v) == grid
        assert sorted(p for wg in v for p in wg) == [(i, r) for i in range(B) for r in range(21)]
        assert [len(wg) for wg in v] == [bands // grid + (w < bands % grid) for w in range(grid)]
        for w, wg in enumerate(v):                                # band w, w + grid, ...
            assert [21 * i + r for i, r in wg] == list(range(w, bands, grid))


@pytest.mark.parametrize("cus", CUS)
def test_smallest_batches(cus):
    for it in (1, 2, 3):
        B = W.smallest_batch(cus, it)
        assert max(len(wg) for wg in W.walk(B, cus)) == it
        assert B == 1 or max(len(wg) for wg in W.walk(B - 1, cus)) == it - 1
        assert 21 * B > (it - 1) * 2 * cus >= 21 * (B - 1)        # the closed form
    if cus == 256:
        assert (W.smallest_batch(cus, 2), W.smallest_batch(cus, 3)) == (25, 49)


@pytest.mark.parametrize("cus", CUS)
def test_deal_classes_changes_the_scale_at_every_step_of_every_workgroup(cus):
    B = W.smallest_batch(cus, 3)
    cls = W.deal_classes(B, cus)
    zero = W.CLASSES.index(0.0)
    seen = set()
    for wg in W.walk(B, cus):                                     # the property itself, restated
        for (a, _), (b, _) in zip(wg, wg[1:]):
            if a != b:
                assert cls[a] != cls[b], (a, b)
                seen.add((cls[a] == zero, cls[b] == zero))
    assert {(True, False), (False, True)} <= seen
    assert set(cls.tolist()) == set(range(len(W.CLASSES)))        # every class is dealt
    # at the two-iteration batch a single pair of images shares a workgroup: it differs
    B2 = W.smallest_batch(cus, 2)
    cls2 = W.deal_classes(B2, cus, both_orders=False)
    assert W.steps(B2, cus) and all(cls2[a] != cls2[b] for a, b in W.steps(B2, cus))


def test_deal_classes_refuses_periods_that_repeat_along_the_walk(monkeypatch):
    """At 256 CUs a workgroup's consecutive images are 24 or 25 apart: periods 4 and 5 give some of
    them the same class, and a search that has only those raises."""
    for period in (4, 5):
        assert not W.classes_ok((np.arange(49) % period) % 4, 49, 256)
    monkeypatch.setattr(W, "PERIODS", (4, 5))
    with pytest.raises(ValueError):
        W.deal_classes(49, 256)


# ---- the checks reject a wrong walk ---------------------------------------------------------------
MIRROR_CUS = 64                  # three iterations at B = 13: the mirror's float64 sums stay small
_CASE = {}


def _case(name):
    """(dp0, c0, W0, classes, exact, bound) of the mixed deal and of the same-binade one, each
    computed once and never changed."""
    if not _CASE:
        B = W.smallest_batch(MIRROR_CUS, 3)
        w0 = O.init_params(128, 4, 4, seed=3, dtype=np.float32)["conv0/W"]
        cls = W.deal_classes(B, MIRROR_CUS)
        for key, scales in (("mixed", np.asarray(W.CLASSES)[cls]), ("same", np.ones(B))):
            dp0, c0 = W.deal("dense", B, scales=scales)
            _CASE[key] = (dp0, c0, w0, cls) + W.exact_and_bound(dp0, c0, w0)
    return _CASE[name]


def test_model_accepts_the_right_walk_and_float32_rounding():
    dp0, c0, w0, cls, exact, bound = _case("mixed")
    got = W.mirror(dp0, c0, w0, MIRROR_CUS)
    r = W.ratios(got, exact, bound)
    print("mirror, largest |err| / bound per class:", W.class_report(r, cls))
    assert W.within_model(got, exact, bound) and r.max() > 0
    assert W.within_model(exact.astype(np.float32), exact, bound)
    assert not got[cls == W.CLASSES.index(0.0)].any()
    for b in range(len(dp0)):                                     # and it is the walk's own image alone
        one = W.mirror(dp0[b:b + 1], c0[b:b + 1], w0, MIRROR_CUS)
        assert np.array_equal(one[0], got[b])


def test_model_rejects_the_previous_images_exponent_on_the_dim_image():
    dp0, c0, w0, cls, exact, bound = _case("mixed")
    bad = W.mirror(dp0, c0, w0, MIRROR_CUS, stale=True)
    r = W.ratios(bad, exact, bound)
    print("stale walk, |err| / bound per class:", W.class_report(np.where(np.isnan(r), np.inf, r), cls))
    dim = cls == W.CLASSES.index(1e-6)
    assert not W.within_model(bad, exact, bound)
    assert not np.all(r[dim] <= 1.0)                              # on a 1e-6 image (a nan fails too)
    # a black image after a bright one is no longer exactly zero, or a bright one after it is lost
    good = W.mirror(dp0, c0, w0, MIRROR_CUS)
    assert any(not np.array_equal(W.mirror(dp0[b:b + 1], c0[b:b + 1], w0, MIRROR_CUS)[0], bad[b])
               for b in np.flatnonzero(dim))                      # slot independence sees it too
    assert not np.array_equal(good, bad)


def test_normwise_check_on_a_same_binade_batch_lets_the_wrong_walk_through():
    """What tests/test_gpu_saliency.py asserts at B <= 4: rel < GRAD_TOL per image on a dense N(0,1)
    deal.  Every image's exponent is the same there, so the wrong walk gives the same planes."""
    dp0, c0, w0, _, exact, bound = _case("same")
    bad = W.mirror(dp0, c0, w0, MIRROR_CUS, stale=True)
    assert all(rel(bad[b], exact[b]) < GRAD_TOL for b in range(len(dp0)))
    assert W.within_model(bad, exact, bound)                      # and so does the model there: the deal matters


def test_amax_exp_and_split_restate_the_kernel():
    assert [W.amax_exp(a) for a in (0.0, 1.0, 2.0 ** 14, 2.0 ** 15 - 1, 4.5e-6, 4.5e4, 2.0 ** -126)] == \
        [0, 14, 0, 0, 32, -1, 100]
    x = np.float32([1.0 + 2.0 ** -12, 3e-5, 0.0, -7.25])
    hi, lo = W.split2(x, 3)
    # 22 significant bits, or fp16's absolute floor (half a subnormal spacing, 2^-25)
    assert np.all(np.abs(hi + lo - x.astype(np.float64) * 8) <= np.maximum(2.0 ** -22 * np.abs(x) * 8, 2.0 ** -25))
    assert lo[0] == 2.0 ** -9 and np.isinf(W.split2(np.float32(1e4), 32)[0])
