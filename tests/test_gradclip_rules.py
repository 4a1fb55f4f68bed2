"""The rule of the global-norm gradient clip (ba3c_amd/gradclip.py), the oracle of the two HIP
launches behind ba3c_clip_grads_global: pure numpy, no GPU."""
import math

import numpy as np
import pytest

from ba3c_amd import gradclip as G

f32, f64 = np.float32, np.float64


def tensors(seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    return [(rs.normal(size=n) * scale).astype(f32) for n in (1, 31, 4096, 4097, 20000)]


def exact_norm(ts):
    return math.sqrt(math.fsum(float(x) * float(x) for t in ts for x in np.asarray(t, f64).reshape(-1)))


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def test_the_norm_is_the_square_root_of_the_exact_sum():
    ts = tensors()
    assert G.global_norm_numpy(ts) == exact_norm(ts)
    assert G.global_norm_numpy([]) == 0.0


@pytest.mark.parametrize("max_norm", [0.5, 7.0, 1e-3])
def test_the_norm_after_is_the_smaller_of_norm_and_max_norm(max_norm):
    ts = tensors(1)
    out, norm, f = G.clip_numpy(ts, max_norm)
    assert norm > max_norm and f == max_norm / norm
    after = exact_norm(out)                                  # of the float64 products
    assert abs(after - min(norm, max_norm)) <= 1e-12 * min(norm, max_norm)
    big = 10.0 * norm
    out, norm2, f2 = G.clip_numpy(ts, big)
    assert norm2 == norm and f2 == 1.0
    assert abs(exact_norm(out) - min(norm, big)) <= 1e-12 * norm


def test_agreement_with_the_textbook_form_where_clipped():
    """tf.clip_by_global_norm: t * c * min(1 / norm, 1 / c)."""
    ts = tensors(2, scale=3.0)
    c = 0.5
    out, norm, f = G.clip_numpy(ts, c)
    assert f < 1.0
    for t, o in zip(ts, out):
        want = t.astype(f64) * c * min(1.0 / norm, 1.0 / c)
        assert np.all(np.abs(o - want) <= 1e-15 * np.abs(want))


def test_an_unclipped_input_comes_back_with_its_float32_bits():
    ts = tensors(3, scale=1e-3)
    ts[2][5] = f32(-0.0)
    ts[2][6] = np.finfo(f32).tiny / f32(8)                  # a subnormal
    out, norm, f = G.clip_numpy(ts, 2.0 * G.global_norm_numpy(ts))
    assert f == 1.0
    for t, o in zip(ts, out):
        assert o.dtype == f64 and np.array_equal(bits(o.astype(f32)), bits(t))
    # at the threshold itself nothing is clipped either: norm > max_norm is false
    out, norm, f = G.clip_numpy(ts, G.global_norm_numpy(ts))
    assert f == 1.0


def test_a_zero_gradient_stays_zero():
    ts = [np.zeros(n, f32) for n in (1, 100)]
    out, norm, f = G.clip_numpy(ts, 0.5)
    assert norm == 0.0 and f == 1.0
    assert all(not o.any() for o in out)


def test_one_element_that_dominates():
    ts = tensors(4, scale=1e-6)
    ts[4][123] = f32(3e18)                                   # its square, ~9e36, is exact in float64
    big = float(ts[4][123])
    out, norm, f = G.clip_numpy(ts, 0.5)
    assert abs(norm - big) <= 1e-12 * big and f == 0.5 / norm
    assert abs(out[4][123] - 0.5) <= 1e-12
    others = out[4].copy()
    others[123] = 0.0
    assert exact_norm(out[:4] + [others]) < 1e-20            # everything else went with it


def test_a_nan_element_leaves_the_factor_at_one():
    ts = tensors(5)
    ts[1][3] = np.nan
    out, norm, f = G.clip_numpy(ts, 0.5)
    assert math.isnan(norm) and f == 1.0
    for t, o in zip(ts, out):
        assert np.array_equal(bits(o.astype(f32)), bits(t))    # the NaN stays where it is


def test_an_infinite_norm_clips_to_zero():
    ts = tensors(6)
    ts[0][0] = f32(np.inf)
    with np.errstate(invalid="ignore"):
        out, norm, f = G.clip_numpy(ts, 0.5)
    assert norm == np.inf and f == 0.0
    assert not out[2].any() and math.isnan(out[0][0])


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_max_norm_must_be_finite_and_positive(bad):
    with pytest.raises(ValueError):
        G.clip_numpy(tensors(), bad)
    from ba3c_amd.model_desc import ClipByGlobalNorm
    with pytest.raises(ValueError):
        ClipByGlobalNorm(bad)
