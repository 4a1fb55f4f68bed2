"""ba3c_amd.perturb, the fixed-point statement of perturbation saliency, held to its own
consequences and to the float64 formula I (1 - M) + A(I) M."""
import numpy as np
import pytest

from atari_frames import atari_frames
from ba3c_amd import perturb as P

RANDOM = np.random.RandomState(1).randint(0, 256, size=(1, 84, 84, 4)).astype(np.uint8)


@pytest.mark.parametrize("level", [0, 1, 128, 255])
def test_weights_sum_to_one_and_a_constant_image_is_reproduced(level):
    assert P.WEIGHTS.sum() == 4096 and P.WEIGHTS.shape == (19,) and P.MASK_Q[0] == 256
    assert np.all(P.perturb_numpy(np.full((1, 84, 84, 4), level, np.uint8)) == level)


@pytest.mark.parametrize("state", [RANDOM, atari_frames(1, 5)], ids=["random", "atari"])
def test_within_one_grey_level_of_the_float64_formula(state):
    """A: the float64 Gaussian (sigma 3) over the same 19 reflected taps; M: the float64 Gaussian
    (sigma 5) over the same 31 x 31 support.  The bound of 1 is the rounding of the Q12 / Q8 tables
    plus the final rounding (measured: 0.81 random, 0.62 Atari-like)."""
    t, ar = np.arange(-9, 10), np.arange(84)
    w = np.exp(-t * t / 18.0) / np.exp(-t * t / 18.0).sum()
    x = state.astype(np.float64)
    a = sum(wi * x[:, :, P.reflect(ar + ti)] for wi, ti in zip(w, t))
    a = sum(wi * a[:, P.reflect(ar + ti)] for wi, ti in zip(w, t))
    got = P.perturb_numpy(state).reshape(P.NC, 84, 84, 4)
    worst = 0.0
    for k, (cy, cx) in enumerate(P.centres()):
        axis = lambda c: np.where(np.abs(ar - c) <= 15, np.exp(-(ar - c) ** 2 / 50.0), 0.0)
        m = np.outer(axis(cy), axis(cx))[:, :, None]
        worst = max(worst, np.abs(got[k] - (x[0] * (1 - m) + a[0] * m)).max())
    print("largest deviation %.3f grey levels" % worst)
    assert worst <= 1.0


def test_far_pixels_and_older_frames_are_untouched():
    all4 = P.perturb_numpy(RANDOM).reshape(P.NC, 84, 84, 4)
    for k, (cy, cx) in enumerate(P.centres()):
        far = (np.abs(np.arange(84) - cy)[:, None] > 15) | (np.abs(np.arange(84) - cx)[None, :] > 15)
        assert np.array_equal(all4[k][far], RANDOM[0][far]) and not np.array_equal(all4[k], RANDOM[0])
    new = P.perturb_numpy(RANDOM, newest=True).reshape(P.NC, 84, 84, 4)
    assert np.array_equal(new[..., :3], np.broadcast_to(RANDOM[..., :3], new[..., :3].shape))
    assert np.array_equal(new[..., 3], all4[..., 3])


def test_upsample_reproduces_the_grid_and_repeats_the_last_cell():
    g = np.random.RandomState(2).rand(2, 17, 17)
    u = P.upsample_numpy(g)
    assert u.dtype == np.float32 and np.array_equal(u[:, ::5, ::5], g.astype(np.float32))
    assert np.all(u[:, 80:, :] == u[:, 80:81, :]) and np.all(u[:, :, 80:] == u[:, :, 80:81])


def test_the_recorder_parses_the_perturbation_maps():
    from ba3c_amd.record import record_parser
    for which in ("pv", "ppi"):
        assert record_parser().parse_args(["--saliency", which]).saliency == which
    with pytest.raises(SystemExit):
        record_parser().parse_args(["--saliency", "x"])
