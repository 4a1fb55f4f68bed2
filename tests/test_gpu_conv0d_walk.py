"""conv0d_kernel's persistent walk on the MI355X (tests/conv0d_walk.py states the schedule): at the
smallest batches at which a workgroup runs two and three iterations, on a deal whose scale class
(1, 1e-6, 1e4, black) changes at every step of every workgroup, dX is held element by element to
the derived error model against float64, every image is bit-equal to its own B = 1 run, and the
normwise and `map` assertions of test_gpu_saliency.py hold; dead windows do not set an image's
scale; nothing survives on the handle."""
import functools

import numpy as np
import pytest
import torch

import conv0d_walk as W
from test_gpu_parity import case, engine
from test_gpu_saliency import held_normwise, run_kernel

pytestmark = pytest.mark.gpu


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def walk_engine(B):
    eng = engine(max_batch=max(64, B))        # the cached max_batch = 64 engine covers B = 49 on 256 CUs
    eng.load_params(weights())
    return eng


@functools.lru_cache(maxsize=None)
def weights():
    return case(3, 1)[0]


@functools.lru_cache(maxsize=None)
def walked(iterations):
    """(classes, dp0, c0, the kernel's dX and map) at the smallest batch with `iterations`
    iterations in some workgroup: computed once, shared, never changed."""
    B = W.smallest_batch(cus(), iterations)
    cls = W.deal_classes(B, cus(), both_orders=iterations > 2)
    assert W.classes_ok(cls, B, cus(), both_orders=iterations > 2)
    assert max(len(v) for v in W.walk(B, cus())) == iterations
    dp0, c0 = W.deal("dense", B, scales=np.asarray(W.CLASSES)[cls])
    dx, m = run_kernel(walk_engine(B), dp0, c0)
    return cls, dp0, c0, dx, m


@pytest.mark.parametrize("iterations", [2, 3])
def test_walk_within_error_model_of_float64(iterations):
    """Largest |err| / bound per scale class on an MI355X (256 CUs: B = 25 and 49), measured after
    the bound was fixed: DESIGN.md section 20.1."""
    cls, dp0, c0, dx, m = walked(iterations)
    exact, bound = W.exact_and_bound(dp0, c0, weights()["conv0/W"])
    r = W.ratios(dx, exact, bound)
    print("%d CUs, B=%d, %d iterations: largest |err| / bound per class %r"
          % (cus(), len(dp0), iterations, W.class_report(r, cls)))
    black = cls == W.CLASSES.index(0.0)
    assert not dx[black].any() and not m[black].any()             # exactly zero, map included
    assert dx[~black].any(axis=(1, 2, 3)).all()
    assert W.within_model(dx, exact, bound), np.flatnonzero(~(r <= 1.0))
    held_normwise(dp0, c0, weights()["conv0/W"], dx, m, "walk B=%d" % len(dp0))


@pytest.mark.parametrize("iterations", [2, 3])
def test_walked_image_equals_its_own_run_alone(iterations):
    """A workgroup that used the previous image's kd, or stale LDS rows or partial sums, would
    differ from the image's B = 1 run (one iteration, one image per workgroup)."""
    cls, dp0, c0, dx, m = walked(iterations)
    eng = walk_engine(len(dp0))
    for j in range(len(dp0)):
        one = run_kernel(eng, dp0[j:j + 1], c0[j:j + 1])
        assert np.array_equal(one[0][0], dx[j]) and np.array_equal(one[1][0], m[j]), (j, W.CLASSES[cls[j]])


def test_dead_windows_do_not_set_the_scale():
    """The per-image maximum is over live windows only; training writes dP0 under dead windows
    too.  2^30 under every dead code: bit-equal to the unscaled run."""
    eng = walk_engine(3)
    dp0, c0 = W.deal("dense", 3)
    loud = np.where(c0 == 255, dp0 * np.float32(2.0 ** 30), dp0)
    assert (c0 == 255).any(axis=(1, 2, 3)).all() and np.abs(loud).max() > 2.0 ** 30
    a, b = run_kernel(eng, dp0, c0), run_kernel(eng, loud, c0)
    assert a[0].any() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_nothing_survives_on_the_handle_from_a_bright_walk():
    """A bright three-iteration batch fills every max partial of the handle; a B = 1 image at 1e-6
    follows and equals, bit for bit, that of a handle that never saw the batch (stale partials
    above `batch`)."""
    from ba3c_amd.engine import Ba3cEngine
    B = W.smallest_batch(cus(), 3)
    bright = W.deal("dense", B, scales=np.full(B, 1e4))
    dim = W.deal("dense", 1, seed=5, scales=[1e-6])
    eng = walk_engine(B)
    run_kernel(eng, *bright)
    after = run_kernel(eng, *dim)
    fresh = Ba3cEngine(num_actions=4, channels=4, fc_neurons=128, fc_splits=4, max_batch=eng.max_batch)
    fresh.load_params(weights())
    alone = run_kernel(fresh, *dim)
    assert alone[0].any() and np.array_equal(after[0], alone[0]) and np.array_equal(after[1], alone[1])
