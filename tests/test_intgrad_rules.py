"""ba3c_amd.intgrad, the statement of integrated-gradients saliency, held to its own definition:
the integer byte rule against a float64 floor, and completeness on the float64 network."""
import numpy as np
import pytest

from atari_frames import atari_frames
from ba3c_amd import intgrad as IG
from oracle import ba3c_oracle as O
from oracle import ba3c_torch_f64 as T
from test_gpu_saliency import autograd_reference


@pytest.mark.parametrize("K", [1, 2, 7, 256])
def test_byte_rule_is_the_float64_floor_and_stays_between_the_ends(K):
    x0, x = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    got = IG.path_bytes(x0, x, K)
    t = 2.0 * np.arange(K).reshape(K, 1, 1) + 1.0
    assert got.shape == (K, 256, 256)
    assert np.array_equal(got, x0 + np.floor((t * (x - x0) + K) / (2.0 * K)))
    assert np.all(got >= np.minimum(x0, x)) and np.all(got <= np.maximum(x0, x))


def test_baselines_and_state_order():
    s = atari_frames(2, 4)
    assert not IG.baseline_numpy(s, "zero").any()
    flat = np.full((1, 84, 84, 4), 93, np.uint8)
    assert np.array_equal(IG.baseline_numpy(flat, "blur"), flat)       # a constant frame is its own blur
    p = IG.path_states(s, 3, "blur")
    assert p.shape == (6, 84, 84, 4) and p.dtype == np.uint8
    assert np.array_equal(p[3:], IG.path_states(s[1:], 3, "blur"))     # state-major, j minor
    assert np.array_equal(IG.path_states(s, 1, "zero"), (s.astype(np.int64) + 1) // 2)   # the one midpoint


def test_completeness_gap_shrinks_with_the_steps():
    """sum(attr) -> V(x) - V(x0) on the float64 network (its own pooling and ReLU decisions at every
    path state): the gap at K = 128 is below the gap at K = 8.  A property of the rule."""
    params = O.init_params(128, 4, 4, seed=2, dtype=np.float64)
    cfg = {"fc_neurons": 128, "fc_splits": 4}
    state = atari_frames(1, 9)
    zeros = lambda n: (np.zeros(n, np.int64), np.zeros(n))

    def value(s):
        return T.loss_and_grads_forced(params, s, *zeros(len(s)), cfg, T.own_decisions(params, s))[1]["pred_value"]
    delta = float(value(state)[0] - value(IG.baseline_numpy(state, "blur"))[0])
    gap = {}
    for K in (8, 128):
        path = IG.path_states(state, K, "blur")
        g = autograd_reference(params, path, zeros(K)[0], np.tile([0.0, 1.0], (K, 1)), T.own_decisions(params, path))
        gap[K] = abs(float(IG.attribution(state, g, K, "blur").sum(dtype=np.float64)) - delta)
        print("K = %d: |sum(attr) - (V(x) - V(x0))| = %.3e of %.3e" % (K, gap[K], abs(delta)))
    assert delta != 0 and gap[128] < gap[8]
