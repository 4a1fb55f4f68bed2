"""Perturbation saliency on the MI355X: ba3c_perturb_states against perturb.perturb_numpy bit for
bit, ba3c_perturb_scores against scores_numpy + upsample_numpy, Ba3cEngine.perturb_maps end to end
and the recorder's --saliency pv."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from atari_frames import atari_frames
from ba3c_amd import perturb as P

pytestmark = pytest.mark.gpu
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
PIXELS = [(0, 0), (0, 83), (83, 83), (41, 41), (80, 5)]    # every edge's reflection, the last grid row


@functools.lru_cache(maxsize=None)
def deal(kind, n, newest):
    """(states uint8 [n,84,84,4], their n * 289 perturbed states by the rule)."""
    if kind == "random":
        s = np.random.RandomState(n).randint(0, 256, size=(n, 84, 84, 4)).astype(np.uint8)
    elif kind == "atari":
        s = atari_frames(n, 3)
    else:
        s = np.full((n, 84, 84, 4), 255 if kind == "white" else 0, np.uint8)
        if kind == "pixels":
            for k, (y, x) in enumerate(PIXELS):
                s[k % n, y, x] = (255, 200, 100, 50 + k)
    return s, P.perturb_numpy(s, newest)


def held_bit_for_bit(kind, n, newest, chunks):
    """Each chunk (first, count) of the n * 289 perturbed states equals the rule's, and the guard
    row after it keeps its 0xAB.  -> the chunks' outputs, concatenated."""
    from ba3c_amd import _lib as L
    lib = L.load()
    s, ref = deal(kind, n, newest)
    src = dev(s)
    got = []
    for first, count in chunks or ((0, n * P.NC),):
        out = torch.full((count + 1, 84, 84, 4), 0xAB, dtype=torch.uint8, device="cuda")
        L.check(lib.ba3c_perturb_states(None, ptr(src), n, first, count, int(newest), ptr(out)))
        out = out.cpu().numpy()
        assert np.array_equal(out[:count], ref[first:first + count]), (first, count)
        assert np.all(out[count] == 0xAB), (first, count)      # nothing past the chunk
        got.append(out[:count])
    return np.concatenate(got), ref


@pytest.mark.parametrize("chunks", [None, ((0, 100), (100, 189))], ids=["whole", "chunks"])
@pytest.mark.parametrize("newest", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", ["random", "atari", "black", "white", "pixels"])
def test_perturbed_states_are_the_rule_bit_for_bit(kind, n, newest, chunks):
    held_bit_for_bit(kind, n, newest, chunks)


# Chunk seams at n = 3 (867 perturbed states; a state is 289 = 17 centre rows of 17; the kernel's
# first workgroup is (first // 17) // 17, first // 17 % 17).  Ba3cEngine.perturb_maps makes all of
# these whenever max_batch does not divide 289.
SEAMS = {
    "crosses_state_0_to_1": ((280, 20),),
    "single_states_at_a_state_boundary_and_the_end": ((288, 1), (289, 1), (866, 1)),
    "one_centre_row": ((306, 17),),
    "one_centre_row_and_a_state_either_side": ((305, 19),),
    "inside_state_1_to_the_end": ((577, 290),),
}
SWEEP = tuple((first, min(64, 867 - first)) for first in range(0, 867, 64))   # the recorder's max_batch


@pytest.mark.parametrize("name", sorted(SEAMS) + ["sweep_of_64"])
@pytest.mark.parametrize("newest", [False, True])
@pytest.mark.parametrize("kind", ["random", "pixels"])
def test_chunk_seams_are_the_rule_bit_for_bit(kind, newest, name):
    got, ref = held_bit_for_bit(kind, 3, newest, SWEEP if name == "sweep_of_64" else SEAMS[name])
    if name == "sweep_of_64":
        assert SWEEP[-1] == (832, 35) and len(SWEEP) == 14     # a ragged last chunk
        assert np.array_equal(got, ref)                        # the sweep, concatenated, is the whole


def within_rounding(got, grid):
    """|map - ref| <= 2^-23 max |ref| per state, and zero where the reference is zero: both sides
    round one float64 value, formed in the same order, to float32.  -> the largest ratio."""
    ref = P.upsample_numpy(grid)
    top = np.abs(ref).max(axis=(1, 2), keepdims=True).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 2.0 ** -23 * top) and np.all(got[ref == 0] == 0)
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(top, 1e-300)).max())


@pytest.mark.parametrize("kind", ["one", "equal", "dense"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("A", [1, 4, 18])
def test_scores_and_map_match_float64(A, n, kind):
    from ba3c_amd import _lib as L
    lib = L.load()
    rs = np.random.RandomState(A + n)
    for mag in (1e-3, 1.0, 1e3):
        p0, v0 = (rs.rand(n, A) * mag).astype(np.float32), (rs.randn(n) * mag).astype(np.float32)
        p, v = np.repeat(p0, P.NC, axis=0), np.repeat(v0, P.NC)
        if kind == "one":
            p[(n - 1) * P.NC + 137], v[(n - 1) * P.NC + 137] = p0[0] * 0.5 + np.float32(mag / 3), v0[0] + np.float32(mag)
        elif kind == "dense":
            p, v = (rs.rand(n * P.NC, A) * mag).astype(np.float32), (rs.randn(n * P.NC) * mag).astype(np.float32)
        for which in (0, 1):
            m = torch.full((n, 84, 84), np.nan, dtype=torch.float32, device="cuda")
            g = torch.full((n, 17, 17), np.nan, dtype=torch.float64, device="cuda")
            ins = [dev(a) for a in (p0, v0, p, v)]
            L.check(lib.ba3c_perturb_scores(None, *[ptr(t) for t in ins], n, A, which, ptr(m),
                                            ptr(g if mag == 1.0 else None)))
            ref = P.scores_numpy(p0, v0, p, v, which)
            print("A=%d n=%d %s mag %g which %d: %.3f of the bound" % (A, n, kind, mag, which, within_rounding(m.cpu().numpy(), ref)))
            assert (not ref.any()) == (kind == "equal")
            if mag == 1.0:
                np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=1e-14, atol=0)


def test_perturb_maps_end_to_end_and_independent_of_max_batch():
    from ba3c_amd.engine import Ba3cEngine
    from ba3c_amd import saliency as S
    state = atari_frames(2, 11)
    engines = [Ba3cEngine(num_actions=4, channels=4, fc_neurons=128, fc_splits=4, max_batch=mb) for mb in (64, 640)]
    for e in engines:
        e.init_params(seed=3)
    p0, _, v0 = engines[1].forward(dev(state))
    p, _, v = engines[1].forward(dev(P.perturb_numpy(state)))
    for which, fn in enumerate((S.perturb_value_map, S.perturb_policy_map)):
        small, big = (fn(e, dev(state)).cpu().numpy() for e in engines)
        assert np.array_equal(small, big) and small.shape == (2, 84, 84) and small.any()
        ref = P.scores_numpy(p0.cpu().numpy(), v0.cpu().numpy(), p.cpu().numpy(), v.cpu().numpy(), which)
        print("which %d: %.3f of the bound" % (which, within_rounding(big, ref)))
    with pytest.raises(ValueError, match="channels == 4"):
        Ba3cEngine(num_actions=4, channels=12, fc_neurons=128, fc_splits=4, max_batch=4).perturb_maps(
            dev(np.zeros((1, 84, 84, 12), np.uint8)), "v")


def test_recorder_stores_the_perturbation_value_map_of_each_decision():
    from ba3c_amd import boxing as K
    from ba3c_amd import saliency as S
    from ba3c_amd.engine import Ba3cEngine
    from ba3c_amd.flags import GRID_BOXING
    from ba3c_amd.record import record_episodes
    eng = Ba3cEngine(num_actions=18, channels=4, fc_neurons=128, fc_splits=4, max_batch=64)
    eng.init_params(seed=1)
    torch.manual_seed(0)
    ep, = record_episodes(eng, GRID_BOXING, 1, n_envs=1, seed=2, limit=6, scale=1, saliency="pv")
    T = ep.steps
    assert ep.saliency.shape == (T, 84, 84) and np.isfinite(ep.saliency).all() and (ep.saliency >= 0).all()
    frames = K.render_numpy(ep.replay()[0][:T])                # the frame each decision saw
    for t in range(T):
        k = min(t + 1, 4)
        state = np.zeros((1, 84, 84, 4), np.uint8)
        state[0, :, :, 4 - k:] = frames[t + 1 - k:t + 1].transpose(1, 2, 0)
        assert np.array_equal(S.perturb_value_map(eng, dev(state), newest=True).cpu().numpy()[0], ep.saliency[t])
