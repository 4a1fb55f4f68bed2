"""Integrated-gradients saliency on the MI355X: ba3c_ig_states against intgrad.path_states bit for
bit, Ba3cEngine.integrated_grads against intgrad's rule over float64 gradients with
test_gpu_saliency's bound for input_grads, its independence of the chunk seams, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ba3c_amd import intgrad as IG
from test_gpu_parity import GRAD_TOL, case, dev, engine, gpu_decisions, rel
from test_gpu_saliency import autograd_reference

pytestmark = pytest.mark.gpu
ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
SEEDS = {"v": (0.0, 1.0), "pi": (1.0, 0.0)}


@functools.lru_cache(maxsize=None)
def deal(n, K, baseline):
    """(random states uint8 [n,84,84,4] with blocks of 0 and of 255, their n * K path states)."""
    rs = np.random.RandomState(n + K)
    s = rs.randint(0, 256, size=(n, 84, 84, 4)).astype(np.uint8)
    s[:, 10:30, 5:40], s[:, 50:84, 60:84], s[:, 0:3, 0:9, 1:3] = 0, 255, 255
    return s, IG.path_states(s, K, baseline)


@pytest.mark.parametrize("n,K,baseline,chunk", [(1, 1, "zero", 1), (3, 7, "zero", 5), (2, 7, "blur", 4),
                                                (1, 256, "blur", 100)])
def test_path_states_are_the_rule_bit_for_bit(n, K, baseline, chunk):
    """Every chunk of the n * K path states, seams inside a state's K points included, and the guard
    row after it keeps its 0xAB.  On the inputs alone: both extremes of a byte, the largest step
    d = 255 from the zero baseline, and both signs of d from the blurred one."""
    from ba3c_amd import _lib as L
    lib = L.load()
    s, ref = deal(n, K, baseline)
    d = s.astype(np.int64) - IG.baseline_numpy(s, baseline)
    assert (s == 0).any() and (s == 255).any() and (d == 0).any() and d.max() >= 128
    assert d.max() == 255 if baseline == "zero" else d.min() <= -128
    src = dev(s)
    for first in range(0, n * K, chunk):
        count = min(chunk, n * K - first)
        out = torch.full((count + 1, 84, 84, 4), 0xAB, dtype=torch.uint8, device="cuda")
        L.check(lib.ba3c_ig_states(None, ptr(src), n, K, IG.BASELINES[baseline], first, count, ptr(out)))
        out = out.cpu().numpy()
        assert np.array_equal(out[:count], ref[first:first + count]), (first, count)
        assert np.all(out[count] == 0xAB), (first, count)          # nothing past the chunk


@pytest.mark.parametrize("kind", sorted(SEEDS))
@pytest.mark.parametrize("n,K,max_batch", [(2, 5, 4), (3, 4, 32)])
def test_attributions_match_the_float64_rule(n, K, max_batch, kind):
    """The oracle: intgrad.attribution over float64 autograd gradients at the same uint8 path
    states, pooling and ReLU decisions those of the HIP path on them (one input_grads call of all
    n * K).  Normwise per state, the bound of input_grads: attr is a fixed linear combination of K
    such gradients."""
    params, state, action, _, _ = case(70 + n, n, wscale=2.0)
    seeds = np.tile(np.float32(SEEDS[kind]), (n, 1))
    eng = engine(max_batch=max_batch)
    eng.load_params(params)
    got = eng.integrated_grads(dev(state), dev(action), dev(seeds), steps=K, baseline="blur").cpu().numpy()
    path, big = IG.path_states(state, K, "blur"), engine(max_batch=64)
    big.load_params(params)
    big.input_grads(dev(path), dev(np.repeat(action, K)), dev(np.repeat(seeds, K, axis=0)))
    g = autograd_reference(params, path, np.repeat(action, K), np.repeat(seeds, K, axis=0), gpu_decisions(big, n * K)[0])
    ref = IG.attribution(state, g, K, "blur")
    assert got.shape == (n, 84, 84, 4) and got.dtype == np.float32
    for b in range(n):
        print("%s n=%d K=%d max_batch=%d state %d: rel %.3e" % (kind, n, K, max_batch, b, rel(got[b], ref[b])))
        assert ref[b].any() and rel(got[b], ref[b]) < GRAD_TOL


def test_attributions_do_not_depend_on_the_chunk_seams():
    params, state, action, _, _ = case(75, 2, wscale=2.0)
    seeds = dev(np.random.RandomState(3).normal(size=(2, 2)).astype(np.float32))
    got = []
    for max_batch in (3, 8, 64):
        eng = engine(max_batch=max_batch)
        eng.load_params(params)
        got.append(eng.integrated_grads(dev(state), dev(action), seeds, steps=5, baseline="zero"))
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]) and got[0].any()


BUF = (ctypes.c_int32 * 64)()
BASE = ctypes.addressof(BUF) + -ctypes.addressof(BUF) % 16
# (state, n, steps, baseline, first, count, out) and the keyword of the refusal; "+N": the aligned buffer + N
REFUSALS = [((None, 2, 7, 0, 0, 4, "+0"), b"null"), (("+0", 2, 7, 0, 0, 4, None), b"null"),
            (("+0", 0, 7, 0, 0, 4, "+0"), b"n must"), (("+0", 2, 0, 0, 0, 4, "+0"), b"steps"),
            (("+0", 2, 257, 0, 0, 4, "+0"), b"steps"), (("+0", 2, 7, 2, 0, 4, "+0"), b"baseline"),
            (("+0", 2, 7, -1, 0, 4, "+0"), b"baseline"), (("+0", 2, 7, 1, -1, 4, "+0"), b"chunk"),
            (("+0", 2, 7, 1, 0, 0, "+0"), b"chunk"), (("+0", 2, 7, 1, 11, 4, "+0"), b"chunk"),
            (("+0", 2, 7, 1, 14, 1, "+0"), b"chunk"), (("+8", 2, 7, 1, 0, 4, "+0"), b"aligned"),
            (("+0", 2, 7, 1, 0, 4, "+4"), b"aligned"), (("+0", 0, 0, 0, 0, 4, "+0"), b"n must")]


@pytest.mark.parametrize("args,word", REFUSALS)
def test_ig_states_refusals(args, word):
    """Each is refused before any GPU call (the pointers are host addresses), the earlier check first."""
    from ba3c_amd import _lib as L
    lib = L.load()
    args = [ctypes.c_void_p(BASE + int(a)) if isinstance(a, str) else a for a in args]
    assert lib.ba3c_ig_states(None, *args) == 1
    assert word in lib.ba3c_last_error(), lib.ba3c_last_error()
