"""Every refusal of ba3c_train_grads_ppo and ba3c_sample_logp.  A refusal returns before any GPU
call, so none of this needs a GPU: return code 1 (BA3C_ERR_INVALID), the keyword of the failed
check in ba3c_last_error(), and for a call with two faults the earlier check's message."""
import ctypes

import pytest

# the arguments after the handle / stream, in the order of include/ba3c.h
GRADS = ("params", "state", "action", "rows", "batch", "beta", "clip", "ws", "grads", "scalars",
         "ratio", "phase")
SAMPLE = ("probs", "pi", "u", "batch", "A", "actions", "logp", "flag")

# (name, the arguments that commit the fault, the keyword of its message), in the order the
# checks run; "+N": the aligned buffer plus N bytes
GRADS_FAULTS = [
    ("null rows", {"rows": None}, b"rows"),
    ("rows + 4", {"rows": "+4"}, b"rows"),
    ("rows + 8", {"rows": "+8"}, b"rows"),
    ("ratio + 4", {"ratio": "+4"}, b"ratio"),
    ("ratio + 8", {"ratio": "+8"}, b"ratio"),
    ("clip 0", {"clip": 0.0}, b"clip_eps"),
    ("clip 1", {"clip": 1.0}, b"clip_eps"),
    ("clip -0.2", {"clip": -0.2}, b"clip_eps"),
    ("clip 3", {"clip": 3.0}, b"clip_eps"),
    ("clip nan", {"clip": float("nan")}, b"clip_eps"),
    ("phase -1", {"phase": -1}, b"phase"),
    ("phase 5", {"phase": 5}, b"phase"),
    ("phase 3", {"phase": 3}, b"phase"),             # the deferred and held reductions are gone:
    ("phase 4", {"phase": 4}, b"phase"),             # a pass is whole (0) or split in two (1, 2)
    ("null params", {"params": None}, b"pointer"),
    ("state + 8", {"state": "+8"}, b"pointer"),
    ("null action", {"action": None}, b"pointer"),
    ("null workspace", {"ws": None}, b"pointer"),
    ("grads + 4", {"grads": "+4"}, b"pointer"),
    ("batch 0", {"batch": 0}, b"batch"),
    ("batch over max_batch", {"batch": 33}, b"batch"),
]
GRADS_ORDER = [({"rows": None}, b"rows"), ({"ratio": "+4"}, b"ratio"), ({"clip": 1.5}, b"clip_eps"),
               ({"phase": 7}, b"phase"), ({"params": None}, b"pointer"), ({"batch": 0}, b"batch")]

SAMPLE_FAULTS = [
    ("null probs", {"probs": None}, b"null pointer"),
    ("null u", {"u": None}, b"null pointer"),
    ("null actions", {"actions": None}, b"null pointer"),
    ("null pi", {"pi": None}, b"pi or logp"),
    ("null logp", {"logp": None}, b"pi or logp"),
    ("batch -1", {"batch": -1}, b"shape"),
    ("A 0", {"A": 0}, b"shape"),
    ("A 32", {"A": 32}, b"shape"),
]
SAMPLE_ORDER = [({"probs": None}, b"null pointer"), ({"pi": None}, b"pi or logp"), ({"A": 0}, b"shape")]


@pytest.fixture(scope="module")
def lib():
    from ba3c_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def handle(lib):
    from ba3c_amd import _lib as L
    c = L.Ba3cConfig(max_batch=32, channels=4, fc_neurons=128, fc_splits=4, num_actions=4,
                     replace_with_conv=1, ps=1)
    h = ctypes.c_void_p()
    assert lib.ba3c_create(ctypes.byref(c), ctypes.byref(h)) == 0, lib.ba3c_last_error()
    yield h
    lib.ba3c_destroy(h)


@pytest.fixture(scope="module")
def base():
    buf = (ctypes.c_int32 * 64)()
    addr = ctypes.addressof(buf)
    addr += -addr % 16
    assert addr + 32 <= ctypes.addressof(buf) + ctypes.sizeof(buf)
    return buf, addr                                 # buf is returned to keep it alive


def _args(base, names, defaults, faults):
    args = dict(defaults)
    for k, v in faults.items():
        assert k in args, k
        args[k] = ctypes.c_void_p(base[1] + int(v)) if isinstance(v, str) else v
    return [args[k] for k in names]


def _grads(lib, handle, base, **faults):
    p = ctypes.c_void_p(base[1])
    d = dict(params=p, state=p, action=p, rows=p, batch=4, beta=0.01, clip=0.2, ws=p, grads=p,
             scalars=None, ratio=p, phase=0)
    return lib.ba3c_train_grads_ppo(handle, None, *_args(base, GRADS, d, faults))


def _sample(lib, handle, base, **faults):
    p = ctypes.c_void_p(base[1])
    d = dict(probs=p, pi=p, u=p, batch=4, A=4, actions=p, logp=p, flag=None)
    return lib.ba3c_sample_logp(None, *_args(base, SAMPLE, d, faults))


CALLS = {"ba3c_train_grads_ppo": (_grads, GRADS_FAULTS, GRADS_ORDER),
         "ba3c_sample_logp": (_sample, SAMPLE_FAULTS, SAMPLE_ORDER)}


@pytest.mark.parametrize("fn", sorted(CALLS))
def test_every_refusal(lib, handle, base, fn):
    call, faults, _ = CALLS[fn]
    for name, f, word in faults:
        assert call(lib, handle, base, **f) == 1, name
        assert word in lib.ba3c_last_error(), (name, lib.ba3c_last_error())


@pytest.mark.parametrize("fn", sorted(CALLS))
def test_the_earlier_check_is_reported(lib, handle, base, fn):
    call, _, order = CALLS[fn]
    for i, (first, word) in enumerate(order):
        for later, later_word in order[i + 1:]:
            assert call(lib, handle, base, **dict(first, **later)) == 1
            msg = lib.ba3c_last_error()
            assert word in msg and later_word not in msg, (first, later, msg)


def test_a_null_handle_and_a_null_ratio(lib, base):
    assert _grads(lib, None, base) == 1 and b"pointer" in lib.ba3c_last_error()
    # ratio is optional: with none given the call gets as far as the next check
    assert _grads(lib, None, base, ratio=None, phase=9) == 1 and b"phase" in lib.ba3c_last_error()


@pytest.mark.parametrize("phase", [-1, 3, 4, 5])
def test_train_grads_phase_refuses_every_phase_but_0_1_2(lib, handle, base, phase):
    p = ctypes.c_void_p(base[1])
    assert lib.ba3c_train_grads_phase(handle, None, p, p, p, p, 4, 0.01, p, p, None, phase) == 1
    msg = lib.ba3c_last_error()
    assert b"phase" in msg and b"0, 1 or 2" in msg, msg


def test_the_deferred_and_held_entry_points_are_not_exported(lib):
    for name in ("ba3c_launch_held", "ba3c_flush_pending", "ba3c_clip_grads_range2"):
        assert not hasattr(lib, name), name


def test_an_empty_batch_samples_nothing(lib, handle, base):
    assert _sample(lib, handle, base, batch=0) == 0
