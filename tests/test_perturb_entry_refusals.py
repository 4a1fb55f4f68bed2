"""Every refusal of ba3c_perturb_states and ba3c_perturb_scores.  A refusal returns before any GPU
call, so none of this needs a GPU: return code 1 (BA3C_ERR_INVALID), the keyword of the failed
check in ba3c_last_error(), and for a call with two faults the earlier check's message."""
import ctypes

import pytest

BUF = (ctypes.c_int32 * 64)()
BASE = ctypes.addressof(BUF) + -ctypes.addressof(BUF) % 16
# the arguments after the stream, in the order of include/ba3c.h, with a call that has no fault
GOOD = {"ba3c_perturb_states": dict(state=BASE, n=2, first=100, count=478, newest=0, out=BASE),
        "ba3c_perturb_scores": dict(probs0=BASE, value0=BASE, probs=BASE, value=BASE, n=2, num_actions=4,
                                    which=1, map=BASE, grid=None)}
ST, SC = "ba3c_perturb_states", "ba3c_perturb_scores"
CASES = [                                      # (entry point, the faults, the keyword of the message)
    (ST, dict(state=None), b"null"), (ST, dict(out=None), b"null"), (ST, dict(n=0), b"n must"),
    (ST, dict(first=-1), b"chunk"), (ST, dict(count=0), b"chunk"), (ST, dict(count=479), b"chunk"),
    (ST, dict(first=578, count=1), b"chunk"), (ST, dict(state=BASE + 8), b"aligned"),
    (ST, dict(out=BASE + 4), b"aligned"),
    (SC, dict(probs0=None), b"null"), (SC, dict(value0=None), b"null"), (SC, dict(probs=None), b"null"),
    (SC, dict(value=None), b"null"), (SC, dict(map=None), b"null"), (SC, dict(n=-3), b"n must"),
    (SC, dict(which=2), b"which"), (SC, dict(which=-1), b"which"), (SC, dict(num_actions=0), b"num_actions"),
    (SC, dict(num_actions=32), b"num_actions"),
    # two faults: the earlier check speaks
    (ST, dict(n=0, out=BASE + 4), b"n must"), (ST, dict(count=479, state=BASE + 8), b"chunk"),
    (SC, dict(map=None, which=2), b"null"), (SC, dict(which=2, num_actions=32), b"which"),
]


@pytest.mark.parametrize("fn,faults,word", CASES)
def test_refusal_and_its_order(fn, faults, word):
    from ba3c_amd import _lib as L
    lib = L.load()
    assert set(faults) <= set(GOOD[fn])
    args = [ctypes.c_void_p(v) if k in ("state", "out", "probs0", "value0", "probs", "value", "map", "grid")
            else v for k, v in dict(GOOD[fn], **faults).items()]
    assert getattr(lib, fn)(None, *args) == 1 and word in lib.ba3c_last_error(), lib.ba3c_last_error()
