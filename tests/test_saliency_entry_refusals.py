"""Every refusal of ba3c_conv0_input_grad and ba3c_input_grads.  A refusal returns before any
GPU call, so none of this needs a GPU: return code 1 (BA3C_ERR_INVALID), the keyword of the failed
check in ba3c_last_error(), and for a call with two faults the earlier check's message."""
import ctypes

import pytest

# the arguments after the handle / stream, in the order of include/ba3c.h
NAMES = {"ba3c_conv0_input_grad": ("params", "ws", "batch", "dstate", "map"),
         "ba3c_input_grads": ("params", "state", "action", "seeds", "batch", "ws", "grads", "dstate", "map")}
# (the arguments that commit the fault, the keyword of its message); "+N": the aligned buffer + N
FAULTS = {
    "ba3c_conv0_input_grad": [({"params": None}, b"pointer"), ({"ws": "+8"}, b"pointer"),
                              ({"dstate": None}, b"pointer"), ({"dstate": "+4"}, b"pointer"),
                              ({"map": "+8"}, b"pointer"), ({"batch": 0}, b"batch"), ({"batch": 33}, b"batch")],
    "ba3c_input_grads": [({"params": "+4"}, b"pointer"), ({"state": None}, b"pointer"),
                         ({"action": None}, b"pointer"), ({"seeds": None}, b"pointer"),
                         ({"seeds": "+8"}, b"pointer"), ({"ws": None}, b"pointer"), ({"grads": "+4"}, b"pointer"),
                         ({"dstate": None}, b"pointer"), ({"map": "+4"}, b"pointer"), ({"batch": -1}, b"batch"),
                         ({"batch": 33}, b"batch")],
}


@pytest.fixture(scope="module")
def lib():
    from ba3c_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def handles(lib):
    from ba3c_amd import _lib as L
    hs = {}
    for C in (4, 12):
        c = L.Ba3cConfig(max_batch=32, channels=C, fc_neurons=128, fc_splits=4, num_actions=4,
                         replace_with_conv=1, ps=1)
        hs[C] = ctypes.c_void_p()
        assert lib.ba3c_create(ctypes.byref(c), ctypes.byref(hs[C])) == 0, lib.ba3c_last_error()
    yield hs
    for h in hs.values():
        lib.ba3c_destroy(h)


BUF = (ctypes.c_int32 * 64)()
BASE = ctypes.addressof(BUF) + -ctypes.addressof(BUF) % 16


def call(lib, fn, handle, **faults):
    p = ctypes.c_void_p(BASE)
    args = dict({k: p for k in NAMES[fn]}, batch=4)
    for k, v in faults.items():
        assert k in args, k
        args[k] = ctypes.c_void_p(BASE + int(v)) if isinstance(v, str) else v
    return getattr(lib, fn)(handle, None, *[args[k] for k in NAMES[fn]])


@pytest.mark.parametrize("fn", sorted(NAMES))
def test_every_refusal_and_the_earlier_check_first(lib, handles, fn):
    for f, word in FAULTS[fn]:
        assert call(lib, fn, handles[4], **f) == 1, f
        assert word in lib.ba3c_last_error(), (f, lib.ba3c_last_error())
    assert call(lib, fn, None) == 1 and b"pointer" in lib.ba3c_last_error()
    # RGB frames are refused last; a null map alone is no fault
    assert call(lib, fn, handles[12], map=None) == 1
    assert b"saliency needs channels == 4" in lib.ba3c_last_error()
    for f, word in (({"dstate": None, "batch": 0}, b"pointer"), ({"batch": 0}, b"batch")):
        assert call(lib, fn, handles[12], **f) == 1 and word in lib.ba3c_last_error()
