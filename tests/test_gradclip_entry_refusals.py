"""Every refusal of ba3c_clip_grads_global, in the order the checks run, and the scratch size
ba3c_global_clip_scratch reports.  A refusal returns before any launch and the size is host
arithmetic, so none of this needs a GPU."""
import ctypes

import pytest

import flat_updates as U

ARGS = ("grads", "max_norm", "scratch", "doubles")

# (name, the arguments that commit the fault, the keyword of its message), in the order of the
# checks; "+N": the aligned buffer plus N bytes; doubles N: the needed count plus N, "=N": N itself
FAULTS = [
    ("null grads", {"grads": None}, b"grads"),
    ("grads + 4", {"grads": "+4"}, b"grads"),
    ("grads + 8", {"grads": "+8"}, b"grads"),
    ("max_norm 0", {"max_norm": 0.0}, b"max_norm"),
    ("max_norm -0.5", {"max_norm": -0.5}, b"max_norm"),
    ("max_norm nan", {"max_norm": float("nan")}, b"max_norm"),
    ("max_norm inf", {"max_norm": float("inf")}, b"max_norm"),
    ("max_norm -inf", {"max_norm": float("-inf")}, b"max_norm"),
    ("null scratch", {"scratch": None}, b"8-byte"),
    ("scratch + 4", {"scratch": "+4"}, b"8-byte"),
    ("scratch + 2", {"scratch": "+2"}, b"8-byte"),
    ("one double short", {"doubles": -1}, b"scratch_doubles"),
    ("no doubles", {"doubles": "=0"}, b"scratch_doubles"),
    ("negative doubles", {"doubles": "=-5"}, b"scratch_doubles"),
]
ORDER = [({"grads": "+4"}, b"grads"), ({"max_norm": float("nan")}, b"max_norm"),
         ({"scratch": "+4"}, b"8-byte"), ({"doubles": -1}, b"scratch_doubles")]


@pytest.fixture(scope="module")
def lib():
    from ba3c_amd import _lib as L
    return L.load()


def make_handle(lib, geom, max_batch=1):
    from ba3c_amd import _lib as L
    g = U.GEOMETRIES[geom]
    c = L.Ba3cConfig(max_batch=max_batch, channels=g["C"], fc_neurons=g["F"], fc_splits=g["S"],
                     num_actions=g["A"], replace_with_conv=0 if g["legacy"] else 1, ps=g["ps"])
    h = ctypes.c_void_p()
    assert lib.ba3c_create(ctypes.byref(c), ctypes.byref(h)) == 0, lib.ba3c_last_error()
    return h


@pytest.fixture(scope="module")
def handle(lib):
    h = make_handle(lib, "odd")
    yield h
    lib.ba3c_destroy(h)


@pytest.fixture(scope="module")
def base():
    buf = (ctypes.c_int32 * 64)()
    addr = ctypes.addressof(buf)
    addr += -addr % 16
    assert addr + 32 <= ctypes.addressof(buf) + ctypes.sizeof(buf)
    return buf, addr                                 # buf is returned to keep it alive


def call(lib, handle, base, **faults):
    need = int(lib.ba3c_global_clip_scratch(handle))
    p = ctypes.c_void_p(base[1])
    args = dict(grads=p, max_norm=0.5, scratch=p, doubles=need)
    for k, v in faults.items():
        assert k in args, k
        if k == "doubles":
            args[k] = int(v[1:]) if isinstance(v, str) else need + v
        else:
            args[k] = ctypes.c_void_p(base[1] + int(v)) if isinstance(v, str) else v
    return lib.ba3c_clip_grads_global(handle, None, *[args[k] for k in ARGS])


def test_every_refusal(lib, handle, base):
    for name, f, word in FAULTS:
        assert call(lib, handle, base, **f) == 1, name
        assert word in lib.ba3c_last_error(), (name, lib.ba3c_last_error())


def test_the_earlier_check_is_reported(lib, handle, base):
    for i, (first, word) in enumerate(ORDER):
        for later, later_word in ORDER[i + 1:]:
            assert call(lib, handle, base, **dict(first, **later)) == 1
            msg = lib.ba3c_last_error()
            assert word in msg and later_word not in msg, (first, later, msg)


def test_a_null_handle_is_the_first_refusal(lib, base):
    p = ctypes.c_void_p(base[1])
    # every later argument is at fault too: the handle's message is the one reported
    assert lib.ba3c_clip_grads_global(None, None, None, float("nan"), None, 0) == 1
    msg = lib.ba3c_last_error()
    assert b"handle" in msg and b"grads" not in msg and b"max_norm" not in msg, msg
    assert lib.ba3c_clip_grads_global(None, None, p, 0.5, p, 1 << 20) == 1
    assert b"handle" in lib.ba3c_last_error()
    assert lib.ba3c_global_clip_scratch(None) == 0


def test_the_short_scratch_message_names_both_counts(lib, handle, base):
    need = int(lib.ba3c_global_clip_scratch(handle))
    assert call(lib, handle, base, doubles=-1) == 1
    msg = lib.ba3c_last_error().decode()
    assert str(need - 1) in msg and str(need) in msg, msg


@pytest.mark.parametrize("geom", sorted(U.GEOMETRIES))
def test_the_scratch_is_one_double_per_chunk_and_two(lib, geom):
    h = make_handle(lib, geom)
    try:
        want = U.chunk_count([n for _, n in U.tensors(geom)]) + 2
        assert lib.ba3c_global_clip_scratch(h) == want
    finally:
        lib.ba3c_destroy(h)
