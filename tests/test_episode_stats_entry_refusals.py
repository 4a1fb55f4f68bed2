"""Every refusal of ba3c_episode_stats through the loaded library, with host pointers.  A refusal
returns before any launch, so none of this needs a GPU: return code 1 (BA3C_ERR_INVALID), the
keyword of the failed check in ba3c_last_error(), and for a call with two faults the earlier
check's message."""
import ctypes

import pytest

# the arguments after `stream`, in the order of include/ba3c.h
ARGS = ("reward", "over", "n", "ret", "len", "log_score", "log_len", "log_env", "cap", "head")
POINTERS = tuple(a for a in ARGS if a not in ("n", "cap"))

# One fault per check, in the order the checks run: (name, arguments that commit it, keyword).
# "+N" stands for the aligned buffer plus N bytes.
FAULTS = [("null " + a, {a: None}, b"null pointer") for a in POINTERS] + [
    ("n_envs 0", {"n": 0}, b"n_envs"),
    ("n_envs -7", {"n": -7}, b"n_envs"),
    ("cap below n_envs", {"n": 9, "cap": 8}, b"cap"),
    ("cap 0", {"cap": 0}, b"cap"),
    ("cap -1", {"cap": -1}, b"cap"),
    ("reward + 4", {"reward": "+4"}, b"aligned"),
    ("ret + 4", {"ret": "+4"}, b"aligned"),
    ("ret + 1", {"ret": "+1"}, b"aligned"),
    ("log_score + 4", {"log_score": "+4"}, b"aligned"),
    ("head + 4", {"head": "+4"}, b"aligned"),
    ("len + 2", {"len": "+2"}, b"aligned"),
    ("log_len + 2", {"log_len": "+2"}, b"aligned"),
    ("log_env + 1", {"log_env": "+1"}, b"aligned"),
]

# The checks in order, one fault of each: (arguments, a word only its message has).
ORDER = [
    ({"log_env": None}, b"null pointer"),
    ({"n": 0}, b"n_envs must"),
    ({"cap": 0}, b"cap must"),
    ({"head": "+4"}, b"aligned"),
]


@pytest.fixture(scope="module")
def lib():
    from ba3c_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def base():
    buf = (ctypes.c_int32 * 64)()
    addr = ctypes.addressof(buf)
    addr += -addr % 16
    assert addr + 32 <= ctypes.addressof(buf) + ctypes.sizeof(buf)
    return buf, addr                                 # buf is returned to keep it alive


def _call(lib, base, **faults):
    p = ctypes.c_void_p(base[1])
    args = dict({a: p for a in POINTERS}, n=4, cap=4)
    for k, v in faults.items():
        args[k] = ctypes.c_void_p(base[1] + int(v)) if isinstance(v, str) else v
    return lib.ba3c_episode_stats(None, *[args[k] for k in ARGS])


def test_every_refusal(lib, base):
    for name, faults, word in FAULTS:
        assert _call(lib, base, **faults) == 1, name
        assert word in lib.ba3c_last_error(), (name, lib.ba3c_last_error())
    assert len(FAULTS) == 21


def test_over_needs_no_alignment_and_cap_may_equal_n_envs(lib, base):
    """The checks that must NOT fire, seen through the one that then does."""
    assert _call(lib, base, over="+1", n=4, cap=4, head="+4") == 1
    assert b"aligned" in lib.ba3c_last_error()
    assert _call(lib, base, over="+3", len="+4", log_len="+4", log_env="+12", reward="+8", n=0) == 1
    assert b"n_envs" in lib.ba3c_last_error()


def test_the_earlier_check_is_reported(lib, base):
    for i, (first, word) in enumerate(ORDER):
        for later, later_word in ORDER[i + 1:]:
            assert _call(lib, base, **dict(first, **later)) == 1
            msg = lib.ba3c_last_error()
            assert word in msg and later_word not in msg, (first, later, msg)
