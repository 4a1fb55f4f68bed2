"""Every refusal of the games' step / decision / render entry points, as one table.  A refusal
returns before any launch, so none of this needs a GPU: return code 1 (BA3C_ERR_INVALID), the
keyword of the failed check in ba3c_last_error(), and for a call with two faults the earlier
check's message."""
import ctypes

import pytest

# the arguments after `stream`, in the order of include/ba3c.h
STEP = ("game", "action", "n", "limit", "reward", "over", "ep", "frame", "state")
SKIP = ("game", "aux", "action", "n", "limit", "lo", "hi", "q16", "reward", "over", "ep", "frame", "state")
DECIDE = SKIP[:8] + ("h_lo", "h_hi") + SKIP[8:]
RENDER = ("game", "n", "frame", "state")

# entry point -> (its arguments, the name of its count, the alignment of its aux rows in bytes)
ENTRIES = {
    "ba3c_breakout_step": (STEP, b"n_envs", None),
    "ba3c_boxing_step": (STEP, b"n_envs", None),
    "ba3c_boxing_duel_step": (STEP, b"n_games", None),
    "ba3c_breakout_step_skip": (SKIP, b"n_envs", 8),
    "ba3c_boxing_step_skip": (SKIP, b"n_envs", 8),
    "ba3c_boxing_duel_decide": (DECIDE, b"n_games", 16),
    "ba3c_breakout_render": (RENDER, b"n_envs", None),
    "ba3c_boxing_render": (RENDER, b"n_envs", None),
    "ba3c_boxing_duel_render": (RENDER, b"n_games", None),
}

# One fault per check, in the order the checks run: (name, arguments that commit it, keyword of
# its message).  A fault applies to the entry points that take all of its arguments; "COUNT"
# stands for the entry point's own count name, "+N" for the aligned buffer plus N bytes.
FAULTS = [
    ("null game", {"game": None}, b"game"),
    ("null action", {"action": None}, b"game"),
    ("null aux", {"aux": None}, b"aux"),
    ("null reward", {"reward": None}, b"output"),
    ("null over", {"over": None}, b"output"),
    ("null ep_score", {"ep": None}, b"output"),
    ("count 0", {"n": 0}, "COUNT"),
    ("count -3", {"n": -3}, "COUNT"),
    ("limit 0", {"limit": 0}, b"limit"),
    ("limit -1", {"limit": -1}, b"limit"),
    ("game + 4", {"game": "+4"}, b"aligned"),
    ("game + 8", {"game": "+8"}, b"aligned"),
    ("state + 8", {"state": "+8"}, b"aligned"),
    ("frame + 2", {"frame": "+2"}, b"aligned"),
    ("aux + 4", {"aux": "+4"}, b"aux"),
    ("aux + 8", {"aux": "+8"}, b"aux"),               # the 16-byte aux rows only
    ("skip lo 0", {"lo": 0}, b"skip"),
    ("skip lo -1", {"lo": -1, "hi": 1}, b"skip"),
    ("skip hi < lo", {"lo": 5, "hi": 2}, b"skip"),
    ("skip hi 17", {"lo": 1, "hi": 17}, b"skip"),
    ("sticky -1", {"q16": -1}, b"sticky"),
    ("sticky 65537", {"q16": 65537}, b"sticky"),
    ("sticky 2^20", {"q16": 1 << 20}, b"sticky"),
    ("start lo 3", {"h_lo": 3}, b"start"),
    ("start hi < lo", {"h_lo": 12, "h_hi": 8}, b"start"),
    ("start hi 20", {"h_hi": 20}, b"start"),
]

# The checks in order, one fault of each: (arguments, a word only its message has).  Of two
# faults in one call the earlier in this list is the one reported.
ORDER = [
    ({"game": None}, b"null game"),
    ({"aux": None}, b"null aux"),
    ({"reward": None}, b"output"),
    ({"n": 0}, b">= 1"),
    ({"state": "+8"}, b"game / state"),
    ({"aux": "+4"}, b"aux must be"),
    ({"hi": 17}, b"skip"),
    ({"q16": 65537}, b"sticky"),
    ({"h_lo": 3}, b"start"),
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


def _call(lib, base, fn, **faults):
    names = ENTRIES[fn][0]
    p = ctypes.c_void_p(base[1])
    args = dict(game=p, aux=p, action=p, n=1, limit=10, lo=2, hi=4, q16=16384, h_lo=8, h_hi=14,
                reward=p, over=p, ep=p, frame=None, state=None)
    for k, v in faults.items():
        args[k] = ctypes.c_void_p(base[1] + int(v)) if isinstance(v, str) else v
    return getattr(lib, fn)(None, *[args[k] for k in names])


def _applies(fn, faults):
    names, _, aux_align = ENTRIES[fn]
    if not set(faults) <= set(names):
        return False
    return faults.get("aux") != "+8" or aux_align == 16


@pytest.mark.parametrize("fn", sorted(ENTRIES))
def test_every_refusal(lib, base, fn):
    count = ENTRIES[fn][1]
    seen = 0
    for name, faults, word in FAULTS:
        if not _applies(fn, faults):
            continue
        assert _call(lib, base, fn, **faults) == 1, name
        msg = lib.ba3c_last_error()
        assert (count if word == "COUNT" else word) in msg, (name, msg)
        if "aux" in faults and faults["aux"] is not None:
            assert b"aligned" in msg and b"%d-byte" % ENTRIES[fn][2] in msg, (name, msg)
        seen += 1
    assert seen == {STEP: 13,SKIP: 22, DECIDE: 26, RENDER: 7}[ENTRIES[fn][0]]


@pytest.mark.parametrize("fn", sorted(ENTRIES))
def test_the_earlier_check_is_reported(lib, base, fn):
    order = [(f, w) for f, w in ORDER if _applies(fn, f)]
    assert len(order) >= 3
    for i, (first, word) in enumerate(order):
        for later, later_word in order[i + 1:]:
            if set(first) & set(later):              # two faults of one argument cannot be combined
                continue
            assert _call(lib, base, fn, **dict(first, **later)) == 1
            msg = lib.ba3c_last_error()
            assert word in msg and later_word not in msg, (first, later, msg)


@pytest.mark.parametrize("fn", [f for f in sorted(ENTRIES) if ENTRIES[f][0] is RENDER])
def test_render_of_nothing_is_ok(lib, base, fn):
    assert _call(lib, base, fn) == 0                 # neither frame nor state: no launch
    assert _call(lib, base, fn, game=None) == 1      # but the checks still ran
