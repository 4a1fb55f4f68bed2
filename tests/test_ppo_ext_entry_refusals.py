"""Every refusal of ba3c_train_grads_ppo_ext and ba3c_ppo_norm_adv.  A refusal returns before any
GPU call, so none of this needs a GPU: return code 1 (BA3C_ERR_INVALID), the keyword of the failed
check in ba3c_last_error(), and for a call with two faults the earlier check's message."""
import ctypes

import pytest

from test_ppo_entry_refusals import GRADS_FAULTS, _args, base, handle, lib  # noqa: F401 (fixtures)

# the arguments after the handle / stream, in the order of include/ba3c.h
GRADS = ("params", "state", "action", "rows", "batch", "beta", "clip", "vclip", "flags", "ws", "grads",
         "scalars", "ratio", "phase")
NORM = ("rows", "n", "stats")

# ba3c_train_grads_ppo's own table (the same checks in the same order), with the two new checks
# where they run: after clip_eps, before the phase
_at = [n for n, _, _ in GRADS_FAULTS].index("phase -1")
EXT_FAULTS = GRADS_FAULTS[:_at] + [
    ("vclip -0.1", {"vclip": -0.1}, b"vclip_eps"),
    ("vclip nan", {"vclip": float("nan")}, b"vclip_eps"),
    ("vclip inf", {"vclip": float("inf")}, b"vclip_eps"),
    ("vclip -inf", {"vclip": float("-inf")}, b"vclip_eps"),
    ("flags 2", {"flags": 2}, b"flags"),
    ("flags 3", {"flags": 3}, b"flags"),
    ("flags top bit", {"flags": 0x80000000}, b"flags"),
] + GRADS_FAULTS[_at:]
EXT_ORDER = [({"rows": None}, b"rows"), ({"ratio": "+4"}, b"ratio"), ({"clip": 1.5}, b"clip_eps"),
             ({"vclip": -1.0}, b"vclip_eps"), ({"flags": 4}, b"flags"), ({"phase": 7}, b"phase"),
             ({"params": None}, b"pointer"), ({"batch": 0}, b"batch")]

NORM_FAULTS = [
    ("null rows", {"rows": None}, b"rows"),
    ("rows + 4", {"rows": "+4"}, b"rows"),
    ("rows + 8", {"rows": "+8"}, b"rows"),
    ("stats + 4", {"stats": "+4"}, b"stats"),
    ("stats + 2", {"stats": "+2"}, b"stats"),
    ("n 0", {"n": 0}, b"count"),
    ("n -1", {"n": -1}, b"count"),
]
NORM_ORDER = [({"rows": "+4"}, b"rows"), ({"stats": "+4"}, b"stats"), ({"n": 0}, b"count")]


def _ext(lib, handle, base, **faults):
    p = ctypes.c_void_p(base[1])
    d = dict(params=p, state=p, action=p, rows=p, batch=4, beta=0.01, clip=0.2, vclip=0.2, flags=1,
             ws=p, grads=p, scalars=None, ratio=p, phase=0)
    return lib.ba3c_train_grads_ppo_ext(handle, None, *_args(base, GRADS, d, faults))


def _norm(lib, handle, base, **faults):
    p = ctypes.c_void_p(base[1])
    a = _args(base, NORM, dict(rows=p, n=4, stats=p), faults)
    return lib.ba3c_ppo_norm_adv(None, *a)


CALLS = {"ba3c_train_grads_ppo_ext": (_ext, EXT_FAULTS, EXT_ORDER),
         "ba3c_ppo_norm_adv": (_norm, NORM_FAULTS, NORM_ORDER)}


def test_the_tables_cover_the_plain_entry_and_the_new_checks():
    assert len(EXT_FAULTS) == len(GRADS_FAULTS) + 7 and all(f in EXT_FAULTS for f in GRADS_FAULTS)
    words = [w for _, _, w in EXT_FAULTS]
    assert words.index(b"vclip_eps") > words.index(b"clip_eps")
    assert words.index(b"flags") > words.index(b"vclip_eps") and words.index(b"phase") > words.index(b"flags")


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


def test_a_null_handle_a_null_ratio_and_the_off_values(lib, base):
    assert _ext(lib, None, base) == 1 and b"pointer" in lib.ba3c_last_error()
    # ratio is optional, vclip_eps 0 and flags 0 are the plain loss: each gets as far as the phase
    for kw in (dict(ratio=None), dict(vclip=0.0), dict(flags=0), dict(vclip=0.0, flags=0)):
        assert _ext(lib, None, base, phase=9, **kw) == 1 and b"phase" in lib.ba3c_last_error()
