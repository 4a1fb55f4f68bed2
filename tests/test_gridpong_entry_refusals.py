"""GridPong's four entry points refuse what the other games' refuse, before any launch: step / decision /
render walk FAULTS and ORDER of tests/test_game_entry_refusals.py, the view env_view's checks in their order."""
import ctypes

import pytest

from test_game_entry_refusals import FAULTS, ORDER, RENDER, SKIP, STEP, base, lib  # noqa: F401 (fixtures)

VIEW = ("game", "n", "sel", "n_sel", "palette", "hud", "scale", "out")
ENTRIES = {"ba3c_gridpong_step": STEP, "ba3c_gridpong_step_skip": SKIP, "ba3c_gridpong_render": RENDER,
           "ba3c_gridpong_view": VIEW}
# the view's checks in order, then more faults of the same checks: (arguments, a word of the message)
VIEW_ORDER = [({"palette": None}, b"null"), ({"n_sel": 0}, b">= 1"), ({"scale": 9}, b"scale"), ({"out": "+2"}, b"aligned")]
VIEW_FAULTS = [(str(f), f, w) for f, w in VIEW_ORDER + [
    ({"game": None}, b"null"), ({"out": None}, b"null"), ({"n": 0}, b">= 1"), ({"scale": 0}, b"scale"),
    ({"game": "+8"}, b"aligned"), ({"sel": "+1"}, b"aligned"), ({"hud": "+2"}, b"aligned")]]


def _call(lib, base, fn, **faults):
    p = ctypes.c_void_p(base[1])
    args = dict(game=p, aux=p, action=p, n=1, limit=10, lo=2, hi=4, q16=16384, reward=p, over=p, ep=p,
                frame=None, state=None, sel=None, n_sel=1, palette=p, hud=None, scale=2, out=p)
    for k, v in faults.items():
        args[k] = ctypes.c_void_p(base[1] + int(v)) if isinstance(v, str) else v
    return getattr(lib, fn)(None, *[args[k] for k in ENTRIES[fn]])


@pytest.mark.parametrize("fn", sorted(ENTRIES))
def test_every_refusal_and_the_first_is_reported(lib, base, fn):
    names = ENTRIES[fn]
    faults, order = (VIEW_FAULTS, VIEW_ORDER) if names is VIEW else (FAULTS, ORDER)
    applies = lambda f: set(f) <= set(names) and f.get("aux") != "+8"      # 8-byte aux rows
    seen = 0
    for name, f, word in faults:
        if applies(f):
            assert _call(lib, base, fn, **f) == 1, name
            assert (b"n_envs" if word == "COUNT" else word) in lib.ba3c_last_error(), name
            seen += 1
    assert seen == {STEP: 13, SKIP: 22, RENDER: 7, VIEW: 11}[names]
    order = [(f, w) for f, w in order if applies(f)]
    for i, (first, word) in enumerate(order):
        for later, later_word in order[i + 1:]:
            if not set(first) & set(later):
                assert _call(lib, base, fn, **dict(first, **later)) == 1
                msg = lib.ba3c_last_error()
                assert word in msg and later_word not in msg, (first, later, msg)
    if names is RENDER:
        assert _call(lib, base, fn) == 0                 # neither frame nor state: no launch
