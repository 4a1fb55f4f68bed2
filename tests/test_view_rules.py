"""The colour view and the episode recorder, on the CPU: `ba3c_amd.view.view_numpy` (the oracle of
the view kernel) against the games' own render_numpy and a hand-worked HUD strip, the palettes,
`hud_from_policy`, the host-side refusals of ba3c_breakout_view / ba3c_boxing_view, and
`ba3c_amd.record.Episode` (replay over the CPU oracle, save / load) built from CPU roll-outs."""
import functools

import numpy as np
import pytest

import boxing_policy
import breakout_policy

GAME_NAMES = ["breakout", "boxing"]


def _game(name):
    from ba3c_amd import boxing, breakout
    from ba3c_amd.flags import GRID_BOXING, GRID_BREAKOUT
    return {"breakout": (breakout, breakout_policy, GRID_BREAKOUT),
            "boxing": (boxing, boxing_policy, GRID_BOXING)}[name]


@functools.lru_cache(maxsize=None)
def reached_rows(name):
    """Every 10th row set of 300 steps of the scripted policy, 5 simulators: [150, 16]."""
    _, P, _ = _game(name)
    return P.trajectory(5, 300, 40000, 3).games[::10].reshape(-1, 16)


def hand_hud():
    """Four HUD rows holding every clamp case, and the strips they must give."""
    from ba3c_amd import view as V
    hud = np.zeros((4, 20), np.uint8)
    hud[0, :4], hud[0, 18], hud[0, 19] = (0, 1, 16, 200), 2, 0          # 200 clamps to 16
    hud[1, :4], hud[1, 18], hud[1, 19] = (0, 1, 16, 200), 255, 84       # no action chosen
    hud[2, 17], hud[2, 18], hud[2, 19] = 5, 17, 255                     # 255 clamps to 84
    hud[3, 0], hud[3, 18], hud[3, 19] = 16, 18, 10                      # 18: no such bar
    want = np.zeros((4, 20, 84, 3), np.uint8)
    want[:, 0] = V.HUD_SEP
    for i, length in enumerate((0, 84, 84, 10)):
        want[i, 1:3, :length] = V.HUD_VALUE
    for i, chosen in ((0, 2), (1, None)):
        want[i, 19, 10:13] = V.HUD_LO                                   # action 1: height 1
        want[i, 4:20, 14:17] = V.HUD_HI if chosen == 2 else V.HUD_LO    # action 2: height 16
        want[i, 4:20, 18:21] = V.HUD_LO                                 # action 3: 200 -> 16
    want[2, 15:20, 74:77] = V.HUD_HI                                    # action 17: x in [74, 77)
    want[3, 4:20, 6:9] = V.HUD_LO                                       # action 0: x in [6, 9)
    return hud, want


@pytest.mark.parametrize("name", GAME_NAMES)
def test_view_at_scale_one_is_the_palette_of_the_render(name):
    from ba3c_amd.view import view_numpy
    K, _, _ = _game(name)
    rows = reached_rows(name)
    got = view_numpy(rows, K.PALETTE)
    assert got.dtype == np.uint8 and got.shape == (rows.shape[0], 84, 84, 3)
    assert (got == K.PALETTE[K.render_numpy(rows)]).all()
    assert (view_numpy(rows, K.PALETTE, scale=1, hud=None, sel=None) == got).all()


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("name", GAME_NAMES)
def test_scaled_blocks_are_constant_and_equal_the_pixel(name, S):
    from ba3c_amd.view import view_numpy
    K, _, _ = _game(name)
    rows = reached_rows(name)[::7]
    hud, _ = hand_hud()
    hud = hud[np.arange(rows.shape[0]) % 4]
    for h in (None, hud):
        one = view_numpy(rows, K.PALETTE, 1, h)
        big = view_numpy(rows, K.PALETTE, S, h)
        hc = 84 + (20 if h is not None else 0)
        assert one.shape[1:] == (hc, 84, 3) and big.shape[1:] == (hc * S, 84 * S, 3)
        blocks = big.reshape(-1, hc, S, 84, S, 3)
        assert (blocks == one[:, :, None, :, None, :]).all()


@pytest.mark.parametrize("name", GAME_NAMES)
def test_hud_strip_equals_the_hand_worked_array(name):
    from ba3c_amd import view as V
    K, _, _ = _game(name)
    hud, want = hand_hud()
    assert V.HUD_H == 20 and len({V.HUD_BG, V.HUD_SEP, V.HUD_VALUE, V.HUD_LO, V.HUD_HI}) == 5
    assert (V.hud_strip_numpy(hud) == want).all()
    rows = reached_rows(name)[40:44]
    got = V.view_numpy(rows, K.PALETTE, 1, hud)
    assert got.shape == (4, 104, 84, 3)
    assert (got[:, :84] == K.PALETTE[K.render_numpy(rows)]).all() and (got[:, 84:] == want).all()
    with pytest.raises(ValueError):
        V.view_numpy(rows, K.PALETTE, 1, hud[:3])
    with pytest.raises(ValueError):
        V.view_numpy(rows, K.PALETTE, 1, hud.astype(np.int32))


@pytest.mark.parametrize("name", GAME_NAMES)
def test_sel_repeats_reverses_and_blanks_what_is_out_of_range(name):
    from ba3c_amd.view import view_numpy
    K, _, _ = _game(name)
    rows = reached_rows(name)[50:55]
    hud, _ = hand_hud()
    sel = np.array([4, 0, 0, 7, -1, 2, 5, 3, 2, 1], np.int32)
    hud = hud[np.arange(sel.size) % 4]
    full = view_numpy(rows, K.PALETTE, 2)
    got = view_numpy(rows, K.PALETTE, 2, sel=sel)
    with_hud = view_numpy(rows, K.PALETTE, 2, hud, sel)
    for i, s in enumerate(sel):
        if 0 <= s < 5:
            assert (got[i] == full[s]).all() and (with_hud[i, :168] == full[s]).all()
            assert (with_hud[i, 168:] == view_numpy(rows[:1], K.PALETTE, 2, hud[i:i + 1])[0, 168:]).all()
        else:
            assert not got[i].any() and not with_hud[i].any()
    assert (view_numpy(rows, K.PALETTE, 2, sel=np.arange(5)[::-1]) == full[::-1]).all()


@pytest.mark.parametrize("scale", [0, 9, -1, 2.0])
def test_scale_outside_one_to_eight_raises(scale):
    from ba3c_amd import breakout as K
    from ba3c_amd.view import view_numpy
    with pytest.raises(ValueError):
        view_numpy(K.initial_game(1), K.PALETTE, scale)
    assert view_numpy(K.initial_game(1), K.PALETTE, 8).shape == (1, 672, 672, 3)


@pytest.mark.parametrize("name,n_shades", [("breakout", 9), ("boxing", 4)])
def test_palette_gives_the_rendered_shades_distinct_colours(name, n_shades):
    K, _, _ = _game(name)
    assert K.PALETTE.dtype == np.uint8 and K.PALETTE.shape == (256, 3)
    shades = np.unique(K.render_numpy(reached_rows(name)))
    assert len(shades) == n_shades and set(shades.tolist()) == set(K.COLOURS)
    colours = {tuple(K.PALETTE[s].tolist()) for s in shades}
    assert len(colours) == len(shades)
    for i in range(256):
        if i not in K.COLOURS:
            assert K.PALETTE[i].tolist() == [i, i, i]


def test_the_two_palettes_differ():
    from ba3c_amd import boxing, breakout
    assert not np.array_equal(boxing.PALETTE, breakout.PALETTE)


def test_hud_from_policy_on_cpu_tensors():
    import torch

    from ba3c_amd.view import hud_from_policy
    g = torch.Generator().manual_seed(0)
    probs = torch.softmax(3 * torch.randn(64, 18, generator=g), dim=1)
    actions = torch.randint(-2, 21, (64,), generator=g)
    value = 4 * torch.randn(64, generator=g)
    value[:3] = torch.tensor([0.0, 50.0, -50.0])
    hud = hud_from_policy(probs, actions, value)
    assert hud.dtype == torch.uint8 and hud.shape == (64, 20)
    h = hud.numpy()
    assert h[:, :18].max() <= 16 and h[:, 19].max() <= 84 and h[:3, 19].tolist() == [42, 84, 0]
    a = actions.numpy()
    assert (h[:, 18] == np.where((a >= 0) & (a < 18), a, 255)).all()
    assert (h[:, :18] == np.round(16 * probs.numpy().astype(np.float64))).all()
    hot = torch.zeros(18, 18)
    hot[torch.arange(18), torch.arange(18)] = 1.0
    assert (hud_from_policy(hot, torch.arange(18), None)[:, :18].numpy() == 16 * np.eye(18)).all()
    four = hud_from_policy(torch.full((2, 4), 0.25), None, None).numpy()       # a 4-action game
    assert four[:, :4].tolist() == [[4] * 4] * 2 and not four[:, 4:18].any()
    assert four[:, 18].tolist() == [255, 255] and four[:, 19].tolist() == [42, 42]


@pytest.mark.parametrize("fn", ["ba3c_breakout_view", "ba3c_boxing_view"])
def test_capi_argument_checks_without_gpu(fn):
    import ctypes

    from ba3c_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, fn)
    f = getattr(lib, fn)
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 16 == 0
    odd2, odd4 = ctypes.c_void_p(p.value + 2), ctypes.c_void_p(p.value + 4)

    def call(game=p, n_envs=1, sel=None, n_sel=1, palette=p, hud=None, scale=1, out=p):
        return f(None, game, n_envs, sel, n_sel, palette, hud, scale, out)
    err = lib.ba3c_last_error
    for null in ("game", "palette", "out"):
        assert call(**{null: None}) == 1 and null.encode() in err()
    assert call(n_envs=0) == 1 and b"n_envs" in err()
    assert call(n_sel=0) == 1 and b"n_sel" in err()
    assert call(n_sel=-3) == 1 and err()
    for scale in (0, 9, -1, 1 << 20):
        assert call(scale=scale) == 1 and b"scale" in err(), scale
    assert call(game=odd4) == 1 and b"aligned" in err()
    for arg in ("sel", "hud", "out"):
        assert call(**{arg: odd2}) == 1 and b"aligned" in err()
    assert lib.ba3c_version() == 1


def cpu_episode(name, skip):
    """One whole episode of a single simulator under the scripted policy, limit 60, rolled out
    with the CPU oracle and written down as an Episode; also the rows it went through."""
    from ba3c_amd import frameskip as F
    from ba3c_amd.record import Episode
    from ba3c_amd.view import view_numpy
    K, P, game_name = _game(name)
    rs = np.random.RandomState(5)
    game, aux = K.initial_game(1, 7), F.initial_aux(1, 7)
    rows, actions, rewards, score = [game[0].copy()], [], [], None
    while score is None:
        a = P.scripted_actions(game, rs)
        if skip is None:
            r, over, ep = K.step_numpy(game, a, 60)
        else:
            r, over, ep = F.step_numpy(K, game, aux, a, 60, *skip)
        actions.append(a[0])
        rewards.append(r[0])
        rows.append(game[0].copy())
        if over[0]:
            score = int(ep[0])
    rows = np.stack(rows)
    T = len(actions)
    probs = rs.random_sample((T, K.NUM_ACTIONS)).astype(np.float32)
    steps = np.arange(0, T, 3)
    ep = Episode(game_name, 60, skip, rows[0], F.initial_aux(1, 7)[0] if skip else None, actions, rewards,
                 probs, rs.normal(size=T), score, view_numpy(rows[steps], K.PALETTE, 2), steps)
    return ep, rows, np.asarray(rewards), score


@pytest.mark.parametrize("skip", [None, (2, 4, 16384)], ids=["plain", "skip-2-4-sticky"])
@pytest.mark.parametrize("name", GAME_NAMES)
def test_episode_replays_and_round_trips(name, skip, tmp_path):
    from ba3c_amd.record import Episode
    ep, rows, rewards, score = cpu_episode(name, skip)
    assert 1 <= ep.steps <= 60 and ep.steps == len(rewards) and ep.score == score
    if skip is not None:
        assert ep.steps < 60 * 2 // 4 + 2                    # at least 2 game steps per decision
    got_rows, got_rewards, got_score = ep.replay()
    assert got_rows.dtype == np.int32 and (got_rows == rows).all()
    assert got_rewards.dtype == np.float64 and (got_rewards == rewards).all() and got_score == score
    files = ep.save(str(tmp_path / "sub" / "ep"))
    assert files[0] == str(tmp_path / "sub" / "ep.npz")
    with np.load(files[0], allow_pickle=False) as f:
        assert {"row0", "actions", "rewards", "probs", "values", "score", "steps", "frames",
                "frame_steps", "game", "limit"} <= set(f.files)
        assert all(f[k].dtype != object for k in f.files)
    back = Episode.load(files[0])
    assert (back.game, back.limit, back.skip, back.score, back.steps) == (
        ep.game, ep.limit, ep.skip, ep.score, ep.steps)
    for k in ("row0", "actions", "rewards", "probs", "values", "frames", "frame_steps"):
        a, b = getattr(ep, k), getattr(back, k)
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), k
    assert (back.aux0 is None) if skip is None else (back.aux0 == ep.aux0).all()
    r2 = back.replay()
    assert (r2[0] == rows).all() and (r2[1] == rewards).all() and r2[2] == score
    try:
        import PIL  # noqa: F401
    except ImportError:
        assert len(files) == 1
    else:
        assert files[1:] == [str(tmp_path / "sub" / "ep.gif")] and (tmp_path / "sub" / "ep.gif").stat().st_size > 0


@pytest.mark.parametrize("argv", [["--random", "--episodes", "1"],
                                  ["--random", "-e", "Breakout-v0"],
                                  ["-e", "GridBreakout-v0"]], ids=["default-env", "synthetic-env", "no-policy"])
def test_record_cli_exits_without_an_on_device_game_or_a_policy(argv, tmp_path):
    from ba3c_amd import record
    with pytest.raises(SystemExit) as e:
        record.main(argv + ["--out", str(tmp_path / "rec")])
    assert isinstance(e.value.code, str) and ("-e " in e.value.code or "--load" in e.value.code)
    assert not (tmp_path / "rec").exists()
