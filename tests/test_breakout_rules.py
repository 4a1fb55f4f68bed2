"""GridBreakout's rules on the CPU (ba3c_amd.breakout, ba3c_amd.envs.BreakoutPlayer): hand
examples with expected values worked out from the written rules, agreement of the two
statements of the rules (vectorised numpy rows vs. scalar Python player), the player wrappers,
the launcher flags and the C ABI's argument checks.  No kernel is launched here."""
import numpy as np
import pytest

from breakout_policy import NAMES, make_row, player_from_row, scripted_actions


def _step(row, action, limit=40000):
    """One step of `row` through BOTH statements of the rules, which must agree; returns
    (fields dict of the new row, reward, over, ep_score, events)."""
    from ba3c_amd import breakout as K
    game = np.asarray(row, np.int32).reshape(1, 16).copy()
    reward, over, ep = K.step_numpy(game, np.array([action]), limit)
    p = player_from_row(row, limit=limit)
    r2, o2 = p.action(action)
    assert p.game_row() == game[0].tolist()
    assert (r2, o2) == (reward[0], bool(over[0]))
    if o2:
        assert p.last_ep_score == ep[0]
    return dict(zip(NAMES, game[0].tolist())), reward[0], bool(over[0]), int(ep[0]), p.last_events


def _ball(bx, by, vx, vy, **kw):
    return make_row(bx=bx, by=by, vx=vx, vy=vy, in_play=1, **kw)


# ---- render ----------------------------------------------------------------------------
def test_initial_frame_pixels():
    from ba3c_amd import breakout as K
    f = K.render_numpy(K.initial_game(1, 0))[0]
    assert f.shape == (84, 84) and f.dtype == np.uint8
    assert [int(f[18 + 3 * r, 6 * r]) for r in range(6)] == [230, 200, 170, 140, 110, 80]
    assert [int(f[20 + 3 * r, 83]) for r in range(6)] == [230, 200, 170, 140, 110, 80]
    assert f[17].max() == 0 and f[36].max() == 0                    # the band is y in [18, 36)
    assert f[78, 36] == 255 and f[79, 47] == 255 and f[78, 35] == 0 and f[79, 48] == 0
    assert f[77].max() == 0 and f[80].max() == 0
    assert f[2, 0] == 128 and f[3, 1] == 128 and f[2, 2] == 0 and f[3, 17] == 128
    assert f[2, 20] == 0 and f[1].max() == 0 and f[4].max() == 0    # 5 lives: x < 18 only
    assert f[50, 50] == 0
    assert f[0].max() == 0                                          # no ball before the serve
    assert (player_from_row(K.initial_game(1, 0)[0]).current_state() == f).all()


def test_ball_is_drawn_over_bricks_only_in_play():
    from ba3c_amd import breakout as K
    g = _ball(10, 19, 1, 2, lives=2).reshape(1, 16)
    f = K.render_numpy(g)[0]
    assert f[19, 10] == 255 and f[20, 11] == 255 and f[19, 12] == 230 and f[21, 10] == 200
    assert f[2, 4] == 128 and f[2, 8] == 0                          # 2 lives
    g[0, NAMES.index("in_play")] = 0
    assert K.render_numpy(g)[0][19, 10] == 230


# ---- step: hand examples ---------------------------------------------------------------
def test_fire_serves_from_the_lcg():
    g, r, over, _, _ = _step(make_row(rng=12345), 1)
    assert (g["rng"], g["bx"], g["by"], g["vx"], g["vy"], g["in_play"]) == (87628868, 53, 40, -1, 2, 1)
    g, _, _, _, _ = _step(make_row(rng=7), 1)
    assert (g["rng"], g["bx"], g["vx"]) == (1025555898, 16, 1)
    g, _, _, _, _ = _step(make_row(rng=-5), 1)                      # uint32 bits in the int32 slot
    assert (g["rng"], g["bx"], g["vx"]) == (1005581598, 51, 1)
    assert r == 0 and not over and g["t"] == 1


@pytest.mark.parametrize("a", [0, 2, 3, 17, -1])
def test_only_fire_serves(a):
    g, _, _, _, _ = _step(make_row(rng=12345), a)
    assert (g["rng"], g["in_play"], g["bx"]) == (12345, 0, 0)


def test_paddle_moves_and_clamps():
    assert _step(make_row(px=36), 2)[0]["px"] == 39
    assert _step(make_row(px=36), 3)[0]["px"] == 33
    assert _step(make_row(px=71), 2)[0]["px"] == 72
    assert _step(make_row(px=72), 2)[0]["px"] == 72
    assert _step(make_row(px=2), 3)[0]["px"] == 0
    assert _step(make_row(px=0), 3)[0]["px"] == 0
    for a in (0, 1, 4, 17, -1, 1 << 40):
        assert _step(make_row(px=36), a)[0]["px"] == 36


@pytest.mark.parametrize("bx,vx,want_bx,want_vx", [(0, -1, 1, 1), (0, -2, 2, 2), (82, 1, 81, -1),
                                                   (82, 2, 80, -2), (1, -1, 0, -1), (81, 1, 82, 1)])
def test_side_walls_reflect(bx, vx, want_bx, want_vx):
    g, _, _, _, ev = _step(_ball(bx, 50, vx, 2), 0)
    assert (g["bx"], g["vx"], g["by"], g["vy"]) == (want_bx, want_vx, 52, 2)
    assert ("wall" in ev) == (want_vx != vx)


def test_ceiling_reflects():
    g, _, _, _, ev = _step(_ball(40, 1, 1, -2), 0)
    assert (g["by"], g["vy"], g["bx"]) == (1, 2, 41) and "ceiling" in ev
    g, _, _, _, ev = _step(_ball(40, 2, 1, -2), 0)
    assert (g["by"], g["vy"]) == (0, -2) and "ceiling" not in ev


def test_first_corner_wins_when_two_bricks_are_touched():
    # rising to (5, 35): the corners (5,35) and (6,35) lie in bricks (5,0) and (5,1)
    g, r, _, _, ev = _step(_ball(4, 37, 1, -2), 0)
    assert r == 1 and g["b5"] == 0x3FFF & ~1 and ev == {"brick1"}
    assert (g["bx"], g["by"], g["vy"]) == (5, 37, 2)                 # keeps its row, turns round
    # with brick (5,0) gone, the second corner takes (5,1)
    g, r, _, _, _ = _step(_ball(4, 37, 1, -2, b5=0x3FFF & ~1), 0)
    assert r == 1 and g["b5"] == 0x3FFF & ~3
    # falling to (5, 17): only the lower corners touch the band, row 0, worth 7
    g, r, _, _, ev = _step(_ball(4, 15, 1, 2), 0)
    assert r == 7 and g["b0"] == 0x3FFF & ~1 and (g["by"], g["vy"]) == (15, -2) and ev == {"brick7"}
    # upper corners in row 1 (dead), lower corners in row 2: the lower-left one scores 4
    g, r, _, _, _ = _step(_ball(10, 25, 1, -2, b1=0), 0)            # -> (11, 23): rows 1 and 2
    assert r == 4 and g["b2"] == 0x3FFF & ~(1 << 1) and g["b1"] == 0
    # upper-left dead, upper-right alive: the upper-right wins over the lower corners
    g, r, _, _, _ = _step(_ball(10, 22, 1, -2, b0=0x3FFF & ~(1 << 1)), 0)   # -> (11, 20)
    assert r == 7 and g["b0"] == 0x3FFF & ~(3 << 1) and g["b1"] == 0x3FFF
    # nothing alive under any corner: the ball flies through
    g, r, _, _, _ = _step(_ball(12, 30, 1, -2, b3=0, b4=0), 0)      # -> (13, 28): rows 3 and 3
    assert r == 0 and (g["bx"], g["by"], g["vy"]) == (13, 28, -2)


@pytest.mark.parametrize("nx,want_vx", [(35, -2), (37, -2), (38, -1), (40, -1), (41, 1), (43, 1),
                                        (44, 2), (47, 2)])
def test_paddle_bands(nx, want_vx):
    # px = 36, d = nx + 1 - 42
    g, r, _, _, ev = _step(_ball(nx - 1, 75, 1, 2), 0)
    assert (g["bx"], g["by"], g["vx"], g["vy"]) == (nx, 76, want_vx, -2) and ev == {"paddle"} and r == 0


@pytest.mark.parametrize("nx", [34, 48])
def test_paddle_edges_miss(nx):
    g, _, _, _, ev = _step(_ball(nx - 1, 75, 1, 2), 0)
    assert (g["by"], g["vy"], g["in_play"]) == (77, 2, 1) and ev == set()


def test_paddle_uses_its_position_after_the_move():
    g, _, _, _, ev = _step(_ball(48, 75, 0, 2), 2)                  # px 36 -> 39 reaches x = 48
    assert g["px"] == 39 and g["vy"] == -2 and "paddle" in ev


def test_a_miss_costs_a_life():
    g, r, over, _, ev = _step(_ball(5, 81, 1, 2), 0)
    assert (g["in_play"], g["lives"], g["by"]) == (0, 4, 83) and not over and r == 0 and ev == {"lost"}
    g, _, _, _, ev = _step(_ball(5, 80, 1, 2), 0)                   # by = 82 is still in play
    assert (g["in_play"], g["lives"], g["by"]) == (1, 5, 82) and ev == set()


def test_the_fifth_miss_ends_the_episode_and_resets():
    g, r, over, ep, ev = _step(_ball(5, 82, 1, 2, lives=1, score=23, t=99, rng=77, px=12, b2=5), 0)
    assert over and ep == 23 and ev == {"lost", "over_lives"}
    assert g == dict(px=36, bx=0, by=0, vx=0, vy=0, in_play=0, lives=5, score=0, t=0, rng=77,
                     b0=0x3FFF, b1=0x3FFF, b2=0x3FFF, b3=0x3FFF, b4=0x3FFF, b5=0x3FFF)


def test_the_step_limit_ends_the_episode():
    g, _, over, ep, ev = _step(make_row(t=8, score=3), 0, limit=10)
    assert not over and g["t"] == 9 and g["score"] == 3
    g, _, over, ep, ev = _step(make_row(t=9, score=3), 0, limit=10)
    assert over and ep == 3 and g["t"] == 0 and g["score"] == 0 and ev == {"over_limit"}


def test_clearing_the_last_brick_ends_the_episode_with_its_value():
    last = dict(b0=0, b1=0, b2=0, b3=0, b4=0, b5=1 << 3)
    g, r, over, ep, ev = _step(_ball(19, 37, 1, -2, score=100, **last), 0)   # -> (20, 35): brick (5,3)
    assert r == 1 and over and ep == 101 and ev == {"brick1", "over_clear"}
    assert g["b5"] == 0x3FFF and g["score"] == 0 and g["lives"] == 5


# ---- the two statements agree --------------------------------------------------------------
def test_numpy_rows_equal_the_scalar_player_bit_for_bit():
    from ba3c_amd import breakout as K
    from ba3c_amd.envs import BreakoutPlayer
    E, steps, limit, seed = 8, 2000, 400, 3
    rs = np.random.RandomState(seed)
    game = K.initial_game(E, seed)
    players = [BreakoutPlayer(e, 4, seed, limit=limit) for e in range(E)]
    seen, scores = set(), [[] for _ in range(E)]
    for s in range(steps):
        assert [p.game_row() for p in players] == game.tolist()
        frames = K.render_numpy(game)
        for e, p in enumerate(players):
            assert (p.current_state() == frames[e]).all()
        a = scripted_actions(game, rs)
        reward, over, ep = K.step_numpy(game, a, limit)
        for e, p in enumerate(players):
            r, o = p.action(int(a[e]))
            assert (r, o) == (reward[e], bool(over[e])) and isinstance(r, float)
            seen |= p.last_events
            if o:
                scores[e].append(int(ep[e]))
    assert [p.stats["score"] for p in players] == scores and all(len(s) >= 4 for s in scores)
    assert {"wall", "brick1", "paddle", "lost", "over_lives", "over_limit"} <= seen


# ---- wrappers, workers, flags, C ABI ------------------------------------------------------
def test_get_player_breakout_states():
    from ba3c_amd.envs import BreakoutPlayer, get_player
    pl = get_player(idx=2, num_actions=4, seed=5, train=False, game="breakout", limit=50)
    s = pl.current_state()
    assert s.shape == (84, 84, 4) and s.dtype == np.uint8
    assert s[..., :3].max() == 0 and s[78, 36, 3] == 255
    total, overs = 0.0, 0
    for i in range(120):
        r, over = pl.action(1 if i % 9 == 0 else 2 + i % 2)
        total += r
        overs += over
        assert pl.current_state().shape == (84, 84, 4)
    assert overs == 2 and len(pl.stats["score"]) == 2             # LimitLengthPlayer(50)
    base = pl
    while not isinstance(base, BreakoutPlayer):
        base = base.player
    assert base.limit is None
    assert get_player(game="synthetic").current_state().shape == (84, 84, 4)
    with pytest.raises(ValueError):
        get_player(game="pong")


def test_simulator_worker_builds_the_breakout_player():
    from ba3c_amd import simulator as S
    from ba3c_amd.envs import BreakoutPlayer
    w = S.SyntheticSimulatorWorker(3, "ipc:///nowhere/c2s", "ipc:///nowhere/s2c", seed=10,
                                   game="breakout")
    pl = w._build_player()
    base = pl
    while not isinstance(base, BreakoutPlayer) and hasattr(base, "player"):
        base = base.player
    assert isinstance(base, BreakoutPlayer) and base.rng == 13 * 1000 + 3
    assert pl.current_state().shape == (84, 84, 4)
    r, over = pl.action(1)
    assert r == 0.0 and over is False and base.in_play == 1


def test_launcher_flags():
    from ba3c_amd.flags import build_parser, resolve
    a = resolve(build_parser().parse_args("-e GridBreakout-v0 --nr_eval 4".split()))
    assert a.environment == "GridBreakout-v0" and a.channels == 1 and a.nr_eval == 4
    with pytest.raises(SystemExit):
        resolve(build_parser().parse_args("-e GridBreakout-v0 --channels 3".split()))
    with pytest.raises(SystemExit):
        resolve(build_parser().parse_args("-e GridBreakout-v0 --num_actions 3".split()))
    with pytest.raises(SystemExit):
        resolve(build_parser().parse_args("--nr_eval 4".split()))
    d = resolve(build_parser().parse_args([]))
    assert d.environment == "Breakout-v0" and d.nr_eval == 0


def test_capi_argument_checks_without_gpu():
    import ctypes

    from ba3c_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ba3c_breakout_step(None, None, p, 1, 10, p, p, p, None, None) == 1
    assert b"game" in lib.ba3c_last_error()
    assert lib.ba3c_breakout_step(None, p, None, 1, 10, p, p, p, None, None) == 1
    assert lib.ba3c_breakout_step(None, p, p, 0, 10, p, p, p, None, None) == 1
    assert lib.ba3c_breakout_step(None, p, p, 1, 0, p, p, p, None, None) == 1
    assert b"limit" in lib.ba3c_last_error()
    assert lib.ba3c_breakout_step(None, p, p, 1, 10, None, p, p, None, None) == 1
    assert lib.ba3c_breakout_render(None, None, 1, None, None) == 1
    assert lib.ba3c_breakout_render(None, p, 0, None, None) == 1
    assert lib.ba3c_version() == 1
