"""GridBoxing's rules on the CPU (ba3c_amd.boxing, ba3c_amd.envs.BoxingPlayer): hand examples
with expected rows worked out from the written rules, agreement of the two statements of the
rules (vectorised numpy rows vs. scalar Python player), the player wrappers, the launcher flags
and the C ABI's argument checks.  No kernel is launched here."""
import numpy as np
import pytest

from boxing_policy import PUNCH, QUIET, chase_actions, lcg as LCG, make_row, player_from_row, rng_where as _rng

FIRE, UP, RIGHT, LEFT, DOWN = 1, 2, 3, 4, 5


def _wander(odx, ody):
    return _rng(lambda r: not r & 3 and (r >> 2) % 3 - 1 == odx and (r >> 4) % 3 - 1 == ody
                and (r >> 8) & 1)


def _i32(v):
    return v - (1 << 32) if v >= 1 << 31 else v


def _step(action, limit=40000, rng=QUIET, **fields):
    """One step of the crafted row through BOTH statements of the rules, which must agree;
    returns (the new row's first nine fields, reward, over, ep_score, events)."""
    from ba3c_amd import boxing as K
    row = make_row(rng=rng, **fields)
    game = row.reshape(1, 16).copy()
    reward, over, ep = K.step_numpy(game, np.array([action]), limit)
    p = player_from_row(row, limit=limit)
    r2, o2 = p.action(action)
    assert p.game_row() == game[0].tolist()
    assert (r2, o2) == (reward[0], bool(over[0]))
    if o2:
        assert p.last_ep_score == ep[0]
    else:
        assert ep[0] == 0
    assert game[0, 9] == _i32(LCG(rng)) and not game[0, 10:].any()      # one draw per step
    return tuple(game[0, :9].tolist()), reward[0], bool(over[0]), int(ep[0]), p.last_events


FRESH = (20, 42, 58, 42, 0, 0, 0, 0, 0)


# ---- step: hand examples ---------------------------------------------------------------
def test_the_action_table():
    """(dx, dy, fire) of ALE's 18 names: on a quiet step from the centre the agent moves by
    2*(dx, dy) and the cooldown starts iff fire."""
    want = [(0, 0, 0), (0, 0, 1), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (1, -1, 0),
            (-1, -1, 0), (1, 1, 0), (-1, 1, 0), (0, -1, 1), (1, 0, 1), (-1, 0, 1), (0, 1, 1),
            (1, -1, 1), (-1, -1, 1), (1, 1, 1), (-1, 1, 1)]
    from ba3c_amd import boxing as K
    for a, (dx, dy, fire) in enumerate(want):
        g, r, over, _, ev = _step(a, ax=40, ay=42, ox=40, oy=20)         # rows far apart: no points
        assert (g[0], g[1], g[4]) == (40 + 2 * dx, 42 + 2 * dy, 8 * fire), a
        assert r == 0 and not over and ev == ({"miss"} if fire else set())
        assert K.action_id(dx, dy, fire) == a
    for a in (18, -1, 1 << 40, (1 << 32) + 1, -(1 << 63), (1 << 63) - 1):
        assert _step(a, ax=40, ay=42, ox=40, oy=20)[0][:5] == _step(0, ax=40, ay=42, ox=40, oy=20)[0][:5]


def test_one_point_hit_knocks_the_opponent_back():
    # gap 10: the opponent holds (8 <= gap <= 11); 9 < 10 <= 14 scores 1; ox >= ax: pushed right
    g, r, over, _, ev = _step(FIRE, ax=40, ox=50)
    assert g == (40, 42, 53, 42, 8, 0, 1, 0, 1) and r == 1 and not over and ev == {"hit1"}
    # the opponent moves before the punch: gap 15 is out of reach, but it closes in to 14
    g, r, _, _, ev = _step(FIRE, ax=40, ox=55)
    assert g == (40, 42, 57, 42, 8, 0, 1, 0, 1) and r == 1 and ev == {"hit1"}


def test_two_point_hit_knocks_the_opponent_back():
    g, r, _, _, ev = _step(FIRE, ax=40, ox=49)                            # gap 9 scores 2
    assert g == (40, 42, 52, 42, 8, 0, 2, 0, 1) and r == 2 and ev == {"hit2"}
    g, r, _, _, ev = _step(FIRE, ax=50, ox=41)                            # from the right: pushed left
    assert g == (50, 42, 38, 42, 8, 0, 2, 0, 1) and r == 2 and ev == {"hit2"}
    g, r, _, _, ev = _step(FIRE, ax=40, ox=49, ay=42, oy=46)              # |dy| = 4 still reaches
    assert g[6] == 2 and g[3] == 45                                       # (and the opponent closes in)
    g, r, _, _, ev = _step(FIRE, ax=40, ox=49, ay=42, oy=48)              # |dy| = 5 after its move: no
    assert g[6] == 0 and g[3] == 47 and ev == {"miss"}


def test_a_miss_still_costs_the_cooldown():
    g, r, over, _, ev = _step(FIRE)                                       # gap 38: the opponent nears
    assert g == (20, 42, 57, 42, 8, 0, 0, 0, 1) and r == 0 and not over and ev == {"miss"}
    g, r, _, _, ev = _step(FIRE, ax=40, ox=49, a_cd=3)                    # still cooling: no punch
    assert g == (40, 42, 49, 42, 2, 0, 0, 0, 1) and r == 0 and ev == set()
    g, r, _, _, ev = _step(FIRE, ax=40, ox=49, a_cd=1)                    # 1 -> 0 in this step: punch
    assert g[4] == 8 and r == 2


def test_knock_backs_clamp_at_the_ropes():
    assert _step(FIRE, ax=63, ox=73)[0] == (63, 42, 74, 42, 8, 0, 1, 0, 1)          # 76 -> 74
    assert _step(FIRE, ax=15, ox=5)[0] == (15, 42, 4, 42, 8, 0, 1, 0, 1)            # 2 -> 4
    g, r, _, _, ev = _step(0, rng=PUNCH, ax=5, ox=15)                                # agent: 2 -> 4
    assert g == (4, 42, 15, 42, 0, 8, 0, 1, 1) and r == -1 and ev == {"got1"}
    g, r, _, _, ev = _step(0, rng=PUNCH, ax=73, ox=63)                               # agent: 76 -> 74
    assert g == (74, 42, 63, 42, 0, 8, 0, 1, 1) and r == -1 and ev == {"got1"}


def test_the_opponent_punches_on_its_coin_only():
    g, r, _, _, ev = _step(0, rng=PUNCH, ax=40, ox=49)
    assert g == (37, 42, 49, 42, 0, 8, 0, 2, 1) and r == -2 and ev == {"got2"}
    assert _step(0, rng=QUIET, ax=40, ox=49)[0] == (40, 42, 49, 42, 0, 0, 0, 0, 1)
    assert _step(0, rng=PUNCH, ax=40, ox=49, o_cd=2)[0] == (40, 42, 49, 42, 0, 1, 0, 0, 1)
    g, r, _, _, ev = _step(0, rng=PUNCH, ax=49, ox=49)               # level: the agent goes left
    assert g[0] == 46 and g[2] == 50                                 # (s == 0: the opponent steps right)


def test_both_punch_in_one_step_and_the_counter_sees_the_knock_back():
    # the agent's 2-point hit pushes ox 49 -> 52; at gap 12 the counter-punch is worth 1
    g, r, over, _, ev = _step(FIRE, rng=PUNCH, ax=40, ox=49)
    assert g == (37, 42, 52, 42, 8, 8, 2, 1, 1) and r == 1 and ev == {"hit2", "got1"}
    # a hit that knocks the opponent out of reach is not answered: it closes in 54 -> 53, is
    # hit for 1 at gap 13 and lands at 56, gap 16 > 14
    g, r, _, _, ev = _step(FIRE, rng=PUNCH, ax=40, ox=54)
    assert g == (40, 42, 56, 42, 8, 0, 1, 0, 1) and r == 1 and ev == {"hit1"}


def test_the_opponent_backs_off_inside_8_and_steps_right_when_level():
    g = _step(0, ax=30, ay=60, ox=30, oy=20)[0]                      # s == 0, gap 0 < 8
    assert g == (30, 60, 31, 21, 0, 0, 0, 0, 1)
    assert _step(0, ax=30, ay=60, ox=35, oy=20)[0][2:4] == (36, 21)  # gap 5: away from the agent
    assert _step(0, ax=30, ay=60, ox=23, oy=20)[0][2:4] == (22, 21)  # gap 7, other side
    assert _step(0, ax=30, ay=60, ox=38, oy=20)[0][2:4] == (38, 21)  # gap 8: holds
    assert _step(0, ax=30, ay=60, ox=41, oy=20)[0][2:4] == (41, 21)  # gap 11: holds
    assert _step(0, ax=30, ay=60, ox=42, oy=70)[0][2:4] == (41, 69)  # gap 12: closes in, and up
    # the gap is taken after the agent's own move
    assert _step(LEFT, ax=30, ay=60, ox=41, oy=20)[0][:3] == (28, 60, 40)


def test_the_opponent_wanders_one_step_in_four():
    for odx in (-1, 0, 1):
        for ody in (-1, 0, 1):
            g = _step(0, rng=_wander(odx, ody), ay=70, oy=20)[0]
            assert g == (20, 70, 58 + odx, 20 + ody, 0, 0, 0, 0, 1)
    assert _step(0, rng=_wander(1, 1), ay=20, ox=74, oy=70)[0][2:4] == (74, 70)
    assert _step(0, rng=_wander(-1, -1), ay=60, ox=4, oy=14)[0][2:4] == (4, 14)


def test_the_agent_stops_at_all_four_ropes():
    far = dict(ox=40, oy=42)
    assert _step(RIGHT, ax=73, ay=20, **far)[0][:2] == (74, 20)
    assert _step(RIGHT, ax=74, ay=20, **far)[0][:2] == (74, 20)
    assert _step(LEFT, ax=5, ay=20, **far)[0][:2] == (4, 20)
    assert _step(LEFT, ax=4, ay=20, **far)[0][:2] == (4, 20)
    assert _step(UP, ax=20, ay=15, ox=40, oy=60)[0][:2] == (20, 14)
    assert _step(UP, ax=20, ay=14, ox=40, oy=60)[0][:2] == (20, 14)
    assert _step(DOWN, ax=20, ay=69, ox=40, oy=20)[0][:2] == (20, 70)
    assert _step(DOWN, ax=20, ay=70, ox=40, oy=20)[0][:2] == (20, 70)
    assert _step(6, ax=74, ay=14, ox=40, oy=60)[0][:2] == (74, 14)           # UPRIGHT in the corner
    assert _step(9, ax=4, ay=70, ox=40, oy=20)[0][:2] == (4, 70)             # DOWNLEFT in the corner


def test_a_knock_out_win_ends_the_episode_and_resets():
    g, r, over, ep, ev = _step(FIRE, ax=40, ox=49, a_score=99, o_score=37, t=500)
    assert over and r == 2 and ep == 101 - 37 and ev == {"hit2", "ko_win"} and g == FRESH
    g, r, over, ep, ev = _step(FIRE, ax=40, ox=50, a_score=98, o_score=37, t=500)   # 99: not yet
    assert not over and g[6] == 99 and ep == 0


def test_a_knock_out_loss_ends_the_episode():
    g, r, over, ep, ev = _step(0, rng=PUNCH, ax=40, ox=49, a_score=10, o_score=99, t=500)
    assert over and r == -2 and ep == 10 - 101 and ev == {"got2", "ko_loss"} and g == FRESH


def test_the_clock_ends_the_episode():
    g, r, over, ep, ev = _step(0, a_score=5, o_score=3, t=1679)
    assert over and ep == 2 and ev == {"over_clock"} and g == FRESH
    g, r, over, ep, ev = _step(0, a_score=5, o_score=3, t=1678)
    assert not over and g[8] == 1679 and g[6:8] == (5, 3)


def test_the_step_limit_below_the_clock_ends_the_episode():
    g, _, over, ep, ev = _step(0, limit=10, t=8, a_score=3, o_score=7)
    assert not over and g[8] == 9
    g, _, over, ep, ev = _step(0, limit=10, t=9, a_score=3, o_score=7)
    assert over and ep == -4 and ev == {"over_limit"} and g == FRESH


def test_initial_rows_and_generators():
    from ba3c_amd import boxing as K
    g = K.initial_game(3, seed=7)
    assert g.shape == (3, 16) and g.dtype == np.int32
    assert g[:, :10].tolist() == [list(FRESH) + [7000 + e] for e in range(3)] and not g[:, 10:].any()


# ---- render ----------------------------------------------------------------------------
def _frame(**fields):
    from ba3c_amd import boxing as K
    row = make_row(**fields)
    f = K.render_numpy(row.reshape(1, 16))[0]
    assert f.shape == (84, 84) and f.dtype == np.uint8
    assert (player_from_row(row).current_state() == f).all()
    return f


def test_initial_frame_pixels():
    f = _frame()
    assert f[42, 20] == 255 and f[49, 25] == 255 and f[50, 20] == 0 and f[42, 26] == 0 and f[41, 20] == 0
    assert f[42, 19] == 0 and (f[42:50, 20:26] == 255).all()
    assert (f[42:50, 58:64] == 130).all() and f[42, 57] == 0 and f[42, 64] == 0 and f[50, 58] == 0
    assert f[45, 26] == 0 and f[45, 57] == 0                               # no arms
    assert f[:8].max() == 0 and (f[8] == 60).all() and f[9:12].max() == 0  # empty bars, full clock
    assert (f[12, 2:82] == 60).all() and f[12, 1] == 0 and f[12, 82] == 0 and (f[79, 2:82] == 60).all()
    assert (f[12:80, 2] == 60).all() and (f[12:80, 81] == 60).all() and f[11, 2] == 0 and f[80, 81] == 0
    assert f[13, 3] == 0 and f[78, 80] == 0 and f[80:].max() == 0
    assert sorted(set(f.ravel().tolist())) == [0, 60, 130, 255]


def test_the_arm_shows_while_cd_is_at_least_6_on_the_facing_side():
    for cd, shown in ((8, True), (7, True), (6, True), (5, False), (0, False)):
        f = _frame(a_cd=cd)
        assert (f[45:47, 26:30] == (255 if shown else 0)).all(), cd
        assert f[44, 26] == 0 and f[47, 26] == 0 and f[45, 30] == 0 and f[45, 19] == 0
        f = _frame(o_cd=cd)
        assert (f[45:47, 54:58] == (130 if shown else 0)).all(), cd
        assert f[44, 57] == 0 and f[47, 57] == 0 and f[45, 53] == 0 and f[45, 64] == 0
    f = _frame(ax=60, ox=30, a_cd=8, o_cd=8)                               # sides swapped
    assert (f[45:47, 56:60] == 255).all() and f[45, 66] == 0 and f[45, 55] == 0
    assert (f[45:47, 36:40] == 130).all() and f[45, 29] == 0 and f[45, 40] == 0
    f = _frame(ax=40, ay=20, ox=40, oy=60, a_cd=8, o_cd=8)                 # level: right / left
    assert (f[23:25, 46:50] == 255).all() and f[23, 39] == 0
    assert (f[63:65, 36:40] == 130).all() and f[63, 46] == 0


def test_bar_lengths():
    f = _frame(a_score=37, o_score=51, t=400)
    assert (f[2:4, :18] == 255).all() and f[2:4, 18:].max() == 0 and f[1].max() == 0 and f[4].max() == 0
    assert (f[5:7, 59:] == 130).all() and f[5:7, :59].max() == 0 and f[7].max() == 0
    assert (f[8, :64] == 60).all() and f[8, 64:].max() == 0
    f = _frame(a_score=99, o_score=1, t=1679)
    assert (f[2, :49] == 255).all() and f[2, 49] == 0 and f[5].max() == 0
    assert f[8, 0] == 60 and f[8, 1:].max() == 0
    f = _frame(t=19)
    assert (f[8] == 60).all()
    assert _frame(t=20)[8, 83] == 0


def test_priority_where_things_overlap():
    f = _frame(ax=40, ay=42, ox=43, oy=44)
    assert f[44, 43] == 255 and f[44, 45] == 255 and f[44, 46] == 130 and f[50, 43] == 130
    f = _frame(ax=40, ay=42, ox=46, oy=42, a_cd=8)                         # agent arm over its body
    assert (f[45:47, 46:50] == 255).all() and f[45, 50] == 130 and f[44, 46] == 130
    f = _frame(ax=46, ay=42, ox=50, oy=42, o_cd=8)                         # agent body over its arm
    assert (f[45, 46:52] == 255).all() and f[45, 52] == 130
    f = _frame(ax=5, ay=42, ox=4, oy=20, a_cd=8)                           # arm over the ring
    assert (f[45:47, 1:5] == 255).all() and f[44, 2] == 60 and f[47, 2] == 60


# ---- the two statements agree --------------------------------------------------------------
def test_numpy_rows_equal_the_scalar_player_bit_for_bit():
    from ba3c_amd import boxing as K
    from ba3c_amd.envs import BoxingPlayer
    E, steps, limit, seed = 37, 1500, 400, 3
    rs = np.random.RandomState(seed)
    game = K.initial_game(E, seed)
    players = [BoxingPlayer(e, 18, seed, limit=limit) for e in range(E)]
    seen, scores, rewards = set(), [[] for _ in range(E)], set()
    for s in range(steps):
        assert [p.game_row() for p in players] == game.tolist()
        if s % 50 == 0:
            frames = K.render_numpy(game)
            for e, p in enumerate(players):
                assert (p.current_state() == frames[e]).all()
        a = rs.randint(18, size=E).astype(np.int64)
        reward, over, ep = K.step_numpy(game, a, limit)
        for e, p in enumerate(players):
            r, o = p.action(int(a[e]))
            assert (r, o) == (reward[e], bool(over[e])) and isinstance(r, float)
            seen |= p.last_events
            rewards.add(r)
            if o:
                scores[e].append(int(ep[e]))
    assert [p.stats["score"] for p in players] == scores and all(len(s) == 3 for s in scores)
    assert {"hit1", "hit2", "miss", "got1", "got2", "over_limit"} <= seen
    assert rewards >= {-2.0, -1.0, 0.0, 1.0, 2.0}


def test_noop_loses_random_draws_and_the_script_wins():
    """The rules make a game: 8 first episodes at seed 3 per policy.  NOOP is knocked out, the
    chase-align-punch script wins every episode, uniform-random lies between."""
    from ba3c_amd import boxing as K

    def play(policy):
        game, rs = K.initial_game(8, 3), np.random.RandomState(3)
        score = [None] * 8
        while None in score:
            _, over, ep = K.step_numpy(game, policy(game, rs))
            for e in np.nonzero(over)[0]:
                score[e] = int(ep[e]) if score[e] is None else score[e]
        return score
    noop = play(lambda g, rs: np.zeros(8, np.int64))
    rand = play(lambda g, rs: rs.randint(18, size=8))
    script = play(lambda g, rs: chase_actions(g))
    assert max(noop) <= -100
    assert min(script) > 0 and np.mean(script) > np.mean(rand) > np.mean(noop) + 50


# ---- wrappers, workers, flags, C ABI ------------------------------------------------------
def test_get_player_boxing_states():
    from ba3c_amd.envs import BoxingPlayer, get_player
    pl = get_player(idx=2, num_actions=18, seed=5, train=False, game="boxing", limit=50)
    s = pl.current_state()
    assert s.shape == (84, 84, 4) and s.dtype == np.uint8
    assert s[..., :3].max() == 0 and s[42, 20, 3] == 255 and s[42, 58, 3] == 130
    overs = 0
    for i in range(120):
        r, over = pl.action(i % 18)
        overs += over
        s = pl.current_state()
        assert s.shape == (84, 84, 4) and s.dtype == np.uint8
    assert overs == 2 and len(pl.stats["score"]) == 2             # LimitLengthPlayer(50)
    base = pl
    while not isinstance(base, BoxingPlayer):
        base = base.player
    assert base.limit is None and base.get_action_space().num_actions() == 18
    with pytest.raises(ValueError):
        get_player(game="pong")
    with pytest.raises(ValueError):
        get_player(game="GridBoxing-v0")


def test_simulator_worker_builds_the_boxing_player():
    from ba3c_amd import simulator as S
    from ba3c_amd.envs import BoxingPlayer
    w = S.SyntheticSimulatorWorker(3, "ipc:///nowhere/c2s", "ipc:///nowhere/s2c", num_actions=18,
                                   seed=10, game="boxing")
    pl = w._build_player()
    base = pl
    while not isinstance(base, BoxingPlayer) and hasattr(base, "player"):
        base = base.player
    assert isinstance(base, BoxingPlayer) and base.rng == 13 * 1000 + 3
    assert pl.current_state().shape == (84, 84, 4)
    r, over = pl.action(11)
    assert r == 0.0 and over is False and (base.ax, base.a_cd) == (22, 8)


def test_launcher_flags():
    from ba3c_amd import flags as F
    from ba3c_amd.boxing import BoxingVec
    from ba3c_amd.breakout import BreakoutVec
    parse = lambda s: F.resolve(F.build_parser().parse_args(s.split()))
    assert F.GRID_BOXING == "GridBoxing-v0"
    a = parse("-e GridBoxing-v0 --num_actions 18 --nr_eval 4")
    assert a.environment == "GridBoxing-v0" and a.channels == 1 and a.nr_eval == 4
    assert parse("-e GridBoxing-v0 --num_actions 20").num_actions == 20
    for bad in ("-e GridBoxing-v0", "-e GridBoxing-v0 --num_actions 17",
                "-e GridBoxing-v0 --num_actions 18 --channels 3", "--nr_eval 4",
                "-e Boxing-v0 --num_actions 18 --nr_eval 4"):
        with pytest.raises(SystemExit):
            parse(bad)
    assert parse("-e GridBreakout-v0 --nr_eval 4").nr_eval == 4
    assert F.GAMES == {"GridBreakout-v0": (BreakoutVec, 4, "breakout"),
                       "GridBoxing-v0": (BoxingVec, 18, "boxing")}
    assert BoxingVec.A == 18


def test_capi_argument_checks_without_gpu():
    import ctypes

    from ba3c_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    assert lib.ba3c_boxing_step(None, None, p, 1, 10, p, p, p, None, None) == 1
    assert b"game" in lib.ba3c_last_error()
    assert lib.ba3c_boxing_step(None, p, None, 1, 10, p, p, p, None, None) == 1
    assert lib.ba3c_boxing_step(None, p, p, 0, 10, p, p, p, None, None) == 1
    assert lib.ba3c_boxing_step(None, p, p, 1, 0, p, p, p, None, None) == 1
    assert b"limit" in lib.ba3c_last_error()
    assert lib.ba3c_boxing_step(None, p, p, 1, 10, None, p, p, None, None) == 1
    assert lib.ba3c_boxing_step(None, odd, p, 1, 10, p, p, p, None, None) == 1
    assert b"aligned" in lib.ba3c_last_error()
    assert lib.ba3c_boxing_render(None, None, 1, None, None) == 1
    assert lib.ba3c_boxing_render(None, p, 0, None, None) == 1
    assert lib.ba3c_boxing_render(None, odd, 1, None, None) == 1
    assert lib.ba3c_boxing_render(None, p, 1, None, None) == 0         # nothing to write: no launch
    assert lib.ba3c_version() == 1
