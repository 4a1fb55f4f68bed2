"""Two-player GridBoxing's rules on the CPU (ba3c_amd.duel): hand examples with expected rows
worked out from the written rules, agreement of step_numpy with a scalar restatement, the
mirror invariant over all 324 action pairs, episode ends, scripted play, the two observations,
the --self_play flag and the C ABI's argument checks.  No kernel is launched here."""
import numpy as np
import pytest

from duel_policy import FRESH, ODD_ACTIONS, chase_side_a, chase_side_b, random_rows, row, step_scalar

FIRE, UP, RIGHT, LEFT, DOWN = 1, 2, 3, 4, 5


def _step(a, b, limit=40000, **fields):
    """One step of the crafted row under (a, b) through duel.step_numpy and the scalar rules,
    which must agree.  -> (the new row's first nine fields, reward_A, over, ep_score_A)."""
    from ba3c_amd import duel as D
    r = row(**fields)
    game = r.reshape(1, 16).copy()
    reward, over, ep = D.step_numpy(game, np.array([a, b]), limit)
    want_row, want_r, want_over, want_ep = step_scalar(r.tolist(), a, b, limit)
    assert game[0].tolist() == want_row and game.dtype == np.int32
    assert reward.dtype == np.float64 and over.dtype == bool and ep.dtype == np.int32
    assert reward.tolist() == [want_r, -want_r] and over.tolist() == [want_over] * 2
    assert ep.tolist() == [want_ep, -want_ep]
    assert game[0, 9] == r[9] and not game[0, 10:].any()            # rng carried, padding zero
    return tuple(game[0, :9].tolist()), reward[0], bool(over[0]), int(ep[0])


# ---- step: hand examples ---------------------------------------------------------------
def test_a_simultaneous_punch_at_near_range_scores_both_and_knocks_them_apart():
    g, r, over, ep = _step(FIRE, FIRE, ax=40, bx=49)                 # gap 9 scores 2 for both
    assert g == (37, 42, 52, 42, 8, 8, 2, 2, 1) and r == 0 and not over and ep == 0
    g, r, _, _ = _step(FIRE, FIRE, ax=40, bx=50)                     # gap 10 scores 1
    assert g == (37, 42, 53, 42, 8, 8, 1, 1, 1) and r == 0
    g, r, _, _ = _step(FIRE, FIRE, ax=50, bx=41)                     # B on the left: apart again
    assert g == (53, 42, 38, 42, 8, 8, 2, 2, 1) and r == 0


def test_a_punch_on_cooldown_lands_nothing():
    g, r, _, _ = _step(FIRE, 0, ax=40, bx=49, a_cd=3)
    assert g == (40, 42, 49, 42, 2, 0, 0, 0, 1) and r == 0
    g, r, _, _ = _step(FIRE, 0, ax=40, bx=49, a_cd=1)                # 1 -> 0 in this step: punch
    assert g == (40, 42, 52, 42, 8, 0, 2, 0, 1) and r == 2
    g, r, _, _ = _step(0, FIRE, ax=40, bx=49, b_cd=2)
    assert g == (40, 42, 49, 42, 0, 1, 0, 0, 1) and r == 0
    g, r, _, _ = _step(FIRE, FIRE, ax=40, bx=49, b_cd=2)             # only A lands
    assert g == (40, 42, 52, 42, 8, 1, 2, 0, 1) and r == 2
    g, r, _, _ = _step(FIRE, 0)                                      # a miss still costs the cooldown
    assert g == (20, 42, 58, 42, 8, 0, 0, 0, 1) and r == 0


def test_side_b_moves_in_its_mirrored_frame():
    assert _step(0, RIGHT)[0] == (20, 42, 56, 42, 0, 0, 0, 0, 1)     # B's RIGHT: the world's bx - 2
    assert _step(0, LEFT)[0] == (20, 42, 60, 42, 0, 0, 0, 0, 1)
    assert _step(0, UP)[0] == (20, 42, 58, 40, 0, 0, 0, 0, 1)               # its dy is unchanged
    assert _step(0, DOWN)[0] == (20, 42, 58, 44, 0, 0, 0, 0, 1)
    assert _step(RIGHT, RIGHT)[0] == (22, 42, 56, 42, 0, 0, 0, 0, 1)     # both move 2 px
    assert _step(6, 6)[0] == (22, 40, 56, 40, 0, 0, 0, 0, 1)             # UPRIGHT, UPRIGHT
    assert _step(0, 16, bx=58)[0] == (20, 42, 56, 44, 0, 8, 0, 0, 1)     # DOWNRIGHTFIRE: a miss
    # the ropes, in B's frame: its LEFT at the world's right rope, its RIGHT at the left one
    assert _step(0, LEFT, bx=73, by=20)[0][2] == 74 and _step(0, LEFT, bx=74, by=20)[0][2] == 74
    assert _step(0, RIGHT, bx=5, by=20)[0][2] == 4 and _step(0, RIGHT, bx=4, by=20)[0][2] == 4
    assert _step(0, UP, by=15)[0][3] == 14 and _step(0, DOWN, by=69)[0][3] == 70
    # the judgement is made after BOTH moves: gap 16 closes to 12 before the punch
    g, r, _, _ = _step(11, RIGHT, ax=30, bx=46)                      # RIGHTFIRE vs RIGHT
    assert g == (32, 42, 47, 42, 8, 0, 1, 0, 1) and r == 1


def test_knock_backs_clamp_at_the_ropes():
    assert _step(FIRE, 0, ax=63, bx=73)[0] == (63, 42, 74, 42, 8, 0, 1, 0, 1)        # 76 -> 74
    assert _step(FIRE, 0, ax=15, bx=5)[0] == (15, 42, 4, 42, 8, 0, 1, 0, 1)          # 2 -> 4
    g, r, _, _ = _step(0, FIRE, ax=5, bx=15)                                          # A: 2 -> 4
    assert g == (4, 42, 15, 42, 0, 8, 0, 1, 1) and r == -1
    g, r, _, _ = _step(0, FIRE, ax=73, bx=63)                                         # A: 76 -> 74
    assert g == (74, 42, 63, 42, 0, 8, 0, 1, 1) and r == -1
    assert _step(FIRE, FIRE, ax=5, bx=13)[0] == (4, 42, 16, 42, 8, 8, 2, 2, 1)        # only A's clamps


def test_level_boxers_are_knocked_apart_with_b_to_the_right():
    g, r, _, _ = _step(FIRE, FIRE, ax=40, bx=40, by=44)              # ax == bx: b_right holds
    assert g == (37, 42, 43, 44, 8, 8, 2, 2, 1) and r == 0
    assert _step(FIRE, 0, ax=40, bx=40, by=44)[0] == (40, 42, 43, 44, 8, 0, 2, 0, 1)
    assert _step(0, FIRE, ax=40, bx=40, by=44)[0] == (37, 42, 40, 44, 0, 8, 0, 2, 1)
    assert _step(FIRE, 0, ax=40, bx=40, by=47)[0] == (40, 42, 40, 47, 8, 0, 0, 0, 1)  # |dy| = 5: no


def test_actions_outside_the_18_are_noop_on_either_side():
    for odd in ODD_ACTIONS + (-(1 << 63), (1 << 63) - 1):
        assert _step(odd, FIRE, ax=40, bx=49) == _step(0, FIRE, ax=40, bx=49)
        assert _step(11, odd, ax=40, bx=49) == _step(11, 0, ax=40, bx=49)
        assert _step(odd, odd, ax=40, bx=49)[0] == (40, 42, 49, 42, 0, 0, 0, 0, 1)


def test_numpy_rows_equal_the_scalar_rules():
    from ba3c_amd import duel as D
    rs = np.random.RandomState(0)
    rows = random_rows(rs, 4000)
    act = rs.randint(-1, 19, size=8000).astype(np.int64)
    for limit in (1000, 40000):
        game = rows.copy()
        reward, over, ep = D.step_numpy(game, act, limit)
        for e in range(4000):
            want = step_scalar(rows[e].tolist(), int(act[e]), int(act[4000 + e]), limit)
            assert game[e].tolist() == want[0]
            assert (reward[e], over[e], ep[e]) == want[1:]
            assert (reward[4000 + e], over[4000 + e], ep[4000 + e]) == (-want[1], want[2], -want[3])
        assert over.any() and not over.all() and (reward > 0).any() and (reward < 0).any()


# ---- the mirror invariant ------------------------------------------------------------------
def test_mirror_rows_is_an_involution_that_fixes_the_fresh_row():
    from ba3c_amd import duel as D
    rows = random_rows(np.random.RandomState(1), 400)
    m = D.mirror_rows(rows)
    assert m.dtype == np.int32 and m.shape == rows.shape and not (m == rows).all()
    assert (D.mirror_rows(m)[:, :10] == rows[:, :10]).all() and not m[:, 10:].any()
    assert (m[:, 0] == 78 - rows[:, 2]).all() and (m[:, 3] == rows[:, 1]).all()
    assert (m[:, 4] == rows[:, 5]).all() and (m[:, 7] == rows[:, 6]).all()
    assert (m[:, 8:10] == rows[:, 8:10]).all()
    fresh = row(rng=77)
    assert (D.mirror_rows(fresh) == fresh).all() and D.mirror_rows(fresh).shape == (16,)


def test_the_rules_are_symmetric_under_the_mirror_for_all_324_action_pairs():
    """step(mirror(g), b, a) == mirror(step(g, a, b)), rewards and ep_scores negated."""
    from ba3c_amd import duel as D
    N = 400
    rows = random_rows(np.random.RandomState(2), N)
    rows[:, 10:] = 0
    a = np.repeat(np.arange(18), 18)
    b = np.tile(np.arange(18), 18)
    game = np.repeat(rows, 324, axis=0)                               # row-major: row x pair
    act = np.concatenate([np.tile(a, N), np.tile(b, N)])
    swapped = np.concatenate([np.tile(b, N), np.tile(a, N)])
    n = game.shape[0]
    for limit in (1000, 40000):
        g1, g2 = game.copy(), D.mirror_rows(game)
        r1, o1, e1 = D.step_numpy(g1, act, limit)
        r2, o2, e2 = D.step_numpy(g2, swapped, limit)
        assert (g2 == D.mirror_rows(g1)).all()
        assert (r2[:n] == -r1[:n]).all() and (r2[:n] == r1[n:]).all() and (r2[n:] == r1[:n]).all()
        assert (o2 == o1).all() and (o1[:n] == o1[n:]).all()
        assert (e2[:n] == -e1[:n]).all() and (e1[n:] == -e1[:n]).all() and (e2[n:] == e1[:n]).all()
        # what the rows covered: hits of 1 and 2 by either side, both at once, clamped knock-backs,
        # level boxers, and every way an episode ends
        both = (r1[:n] == 0) & (g1[:, 4] == 8) & (g1[:, 5] == 8) & (g1[:, 6] > game[:, 6])
        assert set(np.unique(r1).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0} and both.any()
        assert (game[:, 0] == game[:, 2]).any() and o1.any() and not o1.all()
        assert ((g1[:, 2] == 74) & (r1[:n] > 0)).any() and ((g1[:, 0] == 4) & (r1[:n] < 0)).any()
        assert ((e1[:n] == 0) & o1[:n] & (game[:, 6] >= 98)).any()     # a drawn knock-out


# ---- episode ends --------------------------------------------------------------------------
def test_knock_outs_by_either_side_and_by_both_at_once():
    g, r, over, ep = _step(FIRE, 0, ax=40, bx=49, a_score=99, b_score=37, t=500, rng=12345)
    assert over and r == 2 and ep == 101 - 37 and g == FRESH
    g, r, over, ep = _step(FIRE, 0, ax=40, bx=50, a_score=98, b_score=37, t=500)   # 99: not yet
    assert not over and g[6] == 99 and ep == 0
    g, r, over, ep = _step(0, FIRE, ax=40, bx=49, a_score=10, b_score=98, t=500)
    assert over and r == -2 and ep == 10 - 100 and g == FRESH
    g, r, over, ep = _step(FIRE, FIRE, ax=40, bx=49, a_score=98, b_score=98, t=500)
    assert over and r == 0 and ep == 0 and g == FRESH                              # a draw
    g, r, over, ep = _step(FIRE, FIRE, ax=40, bx=50, a_score=99, b_score=98, t=500)
    assert over and r == 0 and ep == 1 and g == FRESH                              # 100 : 99


def test_the_clock_and_the_step_limit_end_the_episode():
    g, r, over, ep = _step(0, 0, a_score=5, b_score=3, t=1679, rng=-7)
    assert over and ep == 2 and g == FRESH
    g, r, over, ep = _step(0, 0, a_score=5, b_score=3, t=1678)
    assert not over and ep == 0 and g[8] == 1679 and g[6:8] == (5, 3)
    g, _, over, ep = _step(0, 0, limit=10, t=8, a_score=3, b_score=7)
    assert not over and g[8] == 9 and ep == 0
    g, _, over, ep = _step(0, 0, limit=10, t=9, a_score=3, b_score=7)
    assert over and ep == -4 and g == FRESH


def test_step_numpy_keeps_the_player_order_over_several_games():
    from ba3c_amd import duel as D
    game = np.stack([row(ax=40, bx=49, rng=5), row(), row(ax=40, bx=49, a_score=99, rng=-3)])
    reward, over, ep = D.step_numpy(game, np.array([FIRE, RIGHT, FIRE, 0, RIGHT, 0]), 40000)
    assert game[:, :9].tolist() == [[40, 42, 52, 42, 8, 0, 2, 0, 1], [22, 42, 56, 42, 0, 0, 0, 0, 1],
                                    list(FRESH)]
    assert game[:, 9].tolist() == [5, 0, -3]
    assert reward.tolist() == [2, 0, 2, -2, 0, -2] and over.tolist() == [False, False, True] * 2
    assert ep.tolist() == [0, 0, 101, 0, 0, -101]
    assert D.initial_game(3, seed=7)[:, :10].tolist() == [list(FRESH) + [7000 + e] for e in range(3)]


# ---- play ----------------------------------------------------------------------------------
def _play(policy_a, policy_b, G=8, seed=3):
    """The first episode of G games: -> (ep_score_A [G], the step each ended at [G])."""
    from ba3c_amd import duel as D
    game, rs = D.initial_game(G, seed), np.random.RandomState(seed)
    score, steps = [None] * G, [None] * G
    for s in range(1, 1681):
        act = np.concatenate([policy_a(game, rs), policy_b(game, rs)])
        _, over, ep = D.step_numpy(game, act)
        for e in np.nonzero(over[:G])[0]:
            if score[e] is None:
                score[e], steps[e] = int(ep[e]), s
        if None not in score:
            break
    return score, steps


def test_random_sides_run_to_the_clock_and_the_script_knocks_a_noop_side_out():
    rand = lambda g, rs: rs.randint(18, size=g.shape[0])
    noop = lambda g, rs: np.zeros(g.shape[0], np.int64)
    r_score, r_steps = _play(rand, rand)
    assert r_steps == [1680] * 8 and max(abs(s) for s in r_score) < 50      # no knock-out in sight
    a_score, a_steps = _play(lambda g, rs: chase_side_a(g), noop)
    assert min(a_score) >= 100 and max(a_steps) < 1680                      # 100 or 101 to nothing
    b_score, b_steps = _play(noop, lambda g, rs: chase_side_b(g))
    assert b_score == [-s for s in a_score] and b_steps == a_steps          # the mirror image
    assert min(a_score) > max(r_score) and min(r_score) > max(b_score)


# ---- render --------------------------------------------------------------------------------
def test_each_side_sees_itself_as_the_white_boxer_on_the_left():
    from ba3c_amd import boxing as K
    from ba3c_amd import duel as D
    rows = random_rows(np.random.RandomState(4), 37)
    f = D.render_numpy(rows)
    assert f.shape == (74, 84, 84) and f.dtype == np.uint8
    assert (f[:37] == K.render_numpy(rows)).all()
    assert (f[37:] == K.render_numpy(D.mirror_rows(rows))).all()
    fresh = D.render_numpy(row().reshape(1, 16))
    assert (fresh[0] == fresh[1]).all() and fresh[0, 42, 20] == 255 and fresh[0, 42, 58] == 130
    one = D.render_numpy(row(ax=30, ay=20, bx=50, by=60, a_cd=8, a_score=10, b_score=40).reshape(1, 16))
    assert (one[0, 20:28, 30:36] == 255).all() and (one[0, 60:68, 50:56] == 130).all()
    assert (one[0, 23:25, 36:40] == 255).all()                               # A's arm, to the right
    assert (one[1, 60:68, 28:34] == 255).all() and (one[1, 20:28, 48:54] == 130).all()
    assert (one[1, 23:25, 44:48] == 130).all()                               # A's arm as B sees it
    assert (one[0, 2, :5] == 255).all() and one[0, 2, 5] == 0 and (one[1, 2, :20] == 255).all()
    assert (one[0, 5, 64:] == 130).all() and one[1, 5, 78] == 0 and (one[1, 5, 79:] == 130).all()


# ---- flags, C ABI --------------------------------------------------------------------------
def test_the_self_play_flag():
    from ba3c_amd import flags as F
    parse = lambda s: F.resolve(F.build_parser().parse_args(s.split()))
    a = parse("-e GridBoxing-v0 --num_actions 18 --self_play --simulator_procs 100")
    assert a.self_play is True and a.simulator_procs == 100
    assert parse("-e GridBoxing-v0 --num_actions 18 --self_play --nr_eval 4").nr_eval == 4
    assert parse("-e GridBoxing-v0 --num_actions 18").self_play is False
    assert parse("").self_play is False and F.build_parser().get_default("self_play") is False
    for bad in ("-e GridBreakout-v0 --self_play", "--self_play", "-e Boxing-v0 --num_actions 18 --self_play",
                "-e GridBoxing-v0 --num_actions 18 --self_play --simulator_procs 99",
                "-e GridBoxing-v0 --num_actions 18 --self_play --frame_skip 2",
                "-e GridBoxing-v0 --num_actions 18 --self_play --sticky 0.25",
                "-e GridBoxing-v0 --num_actions 18 --self_play --frame_skip 2-4 --sticky 0.25"):
        with pytest.raises(SystemExit) as e:
            parse(bad)
        assert isinstance(e.value.code, str) and e.value.code                # a message, not a status
    assert set(F.GAMES) == {"GridBreakout-v0", "GridBoxing-v0"}              # not a third game


def test_the_match_tool_refuses_a_run_without_side_b():
    from ba3c_amd import duel as D
    for argv in ("--load a.npz --episodes 3 --games 2", "--load a.npz --load_b b.npz --random_b",
                 "--random_b --episodes 0", "--random_b -e GridBreakout-v0"):
        with pytest.raises(SystemExit) as e:
            D.main(argv.split())
        assert isinstance(e.value.code, str) and e.value.code


def test_duel_vec_takes_no_frame_skip():
    from ba3c_amd import duel as D
    assert D.BoxingDuelVec.A == 18
    with pytest.raises(TypeError):
        D.BoxingDuelVec(2, frame_skip=2)                                      # no frame skip here


def test_capi_argument_checks_without_gpu():
    import ctypes

    from ba3c_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "ba3c_boxing_duel_step") and hasattr(lib, "ba3c_boxing_duel_render")
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    odd1 = ctypes.c_void_p(p.value + 1)
    step, render = lib.ba3c_boxing_duel_step, lib.ba3c_boxing_duel_render
    assert step(None, None, p, 1, 10, p, p, p, None, None) == 1
    assert b"game" in lib.ba3c_last_error()
    assert step(None, p, None, 1, 10, p, p, p, None, None) == 1
    assert step(None, p, p, 0, 10, p, p, p, None, None) == 1
    assert step(None, p, p, -3, 10, p, p, p, None, None) == 1
    assert step(None, p, p, 1, 0, p, p, p, None, None) == 1
    assert b"limit" in lib.ba3c_last_error()
    for out in ((None, p, p), (p, None, p), (p, p, None)):
        assert step(None, p, p, 1, 10, out[0], out[1], out[2], None, None) == 1
        assert b"output" in lib.ba3c_last_error()
    assert step(None, odd, p, 1, 10, p, p, p, None, None) == 1
    assert b"aligned" in lib.ba3c_last_error()
    assert step(None, p, p, 1, 10, p, p, p, odd1, None) == 1                  # frame: 4-byte
    assert step(None, p, p, 1, 10, p, p, p, None, odd) == 1                   # state: 16-byte
    assert b"aligned" in lib.ba3c_last_error()
    assert render(None, None, 1, None, None) == 1
    assert render(None, p, 0, None, None) == 1
    assert render(None, odd, 1, None, None) == 1
    assert render(None, p, 1, odd1, None) == 1
    assert render(None, p, 1, None, odd) == 1
    assert render(None, p, 1, None, None) == 0                                # nothing to write: no launch
