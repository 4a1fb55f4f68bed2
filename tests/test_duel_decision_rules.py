"""Two-player GridBoxing's decisions on the CPU (ba3c_amd.duel: decide_numpy, drawn starts):
agreement with a scalar restatement of the written rules, the default setting against
step_numpy, episode ends inside a skip, the mirror invariant of a whole decision, the drawn
rows, the draws' frequencies, how much contact a drawn start buys, the flags and the C ABI's
argument checks.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest

from duel_decision import M32, SKIPS, STARTS, decide_scalar, draw_scalar, lcg, signed
from duel_policy import ODD_ACTIONS, random_rows, row

FIRE = 1


def _random_aux(rs, n):
    aux = np.zeros((n, 8), np.int64)
    aux[:, :3] = rs.randint(0, 1 << 32, (n, 3), dtype=np.int64)
    aux[:, 3:5] = rs.randint(0, 18, (n, 2))
    return aux.astype(np.uint32).view(np.int32).reshape(n, 8)


def _random_actions(rs, n):
    act = rs.randint(-1, 19, size=2 * n).astype(np.int64)
    odd = np.array(ODD_ACTIONS + (20, 31, 32), np.int64)         # 20, 31: in [0, 32) yet NOOP
    return np.where(rs.random_sample(2 * n) < 0.15, odd[rs.randint(len(odd), size=2 * n)], act)


# ---- decide_numpy against the scalar rules -------------------------------------------------
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("skip", SKIPS)
def test_numpy_decisions_equal_the_scalar_rules(skip, start):
    from ba3c_amd import duel as D
    n = 600
    rs = np.random.RandomState(0)
    rows, auxs, act = random_rows(rs, n), _random_aux(rs, n), _random_actions(rs, n)
    for limit in (1000, 40000):
        game, aux = rows.copy(), auxs.copy()
        reward, over, ep = D.decide_numpy(game, aux, act, limit, *skip, start=start)
        assert reward.dtype == np.float64 and over.dtype == bool and ep.dtype == np.int32
        assert game.dtype == np.int32 and aux.dtype == np.int32
        short = 0
        for e in range(n):
            want = decide_scalar(rows[e].tolist(), auxs[e].tolist(), int(act[e]), int(act[n + e]), limit,
                                 *skip, start=start)
            assert game[e].tolist() == want[0] and aux[e].tolist() == want[1], e
            assert (reward[e], over[e], ep[e]) == want[2:5], e
            assert (reward[n + e], over[n + e], ep[n + e]) == (-want[2], want[3], -want[4]), e
            short += want[5] < want[6]
        assert over.any() and not over.all() and (reward > 0).any() and (reward < 0).any()
        assert (short > 0) == (skip[1] > 1)                      # ends inside a skip were among them


def test_the_default_setting_is_exactly_one_step_and_draws_nothing():
    from ba3c_amd import duel as D
    n = 2000
    rs = np.random.RandomState(1)
    rows, auxs, act = random_rows(rs, n), _random_aux(rs, n), _random_actions(rs, n)
    for start in (None, (19, 19)):
        for limit in (1000, 40000):
            g1, g2, aux = rows.copy(), rows.copy(), auxs.copy()
            want = D.step_numpy(g1, act, limit)
            got = D.decide_numpy(g2, aux, act, limit, 1, 1, 0, start)
            assert (g1 == g2).all() and all((w == g).all() for w, g in zip(want, got))
            assert (g2[:, 9] == rows[:, 9]).all() and want[1].any()          # rng untouched
            # the aux row still moved: one draw for k, one per side, and prev is the action taken
            assert (aux[:, 0].astype(np.int64) & M32 == [lcg(int(v) & M32) for v in auxs[:, 0]]).all()
            assert (aux[:, 1].astype(np.int64) & M32 == [lcg(int(v) & M32) for v in auxs[:, 1]]).all()
            noop = lambda a: np.where((a >= 0) & (a < 32), a, 0)
            over = want[1][:n]
            assert (aux[:, 3] == np.where(over, 0, noop(act[:n]))).all()
            assert (aux[:, 4] == np.where(over, 0, noop(act[n:]))).all() and not aux[:, 5:].any()


def test_an_episode_that_ends_inside_a_skip_drops_the_rest_and_draws_one_fresh_row():
    from ba3c_amd import duel as D
    r = row(ax=40, bx=49, t=18, a_score=7, b_score=2, rng=12345)
    for start in (None, (4, 7)):
        game = r.reshape(1, 16).copy()
        aux = np.array([[11, 22, 33, 5, 7, 0, 0, 0]], np.int32)
        reward, over, ep = D.decide_numpy(game, aux, np.array([FIRE, 0]), 20, 4, 4, 0, start)
        # t: 18 -> 19 -> 20 = limit: two of the four sub-steps ran; A's punch landed in the first
        assert over.tolist() == [True, True] and reward.tolist() == [2, -2] and ep.tolist() == [7, -7]
        assert aux[0, 3:].tolist() == [0, 0, 0, 0, 0]                            # both prev reset
        assert int(aux[0, 1]) & M32 == lcg(lcg(22)) and int(aux[0, 2]) & M32 == lcg(lcg(33))
        assert int(aux[0, 0]) & M32 == lcg(11)
        if start is None:
            assert game[0, :10].tolist() == [20, 42, 58, 42, 0, 0, 0, 0, 0, 12345]
        else:
            assert game[0, :10].tolist() == draw_scalar(12345, start)            # ONE draw
            assert int(game[0, 9]) & M32 == lcg(12345)
        assert not game[0, 10:].any()
    # one sub-step short of the end: nothing is dropped, nothing is drawn
    game = r.reshape(1, 16).copy()
    aux = np.array([[11, 22, 33, 5, 7, 0, 0, 0]], np.int32)
    _, over, _ = D.decide_numpy(game, aux, np.array([FIRE, 0]), 23, 4, 4, 0, (4, 7))
    assert not over.any() and game[0, 8] == 22 and game[0, 9] == 12345 and aux[0, 3:5].tolist() == [1, 0]


# ---- the mirror invariant ------------------------------------------------------------------
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("skip", SKIPS)
def test_a_whole_decision_is_symmetric_under_the_mirror(skip, start):
    """decide(mirror(g), mirror_aux(x), (b, a)) == mirror(decide(g, x, (a, b))), rewards and
    ep_scores negated -- over several decisions in a row, so drawn rows and reset prevs feed on."""
    from ba3c_amd import duel as D
    n = 1500
    rs = np.random.RandomState(2)
    g1, x1 = random_rows(rs, n), _random_aux(rs, n)
    g1[:, 10:] = 0
    g2, x2 = D.mirror_rows(g1), D.mirror_aux(x1)
    assert (D.mirror_aux(x2) == x1).all() and (x2[:, 0] == x1[:, 0]).all() and not (x2 == x1).all()
    overs = 0
    for d in range(6):
        act = _random_actions(rs, n)
        swapped = np.concatenate([act[n:], act[:n]])
        r1, o1, e1 = D.decide_numpy(g1, x1, act, 1000, *skip, start=start)
        r2, o2, e2 = D.decide_numpy(g2, x2, swapped, 1000, *skip, start=start)
        assert (g2 == D.mirror_rows(g1)).all() and (x2 == D.mirror_aux(x1)).all(), d
        assert (r2[:n] == -r1[:n]).all() and (r2[:n] == r1[n:]).all() and (o2 == o1).all(), d
        assert (e2[:n] == -e1[:n]).all() and (e2[n:] == e1[:n]).all(), d
        overs += int(o1[:n].sum())
    assert overs > 0 and (r1 != 0).any()


def test_every_drawn_row_is_its_own_mirror_image_and_lies_inside_the_clamps():
    from ba3c_amd import duel as D
    rng = np.arange(1 << 16, dtype=np.int64) << 16                # every value of the 16 bits drawn from
    for start in ((4, 7), (4, 19), (7, 7), (4, 4), (18, 19)):
        game = np.zeros((rng.shape[0], 16), np.int32)
        # rows whose NEXT rng has the wanted high bits: draw directly
        _, h, y = D.draw_start(rng, start)
        r = D.frameskip.lcg(rng) >> 16
        assert (h == start[0] + r % (start[1] - start[0] + 1)).all() and (y == 14 + 2 * ((r >> 8) % 29)).all()
        game[:, 0], game[:, 1], game[:, 2], game[:, 3] = 39 - h, y, 39 + h, y
        assert (D.mirror_rows(game) == game).all()
        assert h.min() == start[0] and h.max() == start[1] and y.min() == 14 and y.max() == 70
        assert (game[:, 0] >= 4).all() and (game[:, 2] <= 74).all() and (game[:, 2] - game[:, 0] >= 8).all()
        assert ((game[:, 2] - game[:, 0] <= 14) == (h <= 7)).all()               # reach iff h <= 7
    rows = D.initial_rows(50, 3, (4, 19))
    assert (D.mirror_rows(rows) == rows).all() and len(set(rows[:, 0].tolist())) > 4
    assert (rows[:, 9].astype(np.int64) & M32 == [lcg(3000 + e) for e in range(50)]).all()
    fixed = D.initial_rows(5, 3)
    assert (fixed == D.initial_game(5, 3)).all() and (D.initial_rows(5, 3, (19, 19)) == fixed).all()
    for bad in ((3, 7), (4, 20), (8, 7), (4,), "4-7", (4, 7, 9)):
        with pytest.raises(ValueError):
            D.check_start(bad)
    aux = D.initial_aux(3, 2)
    want = [[signed((2000 + c + e) ^ 0x9E3779B9) for c in (6, 0, 3)] + [0] * 5 for e in range(3)]
    assert aux.tolist() == want and aux.dtype == np.int32


# ---- frequencies ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_drawn_rows_are_spread_over_their_range(seed):
    """h and y over one row's chain of fresh episodes.  h is a 16-bit draw modulo 4 or 16; y is
    the draw's upper 8 bits modulo 29, so y's 24 low values have probability 9/256 and its 5 high
    ones 8/256 (0.906 of uniform): 4000 expected per value keeps those inside the 15 % too."""
    from ba3c_amd import duel as D
    n = 29 * 4000
    rng = int(D.initial_game(1, seed)[0, 9]) & M32
    for start in ((4, 7), (4, 19)):
        hs, ys = np.zeros(20, np.int64), np.zeros(71, np.int64)
        for _ in range(n):
            rng, h, y = D.draw_start(rng, start)
            hs[h] += 1
            ys[y] += 1
        span = start[1] - start[0] + 1
        print("seed %d start %r: h %r y %r" % (seed, start, hs[hs > 0].tolist(), ys[ys > 0].tolist()))
        assert hs[start[0]:start[1] + 1].sum() == n and ys[14:71:2].sum() == n
        assert (np.abs(hs[start[0]:start[1] + 1] - n / span) <= 0.15 * n / span).all()
        assert (np.abs(ys[14:71:2] - n / 29) <= 0.15 * n / 29).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_skip_and_sticky_frequencies_per_side(seed):
    """3000 decisions of 2-4 at 0.25 (100 games x 30): k's three values 1000 +- 15 % each, each
    side's sticky share in [0.22, 0.28], and the two sides' draws differ from each other about
    as often as independent ones would (2 * 0.25 * 0.75 = 0.375; [0.32, 0.43])."""
    from ba3c_amd import duel as D
    G, q16 = 100, 16384
    game, aux = D.initial_rows(G, seed), D.initial_aux(G, seed)
    counts = {2: 0, 3: 0, 4: 0}
    sticky, differ, steps = [0, 0], 0, 0
    for d in range(30):
        # the decision's draws, read off the aux rows' generators; the oracle must consume them
        x = aux.astype(np.int64) & M32
        k = 2 + (D.frameskip.lcg(x[:, 0]) >> 16) % 3
        xa, xb = x[:, 1], x[:, 2]
        for j in range(4):
            live = j < k
            xa, xb = np.where(live, D.frameskip.lcg(xa), xa), np.where(live, D.frameskip.lcg(xb), xb)
            sa, sb = ((xa >> 8) & 0xFFFF) < q16, ((xb >> 8) & 0xFFFF) < q16
            sticky[0] += int((live & sa).sum())
            sticky[1] += int((live & sb).sum())
            differ += int((live & (sa != sb)).sum())
        t0 = game[:, 8].copy()
        act = np.concatenate([np.full(G, 2 + d % 2), np.full(G, 4 + d % 2)])      # never FIRE: no end
        _, over, _ = D.decide_numpy(game, aux, act, 10 ** 9, 2, 4, q16)
        assert not over.any() and (game[:, 8] - t0 == k).all()    # the oracle ran the k it drew
        assert ((aux[:, 1].astype(np.int64) & M32) == xa).all() and ((aux[:, 2].astype(np.int64) & M32) == xb).all()
        for v in k.tolist():
            counts[v] += 1
        steps += int(k.sum())
    shares = [s / steps for s in sticky]
    print("seed %d: k counts %r, sticky shares %r, differ %.4f" % (seed, counts, shares, differ / steps))
    assert min(counts.values()) >= 850 and max(counts.values()) <= 1150, counts
    assert all(0.22 <= s <= 0.28 for s in shares), shares
    assert sticky[0] != sticky[1] and 0.32 <= differ / steps <= 0.43, differ / steps


# ---- contact -------------------------------------------------------------------------------
def _punches(start, G=64, steps=600, limit=300, seed=0):
    """Uniform-random against uniform-random on the oracle: landed punches (a step in which a
    score rose; on the step that ends an episode, a non-zero reward) per game step."""
    from ba3c_amd import duel as D
    rs = np.random.RandomState(seed)
    game = D.initial_rows(G, seed, start)
    landed = 0
    for _ in range(steps):
        before = game[:, 6:8].copy()
        reward, over, _ = D.step_numpy(game, rs.randint(18, size=2 * G), limit, start)
        o = over[:G]
        landed += int(((game[:, 6:8] > before) & ~o[:, None]).sum()) + int((o & (reward[:G] != 0)).sum())
    return landed / float(G * steps)


def test_a_start_within_reach_at_least_doubles_the_contact_of_random_play():
    fixed, near = _punches(None), _punches((4, 7))
    print("punches per 1000 game steps: fixed start %.2f, gap 8-14 %.2f, ratio %.2f"
          % (1000 * fixed, 1000 * near, near / fixed))
    assert fixed > 0 and near >= 2 * fixed


# ---- flags, C ABI --------------------------------------------------------------------------
SELF_PLAY = "-e GridBoxing-v0 --num_actions 18 --self_play "


def test_the_duel_start_flag_and_self_play_with_its_own_frame_skip():
    from ba3c_amd import duel as D
    from ba3c_amd import flags as F
    parse = lambda s, **kw: F.resolve(F.build_parser().parse_args(s.split()), **kw)
    for argv, gap, start in (("", (38, 38), None), ("--duel_start 38", (38, 38), None),
                             ("--duel_start 8", (8, 8), (4, 4)), ("--duel_start 8-14", (8, 14), (4, 7)),
                             ("--duel_start 8-38", (8, 38), (4, 19)), ("--duel_start 14-14", (14, 14), (7, 7)),
                             ("--duel_start 36-38", (36, 38), (18, 19))):
        a = parse(SELF_PLAY + argv)
        assert a.duel_start == gap and D.start_from_gap(a.duel_start) == start
    # self-play's own frame skip: the run's setting, for the games and the evaluation alike
    a = parse(SELF_PLAY + "--duel_frame_skip 2-4 --duel_sticky 0.25 --duel_start 8-14 --nr_eval 2")
    assert (a.duel_frame_skip, a.duel_sticky, a.duel_start, a.nr_eval) == ((2, 4), 0.25, (8, 14), 2)
    assert (a.play_frame_skip, a.play_sticky) == ((2, 4), 0.25) and (a.frame_skip, a.sticky) == (1, 0.0)
    assert parse(SELF_PLAY + "--duel_frame_skip 4").play_frame_skip == 4
    assert parse(SELF_PLAY + "--duel_sticky 0.25").play_sticky == 0.25
    a = parse(SELF_PLAY)
    assert (a.play_frame_skip, a.play_sticky, a.duel_frame_skip, a.duel_sticky) == (1, 0.0, 1, 0.0)
    a = parse("-e GridBoxing-v0 --num_actions 18 --frame_skip 2-4 --sticky 0.25")      # single-player
    assert (a.play_frame_skip, a.play_sticky) == ((2, 4), 0.25)
    # the default needs nothing; the match tool plays two-player games without --self_play
    assert parse("").duel_start == (38, 38) and parse("-e GridBoxing-v0 --num_actions 18 --duel_start 38")
    assert parse("-e GridBoxing-v0 --num_actions 18 --duel_start 8-14", duel_tool=True).duel_start == (8, 14)
    for bad in (SELF_PLAY + "--duel_start 9", SELF_PLAY + "--duel_start 6", SELF_PLAY + "--duel_start 40",
                SELF_PLAY + "--duel_start 14-8", SELF_PLAY + "--duel_start 8-15", SELF_PLAY + "--duel_start 0",
                SELF_PLAY + "--duel_start a", SELF_PLAY + "--duel_start 8-10-12", SELF_PLAY + "--duel_start 8-",
                SELF_PLAY + "--duel_frame_skip 0", SELF_PLAY + "--duel_frame_skip 2-17",
                SELF_PLAY + "--duel_sticky 1.5", SELF_PLAY + "--duel_frame_skip a",
                SELF_PLAY + "--frame_skip 2", SELF_PLAY + "--sticky 0.25",      # these stay single-player's
                SELF_PLAY + "--frame_skip 2-4 --duel_frame_skip 2-4",
                "-e GridBoxing-v0 --num_actions 18 --duel_frame_skip 4", "--duel_sticky 0.25",
                "-e GridBreakout-v0 --duel_frame_skip 4",
                "-e GridBoxing-v0 --num_actions 18 --duel_start 8-14", "--duel_start 8",
                "-e GridBreakout-v0 --duel_start 8-14", "-e GridBreakout-v0 --self_play --duel_start 8-14"):
        with pytest.raises(SystemExit) as e:
            parse(bad)
        assert e.value.code, bad
    for bad in ("--random_b --self_play --duel_start 8-14", "--random_b --duel_start 9",
                "--random_b --duel_start 8-14 -e GridBreakout-v0", "--random_b --record d --scale 9",
                "--random_b --record d --every 0", "--duel_start 8-14",
                "--random_b --duel_frame_skip 4"):
        with pytest.raises(SystemExit) as e:
            D.main(bad.split())
        assert e.value.code, bad
    for gap, want in ((38, None), ("38", None), (8, (4, 4)), ("8-14", (4, 7)), ((8, 38), (4, 19))):
        assert D.start_from_gap(gap) == want
    for bad in (7, 6, 40, "14-8", (8, 14, 20), "x"):
        with pytest.raises(ValueError):
            D.start_from_gap(bad)


def test_duel_vec_refuses_bad_settings_before_it_touches_a_device():
    from ba3c_amd import duel as D
    for kw in (dict(frame_skip=0), dict(frame_skip=17), dict(frame_skip=(3, 2)), dict(sticky=1.5),
               dict(start=(3, 7)), dict(start=(4, 20)), dict(start=(8, 7))):
        with pytest.raises(ValueError):
            D.BoxingDuelDecisionVec(2, device="cuda:99", **kw)


def test_capi_decide_argument_checks_without_gpu():
    from ba3c_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "ba3c_boxing_duel_decide")
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    odd8 = ctypes.c_void_p(p.value + 8)
    odd1 = ctypes.c_void_p(p.value + 1)
    f = lib.ba3c_boxing_duel_decide

    def call(game=p, aux=p, action=p, n=1, limit=10, lo=2, hi=4, q16=16384, s_lo=4, s_hi=7, reward=p,
             over=p, ep=p, frame=None, state=None):
        return f(None, game, aux, action, n, limit, lo, hi, q16, s_lo, s_hi, reward, over, ep, frame, state)

    def refused(word, **kw):
        assert call(**kw) == 1, kw
        assert word in lib.ba3c_last_error(), (kw, lib.ba3c_last_error())

    # everything ba3c_boxing_duel_step refuses
    refused(b"game", game=None)
    refused(b"action", action=None)
    refused(b"n_games", n=0)
    refused(b"n_games", n=-3)
    refused(b"limit", limit=0)
    for name in ("reward", "over", "ep"):
        refused(b"output", **{name: None})
    refused(b"aligned", game=odd)
    refused(b"aligned", frame=odd1)
    refused(b"aligned", state=odd)
    # and the decision's own
    refused(b"aux", aux=None)
    refused(b"aux", aux=odd)
    refused(b"aux", aux=odd8)
    for lo, hi in ((0, 4), (5, 4), (1, 17), (-1, -1)):
        refused(b"skip", lo=lo, hi=hi)
    for q16 in (-1, 65537):
        refused(b"sticky", q16=q16)
    for s_lo, s_hi in ((3, 7), (8, 7), (4, 20), (19, 20), (0, 0)):
        refused(b"start", s_lo=s_lo, s_hi=s_hi)
