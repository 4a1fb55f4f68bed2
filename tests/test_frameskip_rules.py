"""Frame skip and sticky actions on the CPU (ba3c_amd.frameskip, the oracle; envs.FrameSkipPlayer,
its scalar restatement): the decision against the games' own step_numpy, episode ends inside a
skip, stickiness, the frequencies of the two draws, the launcher flags and the C ABI's argument
checks.  No kernel is launched here."""
import numpy as np
import pytest

GAME_NAMES = ["breakout", "boxing"]
T = 8                                            # the column of t in both games' rows


def _game(name):
    from ba3c_amd import boxing, breakout
    return {"breakout": breakout, "boxing": boxing}[name]


def _actions(K, rs, E):
    return rs.randint(K.NUM_ACTIONS, size=E).astype(np.int64)


# ---- (a) lo = hi = 1, q16 = 0 is the plain step -----------------------------------------
@pytest.mark.parametrize("name", GAME_NAMES)
def test_skip_one_without_stickiness_is_the_plain_step(name):
    from ba3c_amd import frameskip as F
    K = _game(name)
    E, limit = 9, 70
    rs = np.random.RandomState(3)
    plain, game, aux = K.initial_game(E, 4), K.initial_game(E, 4), F.initial_aux(E, 4)
    overs = 0
    for s in range(200):
        a = _actions(K, rs, E)
        want = K.step_numpy(plain, a, limit)
        got = F.step_numpy(K, game, aux, a, limit, 1, 1, 0)
        assert (game == plain).all(), s
        for w, g in zip(want, got):
            assert w.dtype == g.dtype and (w == g).all(), s
        assert (aux[:, F.PREV] == np.where(got[1], 0, a)).all(), s
        overs += int(got[1].sum())
    assert overs >= 2 * E


# ---- (b) a fixed k is k plain steps under the same action --------------------------------
@pytest.mark.parametrize("name", GAME_NAMES)
def test_fixed_skip_equals_four_plain_steps_with_rewards_summed(name):
    from ba3c_amd import frameskip as F
    K = _game(name)
    E, limit = 9, 10 ** 6
    rs = np.random.RandomState(5)
    plain, game, aux = K.initial_game(E, 2), K.initial_game(E, 2), F.initial_aux(E, 2)
    compared = rewarded = 0
    for s in range(120):
        a = _actions(K, rs, E)
        before = plain.copy()
        R, ended = np.zeros(E), np.zeros(E, bool)
        for _ in range(4):
            r, o, _ = K.step_numpy(plain, a, limit)
            R += np.where(ended, 0.0, r)
            ended |= o
        reward, over, _ = F.step_numpy(K, game, aux, a, limit, 4, 4, 0)
        keep = ~ended                                   # no sub-step ended an episode
        assert (over == ended).all(), s
        assert (game[keep] == plain[keep]).all() and (reward[keep] == R[keep]).all(), s
        assert (game[keep, T] == before[keep, T] + 4).all(), s
        compared += int(keep.sum())
        rewarded += int((R[keep] != 0).sum())
        plain[ended] = game[ended]                      # continue both from the same rows
    assert compared > 100 * E and rewarded > 0


# ---- (c) an episode ends inside a skip ----------------------------------------------------
@pytest.mark.parametrize("name", GAME_NAMES)
def test_episode_end_inside_a_skip_drops_the_remaining_sub_steps(name):
    from ba3c_amd import frameskip as F
    K = _game(name)
    E, limit, warm = 9, 40, 38
    rs = np.random.RandomState(11)
    game = K.initial_game(E, 6)
    for s in range(warm):                               # bring every row to t = limit - 2
        a = np.full(E, 1, np.int64) if s % 3 == 0 else _actions(K, rs, E)
        _, over, _ = K.step_numpy(game, a, 10 ** 6)
        assert not over.any()
    assert (game[:, T] == limit - 2).all()
    a = _actions(K, rs, E)
    ref = game.copy()
    r1, o1, _ = K.step_numpy(ref, a, limit)
    r2, o2, ep2 = K.step_numpy(ref, a, limit)
    assert not o1.any() and o2.all()
    aux = F.initial_aux(E, 6)
    aux[:, F.PREV] = 3
    rng2 = aux[:, F.RNG2].copy()
    reward, over, ep = F.step_numpy(K, game, aux, a, limit, 4, 4, 0)
    assert over.all() and (ep == ep2).all()             # the score at the second sub-step
    assert (reward == r1 + r2).all()                    # two sub-steps only
    assert (game == ref).all() and (game[:, T] == 0).all()
    fresh = K.initial_game(E, 6)
    rng_col = 9
    cols = [c for c in range(16) if c != rng_col]
    assert (game[:, cols] == fresh[:, cols]).all()      # a fresh episode (the row's rng is kept)
    assert (aux[:, F.PREV] == 0).all()
    want = rng2.astype(np.int64) & 0xFFFFFFFF
    for _ in range(3):                                  # the draw of k and two sub-steps' draws
        want = F.lcg(want)
    assert ((aux[:, F.RNG2].astype(np.int64) & 0xFFFFFFFF) == want).all()


# ---- (d) stickiness ------------------------------------------------------------------------
def test_fully_sticky_never_leaves_the_initial_noop_and_zero_never_sticks():
    from ba3c_amd import breakout as K
    from ba3c_amd import frameskip as F
    E, limit = 9, 10 ** 6
    rs = np.random.RandomState(0)
    game, aux = K.initial_game(E, 1), F.initial_aux(E, 1)
    for s in range(60):
        a = rs.choice([K.RIGHT, K.LEFT, K.FIRE], size=E).astype(np.int64)
        F.step_numpy(K, game, aux, a, limit, 2, 4, F.Q16_ONE)
        assert (game[:, K.PX] == K.PX_START).all() and not game[:, K.IN_PLAY].any(), s
        assert (aux[:, F.PREV] == 0).all(), s
    assert (game[:, T] >= 2 * 60).all()
    # q16 = 0: every sub-step plays the chosen action, whatever was remembered
    game, aux = K.initial_game(E, 1), F.initial_aux(E, 1)
    px = game[:, K.PX].astype(np.int64)
    for s in range(60):
        a = np.where(rs.random_sample(E) < 0.5, K.RIGHT, K.LEFT).astype(np.int64)
        t0 = game[:, T].copy()
        F.step_numpy(K, game, aux, a, limit, 1, 3, 0)
        for e in range(E):
            for _ in range(int(game[e, T] - t0[e])):
                px[e] = min(px[e] + 3, K.PX_MAX) if a[e] == K.RIGHT else max(px[e] - 3, 0)
        assert (game[:, K.PX] == px).all() and (aux[:, F.PREV] == a).all(), s


@pytest.mark.parametrize("name", GAME_NAMES)
def test_out_of_range_actions_are_noop_and_remembered_as_zero(name):
    from ba3c_amd import frameskip as F
    K = _game(name)
    odd = np.array([-1, 32, 1 << 40], np.int64)
    E, limit = odd.size, 10 ** 6
    weird, aux_w = K.initial_game(E, 3), F.initial_aux(E, 3)
    noop, aux_n = K.initial_game(E, 3), F.initial_aux(E, 3)
    aux_w[:, F.PREV] = aux_n[:, F.PREV] = 1
    for s in range(40):
        got = F.step_numpy(K, weird, aux_w, np.roll(odd, s), limit, 2, 4, 16384)
        want = F.step_numpy(K, noop, aux_n, np.zeros(E, np.int64), limit, 2, 4, 16384)
        assert (weird == noop).all() and (aux_w == aux_n).all(), s
        assert all((g == w).all() for g, w in zip(got, want)), s
        assert set(aux_w[:, F.PREV].tolist()) <= {0, 1}, s
    assert (aux_w[:, F.PREV] == 0).all()                # the FIRE remembered at first has faded
    # 31 is inside the remembered range (and a NOOP to both games); 32 is not
    game, aux = K.initial_game(2, 0), F.initial_aux(2, 0)
    F.step_numpy(K, game, aux, np.array([31, 32], np.int64), limit, 1, 1, 0)
    assert aux[:, F.PREV].tolist() == [31, 0]


# ---- (e) frequencies of the two draws, on the oracle alone -------------------------------
@pytest.mark.parametrize("seed", [0, 1, 7])
def test_skip_and_sticky_frequencies(seed):
    from ba3c_amd import breakout as K
    from ba3c_amd import frameskip as F
    game, aux = K.initial_game(1, seed), F.initial_aux(1, seed)
    counts = {2: 0, 3: 0, 4: 0}
    sticky = steps = 0
    for d in range(3000):
        # the decision's draws, read off the aux row's generator; the oracle must consume exactly
        # these (checked below through k, which shows in t, and through the generator's state)
        chosen = 2 + d % 2
        rng2 = int(aux[0, F.RNG2]) & 0xFFFFFFFF
        rng2 = F.lcg(rng2)
        k = 2 + (rng2 >> 16) % 3
        for _ in range(k):
            rng2 = F.lcg(rng2)
            sticky += ((rng2 >> 8) & 0xFFFF) < 16384
        t0 = int(game[0, T])
        _, over, _ = F.step_numpy(K, game, aux, np.array([chosen], np.int64), 10 ** 9, 2, 4, 16384)
        assert not over[0] and int(game[0, T]) - t0 == k       # the oracle ran the k it drew
        assert (int(aux[0, F.RNG2]) & 0xFFFFFFFF) == rng2      # ... and k + 1 draws
        counts[k] += 1
        steps += k
    print("seed %d: k counts %r, sticky share %.4f" % (seed, counts, sticky / steps))
    assert min(counts.values()) >= 850, counts
    assert 0.22 <= sticky / steps <= 0.28, sticky / steps


# ---- (f) the scalar player ------------------------------------------------------------------
@pytest.mark.parametrize("name,limit", [("breakout", 23), ("boxing", 23)])
def test_frame_skip_player_equals_the_oracle(name, limit):
    from ba3c_amd import envs
    from ba3c_amd import frameskip as F
    K = _game(name)
    E, seed, lo, hi, q16 = 5, 4, 2, 4, 16384
    Player = envs.PLAYERS[name]
    players = [envs.FrameSkipPlayer(Player(e, K.NUM_ACTIONS, seed, limit=limit), lo, hi, q16, seed=seed, idx=e)
               for e in range(E)]
    game, aux = K.initial_game(E, seed), F.initial_aux(E, seed)
    assert [p.game_row() for p in players] == game.tolist()
    assert [p.aux_row() for p in players] == aux.tolist()
    rs = np.random.RandomState(9)
    mid_skip = 0
    for s in range(300):
        a = rs.randint(-1, K.NUM_ACTIONS + 1, size=E).astype(np.int64)     # -1 and A: out of range
        k = lo + ((F.lcg(aux[:, F.RNG2].astype(np.int64) & 0xFFFFFFFF) >> 16) % (hi - lo + 1))
        left = limit - game[:, T]
        reward, over, ep = F.step_numpy(K, game, aux, a, limit, lo, hi, q16)
        mid_skip += int((over & (left < k)).sum())      # ended with sub-steps of its k left over
        for e, p in enumerate(players):
            r, o = p.action(int(a[e]))
            assert (r, o) == (reward[e], bool(over[e])), (s, e)
            assert isinstance(r, float)
            assert p.game_row() == game[e].tolist() and p.aux_row() == aux[e].tolist(), (s, e)
            if o:
                assert p.player.last_ep_score == ep[e] and p.prev == 0
        frames = K.render_numpy(game)
        for e, p in enumerate(players):
            assert (p.current_state() == frames[e]).all(), (s, e)
    assert mid_skip >= 10
    assert all(len(p.stats["score"]) >= 10 for p in players)


def test_get_player_inserts_the_frame_skip_player_under_the_history():
    from ba3c_amd import envs
    from ba3c_amd import simulator as S
    pl = envs.get_player(idx=2, num_actions=4, seed=5, train=True, game="breakout", limit=50,
                         frame_skip=(2, 4), sticky=0.25)
    assert isinstance(pl, envs.HistoryFramePlayer) and isinstance(pl.player, envs.FrameSkipPlayer)
    fs = pl.player
    assert (fs.lo, fs.hi, fs.q16) == (2, 4, 16384) and fs.player.limit == 50
    assert fs.aux_row() == [(5002 ^ 0x9E3779B9) - (1 << 32), 0] and fs.player.rng == 5002
    overs = 0
    for i in range(60):
        r, over = pl.action(i % 4)
        overs += over
        assert pl.current_state().shape == (84, 84, 4)
    assert overs >= 2 and len(pl.stats["score"]) == overs         # limit counts game steps
    # the defaults are the chain as before
    base = envs.get_player(game="breakout", train=True)
    assert isinstance(base, envs.LimitLengthPlayer) and isinstance(base.player.player, envs.BreakoutPlayer)
    with pytest.raises(ValueError):
        envs.get_player(game="synthetic", frame_skip=4)
    with pytest.raises(ValueError):
        envs.get_player(game="boxing", num_actions=18, frame_skip=(5, 2))
    w = S.SyntheticSimulatorWorker(3, "ipc:///nowhere/c2s", "ipc:///nowhere/s2c", num_actions=18,
                                   seed=10, game="boxing", frame_skip=4, sticky=0.5)
    inner = w._build_player().player
    assert isinstance(inner, envs.FrameSkipPlayer) and (inner.lo, inner.hi, inner.q16) == (4, 4, 32768)
    assert inner.aux_row()[0] == ((13003 ^ 0x9E3779B9) & 0xFFFFFFFF) - (1 << 32)


# ---- (g) the launcher flags ----------------------------------------------------------------
def test_launcher_flags():
    from ba3c_amd import flags as F
    parse = lambda s: F.resolve(F.build_parser().parse_args(s.split()))
    brk = "-e GridBreakout-v0 "
    assert parse(brk + "--frame_skip 4").frame_skip == 4
    assert parse(brk + "--frame_skip 2-4").frame_skip == (2, 4)
    a = parse("-e GridBoxing-v0 --num_actions 18 --frame_skip 2-4 --sticky 0.25 --nr_eval 2")
    assert (a.frame_skip, a.sticky, a.nr_eval) == ((2, 4), 0.25, 2)
    assert parse(brk + "--sticky 1").sticky == 1.0 and parse(brk + "--frame_skip 16").frame_skip == 16
    for bad in ("--frame_skip 0", "--frame_skip 5-2", "--frame_skip 1-17", "--frame_skip 17",
                "--frame_skip x", "--frame_skip 1-2-3", "--sticky 1.5", "--sticky -0.1"):
        with pytest.raises(SystemExit):
            parse(brk + bad)
    for no_game in ("--frame_skip 4", "--sticky 0.25", "-e Breakout-v0 --frame_skip 2-4"):
        with pytest.raises(SystemExit):
            parse(no_game)
    # the defaults: every other flag as before, the two new ones at "off", no game needed
    d = vars(parse(""))
    assert d.pop("frame_skip") == 1 and d.pop("sticky") == 0.0
    assert d["environment"] == "Breakout-v0" and d["nr_eval"] == 0
    assert parse("--frame_skip 1 --sticky 0").frame_skip == 1     # spelled-out defaults need no game
    assert set(F.GAMES) == {"GridBreakout-v0", "GridBoxing-v0"}


def test_setting_parses_and_checks():
    from ba3c_amd import frameskip as F
    assert F.setting() is None and F.setting(1, 0.0) is None and F.setting((1, 1), 0) is None
    assert F.setting(4) == (4, 4, 0) and F.setting((2, 4), 0.25) == (2, 4, 16384)
    assert F.setting("2-4", 0.9) == (2, 4, 58982) and F.setting(1, 1.0) == (1, 1, 65536)
    for bad in ((0, 0.0), ((5, 2), 0.0), ((1, 17), 0.0), (1, 1.5), (1, -0.5), ((1, 2, 3), 0.0)):
        with pytest.raises(ValueError):
            F.setting(*bad)
    with pytest.raises(ValueError):
        F.step_numpy(None, None, None, None, 1, 3, 2, 0)


# ---- (h) the C ABI's argument checks -------------------------------------------------------
@pytest.mark.parametrize("fn", ["ba3c_breakout_step_skip", "ba3c_boxing_step_skip"])
def test_capi_argument_checks_without_gpu(fn):
    import ctypes

    from ba3c_amd import _lib as L
    lib = L.load()
    f = getattr(lib, fn)
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 16 == 0
    odd4, odd8 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 8)

    def call(game=p, aux=p, action=p, n=1, limit=10, lo=2, hi=4, q16=16384, reward=p, over=p, ep=p,
             frame=None, state=None):
        return f(None, game, aux, action, n, limit, lo, hi, q16, reward, over, ep, frame, state)
    err = lib.ba3c_last_error
    # what the plain step refuses
    assert call(game=None) == 1 and b"game" in err()
    assert call(action=None) == 1
    assert call(n=0) == 1
    assert call(limit=0) == 1 and b"limit" in err()
    for out in ("reward", "over", "ep"):
        assert call(**{out: None}) == 1 and b"output" in err()
    assert call(game=odd4) == 1 and b"aligned" in err()
    assert call(game=odd8) == 1 and b"aligned" in err()
    assert call(state=odd8) == 1 and b"aligned" in err()
    assert call(frame=ctypes.c_void_p(p.value + 2)) == 1 and b"aligned" in err()
    # aux
    assert call(aux=None) == 1 and b"aux" in err()
    assert call(aux=odd4) == 1 and b"aux" in err() and b"aligned" in err()
    # the ranges
    for lo, hi in ((0, 4), (-1, 1), (5, 2), (1, 17), (17, 17)):
        assert call(lo=lo, hi=hi) == 1 and b"skip" in err(), (lo, hi)
    for q16 in (-1, 65537, 1 << 20):
        assert call(q16=q16) == 1 and b"sticky" in err(), q16
    assert lib.ba3c_version() == 1
