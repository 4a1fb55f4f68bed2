"""GridPong's rules on the CPU: step_numpy against hand-worked rows, `envs.PongPlayer` against step_numpy /
render_numpy step for step, the baseline policies' order, and the rows in flags.ALL_GAMES / envs.PLAYERS."""
import numpy as np
import pytest

from ba3c_amd import gridpong as K
from gridpong_policy import tracking_actions

# rng values by their step's draw r = lcg(rng) >> 16: LAPSE: r & 7 = 0, the opponent holds still; MOVE:
# r & 7 = 3, it moves; SERVE_*: a lapse and the serve's bits (row 33 upward at 1, row 52 downward at 2)
LAPSE, MOVE, SERVE_TOP, SERVE_BOTTOM = 1, 3, 41, 81
FIELDS = ("py", "oy", "bx", "by", "vx", "vy", "mine", "theirs", "t", "rng", "hits", "serve")
FRESH = dict(py=42, oy=42, bx=328, by=368, vx=10, vy=0, mine=0, theirs=0, t=0, hits=0, serve=16)


def make_row(**kw):
    f = dict(py=42, oy=42, bx=328, by=368, vx=10, vy=0, mine=0, theirs=0, t=5, rng=LAPSE, hits=0, serve=0)
    f.update(kw)
    return np.array([f[k] for k in FIELDS] + [0] * 4, np.int64).astype(np.uint32).view(np.int32)


# (row, action, limit, the fields the step changes besides t and rng, reward, over, ep_score)
CASES = {
    "top wall": (dict(bx=300, by=100, vy=-8), 0, 99, dict(bx=310, by=100, vy=8), 0, False, 0),
    "bottom wall": (dict(bx=300, by=636, vy=6), 0, 99, dict(bx=310, by=638, vy=-6), 0, False, 0),
    "hit, top edge": (dict(bx=590, by=330), 0, 99, dict(bx=584, by=330, vx=-10, vy=-12, hits=1), 0, False, 0),
    "hit, centre": (dict(bx=590, by=368), 0, 99, dict(bx=584, vx=-10, vy=1, hits=1), 0, False, 0),
    "hit, bottom edge": (dict(bx=590, by=408), 0, 99, dict(bx=584, vx=-10, vy=12, hits=1), 0, False, 0),
    "one row above the paddle": (dict(bx=590, by=320), 0, 99, dict(bx=600), 0, False, 0),
    "the paddle moves first": (dict(bx=590, by=320), 2, 99, dict(py=40, bx=584, vx=-10, vy=-9, hits=1), 0, False, 0),
    "opponent hit": (dict(bx=66, by=352, vx=-10, vy=3), 0, 99, dict(bx=72, by=355, vx=10, vy=-4, hits=1), 0, False, 0),
    "opponent tracks": (dict(by=200, rng=MOVE), 3, 99, dict(py=44, oy=41, bx=338), 0, False, 0),
    "opponent recentres": (dict(oy=20, serve=9, rng=MOVE), 0, 99, dict(oy=21, serve=8), 0, False, 0),
    "point lost": (dict(bx=616, by=200, vy=5, theirs=4, hits=6), 0, 99,
                   dict(bx=328, by=368, vx=10, vy=0, theirs=5, hits=0, serve=16), -1, False, 0),
    "point won": (dict(bx=40, by=200, vx=-12, vy=5, mine=2, hits=5), 0, 99,
                  dict(bx=328, by=368, vx=-10, vy=0, mine=3, hits=0, serve=16), 1, False, 0),
    "waiting": (dict(serve=5, vx=-10), 2, 99, dict(py=40, serve=4), 0, False, 0),
    "serve after the delay": (dict(serve=1, rng=SERVE_TOP), 0, 99, dict(by=264, vy=-1, serve=0), 0, False, 0),
    "serve on FIRE": (dict(serve=9, vx=-10, rng=SERVE_BOTTOM), 5, 99, dict(py=44, by=416, vy=2, serve=0), 0, False, 0),
    "speed-up at the 4th hit": (dict(bx=590, hits=3), 0, 99, dict(bx=584, vx=-12, vy=1, hits=4), 0, False, 0),
    "speed-up at the 8th hit": (dict(bx=66, vx=-12, hits=7), 0, 99, dict(bx=74, vx=14, vy=1, hits=8), 0, False, 0),
    "the cap": (dict(bx=588, vx=14, hits=40), 0, 99, dict(bx=582, vx=-14, vy=1, hits=41), 0, False, 0),
    "the 21st point wins": (dict(bx=40, vx=-10, mine=20, theirs=7), 0, 99, FRESH, 1, True, 14),
    "the 21st point loses": (dict(bx=616, mine=3, theirs=20), 0, 99, FRESH, -1, True, -18),
    "the step limit": (dict(py=30, mine=3, theirs=5, t=98), 3, 99, FRESH, 0, True, -2),
    "action 6 is NOOP": (dict(), 6, 99, dict(bx=338), 0, False, 0),
    "action 2^32 + 2 is NOOP": (dict(), (1 << 32) + 2, 99, dict(bx=338), 0, False, 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_numpy_equals_the_hand_worked_row(name):
    row, action, limit, changes, reward, over, ep = CASES[name]
    game = make_row(**row).reshape(1, 16)
    stepped = dict(row, t=row.get("t", 5) + 1, rng=(row.get("rng", LAPSE) * 1664525 + 1013904223) % (1 << 32))
    want = make_row(**dict(stepped, **changes))
    got = K.step_numpy(game, np.array([action], np.int64), limit)
    assert game[0].tolist() == want.tolist(), dict(zip(FIELDS, game[0].tolist()))
    assert (got[0].tolist(), got[1].tolist(), got[2].tolist()) == ([float(reward)], [over], [ep])


def first_episodes(policy, n=8, seed=3):
    """ep_score of the first episode of each of n simulators under policy(game, rs) -> actions."""
    game, rs = K.initial_game(n, seed), np.random.RandomState(seed)
    score = np.full(n, 99)
    while (score == 99).any():
        _, over, ep = K.step_numpy(game, policy(game, rs))
        score = np.where(over & (score == 99), ep, score)
    return score


def test_baselines_are_ordered_and_the_script_wins_every_episode():
    noop = first_episodes(lambda g, rs: np.zeros(len(g), np.int64))
    rand = first_episodes(lambda g, rs: rs.randint(K.NUM_ACTIONS, size=len(g)))
    script = first_episodes(tracking_actions)
    assert noop.mean() < rand.mean() < script.mean(), (noop, rand, script)
    assert (script > 0).all() and (noop == -21).all()


def test_player_equals_step_numpy_and_render_numpy_step_for_step():
    from ba3c_amd.envs import PongPlayer
    E, limit, seed = 4, 450, 2
    game, rs = K.initial_game(E, seed), np.random.RandomState(seed)
    players = [PongPlayer(e, seed=seed, limit=limit) for e in range(E)]
    seen = set()
    for s in range(900):
        a = rs.randint(-1, 8, size=E).astype(np.int64)
        a[:2] = tracking_actions(game, rs)[:2]          # two scripted rows, two random ones
        reward, over, ep = K.step_numpy(game, a, limit)
        frames = K.render_numpy(game)
        for e, p in enumerate(players):
            assert p.action(int(a[e])) == (reward[e], bool(over[e])), (s, e)
            assert p.game_row() == game[e].tolist() and (not over[e] or p.last_ep_score == ep[e]), (s, e)
            assert (p.current_state() == frames[e]).all(), (s, e)
            seen |= p.last_events
    assert seen >= {"serve", "wall", "hit", "opp_hit", "speedup", "point", "lost", "over_limit"}, seen


def test_the_tables_know_the_game():
    from ba3c_amd import flags
    from ba3c_amd.envs import PLAYERS, PongPlayer, get_player
    parse = lambda s: flags.resolve(flags.build_parser().parse_args(s.split()))
    args = parse("-e GridPong-v0 --num_actions 6")
    assert (args.channels, args.num_actions) == (1, 6)
    assert flags.ALL_GAMES["GridPong-v0"] == (K.PongVec, 6, "gridpong") and PLAYERS["gridpong"] is PongPlayer
    with pytest.raises(SystemExit):
        parse("-e GridPong-v0 --num_actions 5")
    pl = get_player(game="gridpong", num_actions=6, limit=50)
    assert pl.current_state().shape == (84, 84, 4) and pl.action(1)[1] is False
    with pytest.raises(ValueError):
        get_player(game="pong")
