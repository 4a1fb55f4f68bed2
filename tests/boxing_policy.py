"""Shared pieces of the GridBoxing tests: the scripted policy, crafted game rows, and one cached
CPU trajectory per case (the oracle side: step_numpy on the rows, BoxingPlayer's `last_events`
log on the same actions)."""
import functools

import numpy as np

NAMES = ["ax", "ay", "ox", "oy", "a_cd", "o_cd", "a_score", "o_score", "t", "rng"] + ["pad%d" % i for i in range(6)]
EVENTS = ["hit1", "hit2", "miss", "got1", "got2", "ko_win", "ko_loss", "over_clock", "over_limit"]


def lcg(rng):
    return (rng * 1664525 + 1013904223) % (1 << 32)


def rng_where(pred):
    """The smallest generator state whose NEXT draw r = lcg(rng) >> 16 satisfies pred(r)."""
    return next(s for s in range(1 << 16) if pred(lcg(s) >> 16))


# r & 3 != 0: the opponent closes in; bit 8 set: it does not punch (clear: it punches if it can)
QUIET = rng_where(lambda r: r & 3 and (r >> 8) & 1)
PUNCH = rng_where(lambda r: r & 3 and not (r >> 8) & 1)


def make_row(**kw):
    """A fresh-episode game row with the named fields replaced."""
    from ba3c_amd import boxing as K
    row = K.initial_game(1, 0)[0].copy()
    for k, v in kw.items():
        row[NAMES.index(k)] = v
    return row


def player_from_row(row, limit=None):
    """A BoxingPlayer whose episode state is `row`."""
    from ba3c_amd.envs import BoxingPlayer
    p = BoxingPlayer(0, 18, 0, limit=limit)
    (p.ax, p.ay, p.ox, p.oy, p.a_cd, p.o_cd, p.a_score, p.o_score, p.t) = (int(v) for v in row[:9])
    p.rng = int(row[9]) % (1 << 32)
    return p


def chase_actions(game):
    """The chase-align-punch script for every row of `game`: move towards the opponent's row
    while more than 4 px off it, close in horizontally while more than 9 px away, and punch
    whenever the cooldown allows."""
    from ba3c_amd import boxing as K
    g = game.astype(np.int64)
    ax, ay, ox, oy, a_cd = (g[:, i] for i in (K.AX, K.AY, K.OX, K.OY, K.A_CD))
    dy = np.where(np.abs(ay - oy) > K.REACH_Y, np.sign(oy - ay), 0)
    dx = np.where(np.abs(ax - ox) > K.REACH_NEAR, np.sign(ox - ax), 0)
    fire = a_cd <= 1                                   # the step decrements before it tests
    table = {(x, y, f): K.action_id(x, y, f) for x in (-1, 0, 1) for y in (-1, 0, 1) for f in (0, 1)}
    return np.array([table[(int(x), int(y), int(f))] for x, y, f in zip(dx, dy, fire)], np.int64)


def scripted_actions(game, rs):
    """Env e follows chase_actions with probability p = 0.1 + 0.8 e/(E-1), else plays a
    uniform random one of the 18 actions."""
    E = game.shape[0]
    p = 0.1 + 0.8 * np.arange(E) / max(E - 1, 1)
    u = rs.random_sample(E)
    ra = rs.randint(18, size=E)
    return np.where(u < p, chase_actions(game), ra).astype(np.int64)


class Trajectory(object):
    """actions [S,E], games [S+1,E,16] (games[0] the initial rows), reward [S,E] float64,
    over [S,E] bool, ep_score [S,E] int32, events: {name: count} from BoxingPlayer."""


@functools.lru_cache(maxsize=None)
def trajectory(E, steps, limit, seed, with_events=False):
    from ba3c_amd import boxing as K
    from ba3c_amd.envs import BoxingPlayer
    rs = np.random.RandomState(seed)
    game = K.initial_game(E, seed)
    players = [BoxingPlayer(e, 18, seed, limit=limit) for e in range(E)] if with_events else []
    tr = Trajectory()
    tr.actions = np.zeros((steps, E), np.int64)
    tr.games = np.zeros((steps + 1, E, 16), np.int32)
    tr.reward = np.zeros((steps, E), np.float64)
    tr.over = np.zeros((steps, E), bool)
    tr.ep_score = np.zeros((steps, E), np.int32)
    tr.events = dict.fromkeys(EVENTS, 0)
    tr.games[0] = game
    for s in range(steps):
        a = scripted_actions(game, rs)
        tr.actions[s] = a
        tr.reward[s], tr.over[s], tr.ep_score[s] = K.step_numpy(game, a, limit)
        tr.games[s + 1] = game
        for e, p in enumerate(players):
            r, o = p.action(int(a[e]))
            assert (r, o) == (tr.reward[s, e], tr.over[s, e]) and p.game_row() == game[e].tolist()
            for name in p.last_events:
                tr.events[name] += 1
    for v in (tr.actions, tr.games, tr.reward, tr.over, tr.ep_score):
        v.setflags(write=False)
    return tr


def history_push_numpy(state, frames, over):
    """HistoryFramePlayer.action for [E,84,84,4] states: append the frame; on over the history
    is cleared to zeros + frame."""
    new = np.concatenate([state[..., 1:], frames[..., None]], axis=-1)
    new[over, :, :, :3] = 0
    return new
