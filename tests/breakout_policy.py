"""Shared pieces of the GridBreakout tests: the scripted policy, crafted game rows, and one
cached CPU trajectory per case (the oracle side: step_numpy on the rows, BreakoutPlayer's
`last_events` log on the same actions)."""
import functools

import numpy as np

NAMES = ["px", "bx", "by", "vx", "vy", "in_play", "lives", "score", "t", "rng",
         "b0", "b1", "b2", "b3", "b4", "b5"]
EVENTS = ["wall", "ceiling", "brick7", "brick4", "brick1", "paddle", "lost", "over_lives",
          "over_clear", "over_limit"]


def make_row(**kw):
    """A fresh-episode game row with the named fields replaced."""
    from ba3c_amd import breakout as K
    row = K.initial_game(1, 0)[0].copy()
    for k, v in kw.items():
        row[NAMES.index(k)] = v
    return row


def player_from_row(row, limit=None):
    """A BreakoutPlayer whose episode state is `row`."""
    from ba3c_amd.envs import BreakoutPlayer
    p = BreakoutPlayer(0, 4, 0, limit=limit)
    (p.px, p.bx, p.by, p.vx, p.vy, p.in_play, p.lives, p.score, p.t) = (int(v) for v in row[:9])
    p.rng = int(row[9]) % (1 << 32)
    p.bricks = [int(v) for v in row[10:16]]
    return p


def scripted_actions(game, rs):
    """The issue's scripted policy for every row of `game`: env e has skill
    p = 0.3 + 0.69 e/(E-1); FIRE with probability 0.9 when the ball is not in play; otherwise
    with probability p steer px+5 towards bx (dead zone +-1), else a uniform random action."""
    E = game.shape[0]
    p = 0.3 + 0.69 * np.arange(E) / max(E - 1, 1)
    u = rs.random_sample(E)
    ra = rs.randint(4, size=E)
    px, bx, in_play = game[:, 0].astype(np.int64), game[:, 1].astype(np.int64), game[:, 5] != 0
    c = px + 5
    steer = np.where(c < bx - 1, 2, np.where(c > bx + 1, 3, 0))
    act = np.where(in_play, np.where(u < p, steer, ra), np.where(u < 0.9, 1, ra))
    return act.astype(np.int64)


class Trajectory(object):
    """actions [S,E], games [S+1,E,16] (games[0] the initial rows), reward [S,E] float64,
    over [S,E] bool, ep_score [S,E] int32, events: {name: count} from BreakoutPlayer."""


@functools.lru_cache(maxsize=None)
def trajectory(E, steps, limit, seed, with_events=False):
    from ba3c_amd import breakout as K
    from ba3c_amd.envs import BreakoutPlayer
    rs = np.random.RandomState(seed)
    game = K.initial_game(E, seed)
    players = [BreakoutPlayer(e, 4, seed, limit=limit) for e in range(E)] if with_events else []
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
