"""Shared pieces of the two-player GridBoxing tests: a scalar restatement of the written rules
(plain Python ints, independent of duel.step_numpy's array code), crafted and random rows, one
cached CPU trajectory per case, and the scripted sides (on rows for the CPU tests, on the
stacked state for `match`)."""
import functools

import numpy as np

from boxing_policy import chase_actions, make_row

FRESH = (20, 42, 58, 42, 0, 0, 0, 0, 0)
ODD_ACTIONS = (-1, 18, 1 << 40, (1 << 32) + 1, -(1 << 62), (1 << 32) + 17)   # all NOOP
_ALIAS = {"bx": "ox", "by": "oy", "b_cd": "o_cd", "b_score": "o_score"}


def row(**kw):
    """A fresh row with the named fields (ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t, rng)
    replaced."""
    return make_row(**{_ALIAS.get(k, k): v for k, v in kw.items()})


def _components(a):
    """(dx, dy, fire) of ALE's action a as boxing.py's docstring lists the 18 names."""
    names = ["", "F", "U", "R", "L", "D", "UR", "UL", "DR", "DL", "UF", "RF", "LF", "DF", "URF", "ULF",
             "DRF", "DLF"]
    n = names[a] if 0 <= a < 18 else ""
    return ("R" in n) - ("L" in n), ("D" in n) - ("U" in n), "F" in n


def step_scalar(r, a, b, limit):
    """The written rules of duel.py's docstring on one row (a list of 16 ints), as plain ints.
    -> (new row, reward_A, over, ep_score_A or 0)."""
    clamp = lambda v, lo, hi: min(max(v, lo), hi)
    ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t, rng = (int(v) for v in r[:10])
    (dx_a, dy_a, fire_a), (dx_b, dy_b, fire_b) = _components(a), _components(b)
    a_cd, b_cd = max(a_cd - 1, 0), max(b_cd - 1, 0)
    ax, ay = clamp(ax + 2 * dx_a, 4, 74), clamp(ay + 2 * dy_a, 14, 70)
    bx, by = clamp(bx - 2 * dx_b, 4, 74), clamp(by + 2 * dy_b, 14, 70)
    gx, gy = abs(ax - bx), abs(ay - by)
    p = 0 if gy > 4 or gx > 14 else (2 if gx <= 9 else 1)
    b_right = bx >= ax
    pa = pb = 0
    if fire_a and a_cd == 0:
        a_cd, pa = 8, p
    if fire_b and b_cd == 0:
        b_cd, pb = 8, p
    a_score += pa
    b_score += pb
    if pa:
        bx = clamp(bx + (3 if b_right else -3), 4, 74)
    if pb:
        ax = clamp(ax + (-3 if b_right else 3), 4, 74)
    t += 1
    over = a_score >= 100 or b_score >= 100 or t >= 1680 or t >= limit
    ep = a_score - b_score if over else 0
    if over:
        ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t = FRESH
    return [ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t, rng] + [0] * 6, pa - pb, over, ep


def random_rows(rs, n):
    """[n,16] int32 rows: a quarter anywhere in the ring, a quarter within reach of each other,
    a quarter at the ropes, a quarter within reach with scores 96..101 (a step never leaves 100
    or 101 in a row, but the rules are defined and symmetric there too), with cooldowns 0..8,
    t up to one step below the clock and any rng."""
    g = np.zeros((n, 16), np.int64)
    k = np.arange(n) % 4
    g[:, 0], g[:, 1] = rs.randint(4, 75, n), rs.randint(14, 71, n)
    g[:, 2], g[:, 3] = rs.randint(4, 75, n), rs.randint(14, 71, n)
    near = k >= 1
    g[near, 2] = np.clip(g[near, 0] + rs.randint(-15, 16, near.sum()), 4, 74)
    g[near, 3] = np.clip(g[near, 1] + rs.randint(-5, 6, near.sum()), 14, 70)
    ropes = k == 2
    g[ropes, 0] = rs.choice([4, 5, 6, 72, 73, 74], ropes.sum())
    g[ropes, 2] = np.clip(g[ropes, 0] + rs.randint(-12, 13, ropes.sum()), 4, 74)
    g[ropes, 1] = rs.choice([14, 15, 69, 70], ropes.sum())
    g[ropes, 3] = np.clip(g[ropes, 1] + rs.randint(-4, 5, ropes.sum()), 14, 70)
    g[:, 4], g[:, 5] = rs.choice([0, 0, 0, 1, 2, 5, 8], n), rs.choice([0, 0, 0, 1, 2, 5, 8], n)
    g[:, 6], g[:, 7] = rs.randint(0, 100, n), rs.randint(0, 100, n)
    ko = k == 3
    g[ko, 6], g[ko, 7] = rs.randint(96, 102, ko.sum()), rs.randint(96, 102, ko.sum())
    g[:, 8] = rs.choice([0, 1, 500, 998, 999, 1678, 1679], n)
    g[:, 9] = rs.randint(0, 1 << 32, n, dtype=np.int64)
    return g.astype(np.uint32).view(np.int32).reshape(n, 16)


def crafted_rows(G, seed):
    """[G,16] int32 starting rows placed within reach of each other with scores 90..99, so that
    knock-backs and knock-outs occur within a few steps of random play."""
    rs = np.random.RandomState(seed)
    g = np.stack([row() for _ in range(G)]).astype(np.int64)
    g[:, 0], g[:, 1] = rs.randint(4, 75, G), rs.randint(14, 71, G)
    g[:, 2] = np.clip(g[:, 0] + rs.randint(-12, 13, G), 4, 74)
    g[:, 3] = np.clip(g[:, 1] + rs.randint(-4, 5, G), 14, 70)
    g[:, 6], g[:, 7] = rs.randint(90, 100, G), rs.randint(90, 100, G)
    g[:, 9] = 1000 * seed + np.arange(G)
    return g.astype(np.int32)


class Trajectory(object):
    """actions [S,2G], games [S+1,G,16] (games[0] the starting rows), reward [S,2G] float64,
    over [S,2G] bool, ep_score [S,2G] int32."""


@functools.lru_cache(maxsize=None)
def trajectory(G, steps, limit, seed):
    """Play from crafted_rows through duel.step_numpy: each player follows the chase-align-punch
    script on half of its steps (so punches keep landing after the boxers drift apart) and else
    plays a uniform random action, one in ten of those an out-of-range value."""
    from ba3c_amd import duel as D
    rs = np.random.RandomState(seed)
    game = crafted_rows(G, seed)
    tr = Trajectory()
    tr.actions = np.zeros((steps, 2 * G), np.int64)
    tr.games = np.zeros((steps + 1, G, 16), np.int32)
    tr.reward = np.zeros((steps, 2 * G), np.float64)
    tr.over = np.zeros((steps, 2 * G), bool)
    tr.ep_score = np.zeros((steps, 2 * G), np.int32)
    tr.games[0] = game
    odd = np.array(ODD_ACTIONS, np.int64)
    for s in range(steps):
        a = rs.randint(18, size=2 * G).astype(np.int64)
        a = np.where(rs.random_sample(2 * G) < 0.1, odd[rs.randint(len(odd), size=2 * G)], a)
        script = np.concatenate([chase_side_a(game), chase_side_b(game)])
        a = np.where(rs.random_sample(2 * G) < 0.5, script, a)
        tr.actions[s] = a
        tr.reward[s], tr.over[s], tr.ep_score[s] = D.step_numpy(game, a, limit)
        tr.games[s + 1] = game
    for v in (tr.actions, tr.games, tr.reward, tr.over, tr.ep_score):
        v.setflags(write=False)
    return tr


def chase_side_a(game):
    """The chase-align-punch script (boxing_policy.chase_actions) as side A of every row."""
    return chase_actions(game)


def chase_side_b(game):
    """The same script as side B: it plays the mirrored rows, in which it is side A."""
    from ba3c_amd import duel as D
    return chase_actions(D.mirror_rows(game))


# ---- sides for `match`: policy(state) -> probs, decided from the newest frame alone ---------
def _one_hot(actions, n=18):
    import torch
    p = torch.zeros(actions.shape[0], n, dtype=torch.float32, device=actions.device)
    p[torch.arange(actions.shape[0], device=actions.device), actions] = 1.0
    return p


def noop_policy(state):
    """Constant NOOP logits.  (Evaluation's PreventStuckPlayer turns the 30th NOOP in a row, and
    every one after it, into FIRE: this side stands still and punches whenever it can.)"""
    import torch
    return _one_hot(torch.zeros(state.shape[0], dtype=torch.int64, device=state.device))


def hit_and_run_policy(state):
    """A script that reads its own newest frame (itself: shade 255, the other boxer: 130).  It
    hovers 6 rows above the other boxer, just out of reach, within 9 px horizontally, and while
    the other boxer's arm shows (it punched at most 3 steps ago, so it cannot punch now) steps
    down into reach and punches.  Against a side that stands still and punches on a fixed beat
    it lands every punch and takes none."""
    import torch
    f = state[..., 3].to(torch.int64)[:, 13:79]                     # inside the ring: rows 13..78
    me, you = f == 255, f == 130
    rows_me, rows_you = me.any(2), you.any(2)
    ys = torch.arange(13, 79, device=state.device)
    big = torch.full_like(ys, 1000)
    ay = torch.where(rows_me, ys, big).min(1).values                # my top row: never hidden
    by = torch.where(rows_you, ys, -big).max(1).values - 7          # its bottom row: I am above it
    xs = torch.arange(84, device=state.device)
    big = torch.full_like(xs, 1000)
    ax = torch.where(me.sum(1) >= 8, xs, big).min(1).values         # body columns are 8 high,
    bx = torch.where(you.sum(1) >= 3, xs, big).min(1).values        # arm columns 2
    arm = you.sum(2).max(1).values >= 7                             # a row of body + arm is 10 wide
    dx = torch.where((bx - ax).abs() > 9, torch.sign(bx - ax), torch.zeros_like(ax))
    dy = torch.sign(torch.where(arm, by - 4, by - 6) - ay)
    # ALE's numbering: index [fire][dy + 1][dx + 1]
    table = torch.tensor([[[7, 2, 6], [4, 0, 3], [9, 5, 8]],
                          [[15, 10, 14], [12, 1, 11], [17, 13, 16]]], device=state.device)
    return _one_hot(table[arm.long(), dy + 1, dx + 1])
