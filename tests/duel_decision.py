"""Shared pieces of the tests of two-player GridBoxing's DECISIONS (frame skip, sticky actions per
side, drawn starts): a scalar restatement of duel.py's written rules in plain Python ints over
duel_policy.step_scalar, the settings every test crosses, and one cached CPU trajectory per case
that also reports what it covered."""
import functools

import numpy as np

from duel_policy import ODD_ACTIONS, chase_side_a, chase_side_b, crafted_rows, step_scalar

M32 = 0xFFFFFFFF
SKIPS = ((1, 1, 0), (4, 4, 0), (2, 4, 16384), (1, 16, 58982))
STARTS = (None, (4, 7), (4, 19))             # None: the fixed start, which is also (19, 19)


def lcg(x):
    return (x * 1664525 + 1013904223) & M32


def signed(x):
    return x - (1 << 32) if x >= (1 << 31) else x


def draw_scalar(rng, start):
    """The written draw of a fresh row: rng (an unsigned int) -> (the row's first ten fields)."""
    lo, hi = start
    rng = lcg(rng)
    r = rng >> 16
    h = lo + r % (hi - lo + 1)
    y = 14 + 2 * ((r >> 8) % 29)
    return [39 - h, y, 39 + h, y, 0, 0, 0, 0, 0, signed(rng)]


def decide_scalar(row, aux, a, b, limit, lo, hi, q16, start):
    """One decision of one game (row: 16 ints, aux: 8 ints) as duel.py's docstring writes it.
    -> (new row, new aux, reward_A, over, ep_score_A or 0, executed sub-steps, k)."""
    row = [int(v) for v in row]
    rng_k, rng_a, rng_b = (int(v) & M32 for v in aux[:3])
    prev_a, prev_b = int(aux[3]), int(aux[4])
    a = a if 0 <= a < 32 else 0
    b = b if 0 <= b < 32 else 0
    rng_k = lcg(rng_k)
    k = lo + ((rng_k >> 16) % (hi - lo + 1))
    R, over, ep, n = 0, False, 0, 0
    for _ in range(k):
        rng_a = lcg(rng_a)
        prev_a = prev_a if ((rng_a >> 8) & 0xFFFF) < q16 else a
        rng_b = lcg(rng_b)
        prev_b = prev_b if ((rng_b >> 8) & 0xFFFF) < q16 else b
        row, r, over, ep = step_scalar(row, prev_a, prev_b, limit)
        R += r
        n += 1
        if over:
            if start is not None and tuple(start) != (19, 19):
                row = draw_scalar(row[9] & M32, start) + [0] * 6
            prev_a = prev_b = 0
            break
    return row, [signed(rng_k), signed(rng_a), signed(rng_b), prev_a, prev_b, 0, 0, 0], R, over, ep, n, k


def executed(aux_before, aux_after, col=1):
    """The sub-steps each game executed in a decision: how far side A's generator moved."""
    x = aux_before[:, col].astype(np.int64) & M32
    want = aux_after[:, col].astype(np.int64) & M32
    n = np.full(x.shape[0], -1, np.int64)
    for j in range(17):
        n = np.where((n < 0) & (x == want), j, n)
        x = (x * 1664525 + 1013904223) & M32
    assert (n >= 0).all()
    return n


class Trajectory(object):
    """actions [S,2G], games [S+1,G,16], auxs [S+1,G,8], reward [S,2G] float64, over [S,2G] bool,
    ep_score [S,2G] int32, n_exec [S,G] and k [S,G] (executed sub-steps, drawn skip)."""


@functools.lru_cache(maxsize=None)
def trajectory(G, steps, limit, seed, skip, start):
    """Play from crafted_rows through duel.decide_numpy as duel_policy.trajectory plays steps:
    each player follows the chase-align-punch script on half of its decisions and else plays a
    uniform random action, one in ten of those an out-of-range value."""
    from ba3c_amd import duel as D
    rs = np.random.RandomState(seed)
    game, aux = crafted_rows(G, seed), D.initial_aux(G, seed)
    tr = Trajectory()
    tr.actions = np.zeros((steps, 2 * G), np.int64)
    tr.games = np.zeros((steps + 1, G, 16), np.int32)
    tr.auxs = np.zeros((steps + 1, G, 8), np.int32)
    tr.reward = np.zeros((steps, 2 * G), np.float64)
    tr.over = np.zeros((steps, 2 * G), bool)
    tr.ep_score = np.zeros((steps, 2 * G), np.int32)
    tr.n_exec = np.zeros((steps, G), np.int64)
    tr.k = np.zeros((steps, G), np.int64)
    tr.games[0], tr.auxs[0] = game, aux
    odd = np.array(ODD_ACTIONS, np.int64)
    lo, hi, q16 = skip
    for s in range(steps):
        a = rs.randint(18, size=2 * G).astype(np.int64)
        a = np.where(rs.random_sample(2 * G) < 0.1, odd[rs.randint(len(odd), size=2 * G)], a)
        script = np.concatenate([chase_side_a(game), chase_side_b(game)])
        a = np.where(rs.random_sample(2 * G) < 0.5, script, a)
        tr.actions[s] = a
        tr.reward[s], tr.over[s], tr.ep_score[s] = D.decide_numpy(game, aux, a, limit, lo, hi, q16, start)
        tr.games[s + 1], tr.auxs[s + 1] = game, aux
        tr.n_exec[s] = executed(tr.auxs[s], tr.auxs[s + 1])
        rng_k = (tr.auxs[s + 1][:, 0].astype(np.int64) & M32)
        tr.k[s] = lo + (rng_k >> 16) % (hi - lo + 1)
    for v in (tr.actions, tr.games, tr.auxs, tr.reward, tr.over, tr.ep_score, tr.n_exec, tr.k):
        v.setflags(write=False)
    return tr


def one_sided_repeats(tr, q16):
    """The number of executed sub-steps in which exactly one side's sticky draw repeated."""
    count = 0
    S, G = tr.n_exec.shape
    for s in range(S):
        xa = tr.auxs[s][:, 1].astype(np.int64) & M32
        xb = tr.auxs[s][:, 2].astype(np.int64) & M32
        for j in range(int(tr.n_exec[s].max())):
            xa, xb = (xa * 1664525 + 1013904223) & M32, (xb * 1664525 + 1013904223) & M32
            live = j < tr.n_exec[s]
            count += int((live & ((((xa >> 8) & 0xFFFF) < q16) != (((xb >> 8) & 0xFFFF) < q16))).sum())
    return count


def assert_covered(tr, G, limit, skip, start):
    """What a GPU comparison over `tr` stands on: a landed punch for each side, a knock-out, an
    episode end inside a skip, an out-of-range action, a sticky repeat on one side only, and (a
    drawn start, G > 1) at least two distinct drawn rows in every game -- each where the setting
    can produce it."""
    lo, hi, q16 = skip
    over = tr.over[:, :G]
    t_end = tr.games[:-1, :, 8] + tr.n_exec
    assert over.any() and (tr.n_exec >= 1).all() and (tr.n_exec <= tr.k).all()
    assert (tr.n_exec[~over] == tr.k[~over]).all()
    if G > 1:
        assert (tr.reward[:, :G] > 0).any() and (tr.reward[:, :G] < 0).any()
        assert (over & (t_end < limit)).any()                           # a knock-out
        assert np.isin(tr.actions, ODD_ACTIONS).any()
        if hi > 1:
            assert (over & (tr.n_exec < tr.k)).any()                    # the rest of the skip dropped
        if 0 < q16 < 65536:
            assert one_sided_repeats(tr, q16) > 0
    if start is not None and tuple(start) != (19, 19):
        for e in range(G):
            drawn = tr.games[1:, e][over[:, e]]
            assert G == 1 or len({tuple(r[:4]) for r in drawn.tolist()}) >= 2, e
            assert (drawn[:, 9] != tr.games[:-1, e, 9][over[:, e]]).all()
    else:
        assert (tr.games[:, :, 9] == tr.games[0, :, 9]).all()           # the fixed start draws nothing
