"""Frame skip and sticky actions for the on-device games (GridBreakout, GridBoxing): what one
policy DECISION does to a simulator.  ALE's `-v0` ids run each chosen action for a number of
frames drawn per decision and, with some probability per frame, repeat the previous frame's
action instead of the chosen one ("sticky" actions); this module states that ONCE, over the
games' own `step_numpy`, and is the oracle of the HIP kernel (csrc/ba3c_envkernel.h:
sim_kernel<SoloSim<Rules>, true>, behind ba3c_breakout_step_skip / ba3c_boxing_step_skip) and of
`ba3c_amd.envs.FrameSkipPlayer`.  It restates no rule of either game.

The 16-int game rows are full and their layout is public, so a decision keeps its own state in
a per-simulator auxiliary row `aux[e] = [rng2, prev]`, two int32:

    rng2 = ((seed*1000 + e) ^ 0x9E3779B9) mod 2^32     the decision's own generator
    prev = 0                                           the last effective action (NOOP)

`lcg` is the games' LCG (1664525, 1013904223) on a stream of its own: the row's `rng` (the serve
sequence, the opponent) is drawn exactly as without frame skip.

One decision with parameters lo, hi, q16 (1 <= lo <= hi <= 16, 0 <= q16 <= 65536; q16 = 65536:
every sub-step is sticky), in exactly this order:

    a    = action[e] if 0 <= action[e] < 32 else 0     # out of range: NOOP, before it can be
    rng2 = lcg(rng2);  k = lo + ((rng2 >> 16) % (hi - lo + 1))               # remembered
    R = 0; over = False
    for j in range(k):
        rng2 = lcg(rng2)
        eff  = prev if ((rng2 >> 8) & 0xFFFF) < q16 else a
        prev = eff
        r, o, ep = game.step(row, eff, limit)          # the game's own step, unchanged
        R += r
        if o: over = True; ep_score = ep; prev = 0; break      # the row has auto-reset: the
    reward = float64(R)                                        # remaining sub-steps are dropped

The frame (and the history push) of a decision is the frame after the last executed sub-step;
on `over` that is the new episode's first frame and the history is cleared, as for a plain step.
`limit` keeps counting GAME STEPS (the row's `t`): under frame skip it no longer counts
decisions.  Rendering stays the game's `render_numpy`.
"""
import numpy as np

LCG_A, LCG_C = 1664525, 1013904223
AUX_INTS = 2
RNG2, PREV = range(2)
SEED_XOR = 0x9E3779B9
MAX_SKIP = 16
ACTION_BOUND = 32            # actions outside [0, 32) are NOOP before they can be remembered
Q16_ONE = 1 << 16


def lcg(x):
    return (x * LCG_A + LCG_C) & 0xFFFFFFFF


def initial_rng2(seed, e):
    """The start of simulator e's decision generator (Python int in [0, 2^32))."""
    return ((int(seed) * 1000 + int(e)) ^ SEED_XOR) & 0xFFFFFFFF


def initial_aux(n_envs, seed=0):
    """[E,2] int32 aux rows of fresh simulators."""
    aux = np.zeros((int(n_envs), AUX_INTS), np.int32)
    rng2 = ((np.int64(seed) * 1000 + np.arange(n_envs, dtype=np.int64)) ^ SEED_XOR) & 0xFFFFFFFF
    aux[:, RNG2] = rng2.astype(np.uint32).view(np.int32)
    return aux


def check(lo, hi, q16):
    """The parameter ranges every layer holds; raises ValueError."""
    if not 1 <= lo <= hi <= MAX_SKIP:
        raise ValueError("frame skip %r-%r: needs 1 <= lo <= hi <= %d" % (lo, hi, MAX_SKIP))
    if not 0 <= q16 <= Q16_ONE:
        raise ValueError("sticky probability must be in [0, 1]")


def parse_skip(frame_skip):
    """An int K, a (lo, hi) pair or a string "K" / "LO-HI" -> (lo, hi), inclusive."""
    if isinstance(frame_skip, str):
        frame_skip = [int(p) for p in frame_skip.split("-")]      # "-3", "a": ValueError
    if not isinstance(frame_skip, (tuple, list)):
        frame_skip = [frame_skip]
    if len(frame_skip) not in (1, 2):
        raise ValueError("frame skip %r: expected K or LO-HI" % (frame_skip,))
    return int(frame_skip[0]), int(frame_skip[-1])


def setting(frame_skip=1, sticky=0.0):
    """(lo, hi, q16) of a vector's or a player's `frame_skip=` / `sticky=` arguments, checked;
    None for the defaults, which are the plain one-step path."""
    lo, hi = parse_skip(frame_skip)
    if not 0.0 <= float(sticky) <= 1.0:
        raise ValueError("sticky probability must be in [0, 1]")
    q16 = int(round(float(sticky) * Q16_ONE))
    check(lo, hi, q16)
    return None if (lo, hi, q16) == (1, 1, 0) else (lo, hi, q16)


def step_numpy(game_module, game, aux, actions, limit, lo, hi, q16):
    """One decision of every row of `game` ([E,16] int32) and `aux` ([E,2] int32), both updated
    in place, under `actions` [E]; game_module is ba3c_amd.breakout or ba3c_amd.boxing.
    Returns (reward float64 [E], over bool [E], ep_score int32 [E], 0 where not over)."""
    check(lo, hi, q16)
    E = game.shape[0]
    a = np.asarray(actions).astype(np.int64).reshape(E)
    a = np.where((a >= 0) & (a < ACTION_BOUND), a, 0)
    rng2 = aux[:, RNG2].astype(np.int64) & 0xFFFFFFFF
    prev = aux[:, PREV].astype(np.int64)
    rng2 = lcg(rng2)
    k = lo + ((rng2 >> 16) % (hi - lo + 1))
    R = np.zeros(E, np.float64)
    over = np.zeros(E, bool)
    ep_score = np.zeros(E, np.int32)
    for j in range(hi):
        live = (j < k) & ~over
        if not live.any():
            break
        rng2 = np.where(live, lcg(rng2), rng2)
        eff = np.where(((rng2 >> 8) & 0xFFFF) < q16, prev, a)
        kept = game.copy()
        r, o, ep = game_module.step_numpy(game, eff, limit)
        game[~live] = kept[~live]         # k exhausted or episode ended: that row did not step
        ended = live & o
        R += np.where(live, r, 0.0)
        over |= ended
        ep_score = np.where(ended, ep, ep_score).astype(np.int32)
        prev = np.where(ended, 0, np.where(live, eff, prev))
    aux[:, RNG2] = rng2.astype(np.uint32).view(np.int32)
    aux[:, PREV] = prev.astype(np.int32)
    return R, over, ep_score
