"""Two-player GridBoxing: a second way to run GridBoxing (ba3c_amd.boxing) in which BOTH boxers
are driven by actions and each side receives its own observation, for self-play training
(`python -m ba3c_amd.train -e GridBoxing-v0 --self_play`) and policy-vs-policy matches
(`match`, `python -m ba3c_amd.duel`).  This module holds the rules ONCE: `step_numpy`,
`render_numpy` and `mirror_rows` (the oracle of the HIP kernel in csrc/ba3c_duel.h) over
GridBoxing's constants, and `BoxingDuelVec`, G games = 2G players on the device with
BoxingVec's interface (`BoxingDuelDecisionVec`: the same under frame skip, sticky actions and
drawn starts).

Row: GridBoxing's, `game[e] = [ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t, rng, 0, ...]`,
16 int32, side B in the scripted opponent's columns.  `rng` is carried unchanged: a step draws
nothing.  A fresh episode is GridBoxing's: (20, 42, 58, 42), the rest zero (or a drawn row, see
"Drawn starts" below, the only rule that draws from `rng`).

Players: G games have 2G players.  Player p = e is side A of game e, player p = G + e is side B
of game e; every per-player array (actions in; reward, over, ep_score, frame, state out) has 2G
rows in that order, so one predictor forward over state[2G] serves both sides.

Actions: each side picks one of ALE's 18 actions (boxing.py) in its OWN frame of reference, in
which it is the white boxer that starts on the left.  Side B's frame is the mirror x -> 78 - x
of the world: its RIGHT is the world's left, its dy is unchanged.  Out-of-range values are NOOP;
an action is range-checked and shifts the five masks, it never indexes memory.

step(a, b), in exactly this order:

    a_cd = max(a_cd - 1, 0); b_cd = max(b_cd - 1, 0)
    ax = clamp(ax + 2*dx_a, 4, 74); ay = clamp(ay + 2*dy_a, 14, 70)
    bx = clamp(bx - 2*dx_b, 4, 74); by = clamp(by + 2*dy_b, 14, 70)   # both sides move 2 px
    p = pts(); b_right = (bx >= ax)        # ONE judgement, on the positions after both moves
    pa = pb = 0
    if fire_a and a_cd == 0: a_cd = 8; pa = p
    if fire_b and b_cd == 0: b_cd = 8; pb = p
    a_score += pa; b_score += pb
    if pa: bx = clamp(bx + (3 if b_right else -3), 4, 74)
    if pb: ax = clamp(ax + (-3 if b_right else 3), 4, 74)
    t += 1
    over = a_score >= 100 or b_score >= 100 or t >= 1680 or t >= limit
    reward_A = pa - pb; reward_B = -reward_A; over is shared
    ep_score_A = a_score - b_score; ep_score_B = -ep_score_A       # written only where over
    if over: fresh episode (rng kept)

pts() is boxing._pts.

Mirror invariant: mirror_rows(g) = (78-bx, by, 78-ax, ay, b_cd, a_cd, b_score, a_score, t, rng,
0...) is an involution that maps the fresh row to itself, and the rules are exactly symmetric
under it: step(mirror(g), b, a) == mirror(step(g, a, b)) with rewards and ep_scores negated.
(pts() depends on |ax - bx| and |ay - by| only; bx >= ax is the same statement in both frames,
and every clamp range [4, 74] is its own image under x -> 78 - x.)  Neither side is favoured.

Observations: side A's frame is boxing.render_numpy(row), side B's is
boxing.render_numpy(mirror_rows(row)); there are no new render rules.  A step returns the frame
AFTER the step; on `over` that is the new episode's first frame, and both histories restart.

Drawn starts: a setting start = (h_lo, h_hi), 4 <= h_lo <= h_hi <= 19, is the range of the
HALF-gap between the boxers of a fresh episode.  (19, 19) is the fixed start above and draws
nothing: rng stays untouched.  Any other setting makes the fresh row from the row's own rng, which
no other rule of the duel reads or writes:

    rng = lcg(rng); r = rng >> 16
    h = h_lo + r % (h_hi - h_lo + 1);  y = 14 + 2 * ((r >> 8) % 29)
    row = (39 - h, y, 39 + h, y, 0, 0, 0, 0, 0, rng, 0...)

h >= 4 keeps the 6 px bodies apart; the boxers are within reach (gap 2h <= 14) iff h <= 7; y
runs over the even rows 14..70.  Users give the gap in pixels, 2h: even numbers 8..38, 38 being
the fixed start (`start_from_gap`).  Every drawn row is its own image under mirror_rows
(78 - (39 - h) = 39 + h, the y's are equal, the rest is zero), and rng is the same field on both
sides of the mirror, so step(mirror(g)) draws the same h and y as step(g) and lands on the same
self-mirrored row: the mirror invariant stays exact.  `initial_rows` applies the same draw to
initial_game's rows, so first episodes are drawn too.

One decision (`decide_numpy`): frame skip and sticky actions as ba3c_amd.frameskip states them,
per side.  aux[e] = [rng_k, rng_a, rng_b, prev_a, prev_b, 0, 0, 0], 8 int32: the skip's generator,
one generator per side for its sticky draws and each side's last effective action, all on
frameskip's LCG.  With parameters lo, hi, q16 (frameskip's ranges) and start, in this order:

    a, b = the two actions, each 0 (NOOP) unless in [0, 32)
    rng_k = lcg(rng_k); k = lo + ((rng_k >> 16) % (hi - lo + 1))
    R = 0
    for j in range(k):
        rng_a = lcg(rng_a); prev_a = prev_a if ((rng_a >> 8) & 0xFFFF) < q16 else a
        rng_b = lcg(rng_b); prev_b = prev_b if ((rng_b >> 8) & 0xFFFF) < q16 else b
        r, over, ep = step(prev_a, prev_b), whose fresh row is start's
        R += r
        if over: prev_a = prev_b = 0; break                # the remaining sub-steps are dropped
    reward_A = R; reward_B = -R; over and ep_score as the last executed step's

The frame (and the history push) is the one after the last executed sub-step.  `limit` counts
game steps.  With (1, 1, 0) and the fixed start a decision is exactly step.  The skip is shared,
so it has ONE generator; the sticky draws are per side, so each side has its own, and
`mirror_aux` (swap rng_a / rng_b and prev_a / prev_b, keep rng_k) extends the mirror invariant to
decisions: decide(mirror(g), mirror_aux(x), (b, a)) == mirror(decide(g, x, (a, b))), rewards and
ep_scores negated.  Had both sides drawn from one generator, the order of the two draws would
have told them apart.
"""
import numpy as np

from . import boxing, frameskip
from .boxing import (AX, AX0, AY, AY0, A_CD, A_SCORE, CLOCK, COOLDOWN, DEFAULT_LIMIT, DOWN_MASK, FIRE_MASK,
                     H, KNOCK, KO, LEFT_MASK, NOOP, NUM_ACTIONS, OX, OX0, OY, OY0, O_CD, O_SCORE, PALETTE,
                     RIGHT_MASK, RNG, T, UP_MASK, W, X_MAX, X_MIN, Y_MAX, Y_MIN, _clamp, _pts,
                     initial_game)
from .gamevec import GameVec

STEP = 2                                 # both sides move 2 px per step
MIRROR = 78                              # x -> 78 - x: body top-lefts 4..74 map onto themselves
BX, BY, B_CD, B_SCORE = OX, OY, O_CD, O_SCORE
CENTRE = 39                              # a drawn row is (39 - h, y, 39 + h, y): its own mirror image
H_MIN, H_MAX = 4, 19                     # half-gaps: bodies apart .. the fixed start
FIXED_START = (H_MAX, H_MAX)             # (20, 42, 58, 42), no draw
Y_DRAWS = 29                             # y = 14 + 2 * (0..28): the even rows 14..70
AUX_INTS = 8
RNG_K, RNG_A, RNG_B, PREV_A, PREV_B = range(5)


def mirror_rows(game):
    """The rows as side B sees them: x -> 78 - x and the two sides exchanged ([..., 16] int32)."""
    g = np.asarray(game)
    m = np.zeros_like(g)
    m[..., AX], m[..., AY], m[..., BX], m[..., BY] = MIRROR - g[..., BX], g[..., BY], MIRROR - g[..., AX], g[..., AY]
    m[..., A_CD], m[..., B_CD], m[..., A_SCORE], m[..., B_SCORE] = (g[..., B_CD], g[..., A_CD], g[..., B_SCORE],
                                                                   g[..., A_SCORE])
    m[..., T], m[..., RNG] = g[..., T], g[..., RNG]
    return m


def _decode(a):
    """(dx, dy, fire) of int64 actions in their side's own frame; out of range: NOOP."""
    sh = np.where((a >= 0) & (a < NUM_ACTIONS), a, NOOP)
    up, down, right, left, fire = (((m >> sh) & 1) for m in
                                   (UP_MASK, DOWN_MASK, RIGHT_MASK, LEFT_MASK, FIRE_MASK))
    return right - left, down - up, fire == 1


def check_start(start):
    """(h_lo, h_hi) of a `start=` argument (None: the fixed start), checked; raises ValueError."""
    if start is None:
        return FIXED_START
    if not isinstance(start, (tuple, list)) or len(start) != 2:
        raise ValueError("start %r: expected (h_lo, h_hi)" % (start,))
    lo, hi = int(start[0]), int(start[1])
    if not H_MIN <= lo <= hi <= H_MAX:
        raise ValueError("start half-gap %r-%r: needs %d <= lo <= hi <= %d" % (lo, hi, H_MIN, H_MAX))
    return lo, hi


def parse_gap(s):
    """A string "GAP" / "LO-HI" (pixels) -> (lo, hi), inclusive; the range is start_from_gap's."""
    parts = [int(p) for p in str(s).split("-")]                # "-8", "a": ValueError
    if len(parts) not in (1, 2):
        raise ValueError("start gap %r: expected GAP or LO-HI" % (s,))
    return parts[0], parts[-1]


def start_from_gap(gap):
    """The user-facing unit -> `start=`: a gap in pixels (an int, a (lo, hi) pair or a string
    "GAP" / "LO-HI"; even numbers 8..38) -> (h_lo, h_hi), or None for 38, the fixed start."""
    if isinstance(gap, str):
        gap = parse_gap(gap)
    if not isinstance(gap, (tuple, list)):
        gap = (gap, gap)
    lo, hi = int(gap[0]), int(gap[-1])
    if len(gap) != 2 or lo % 2 or hi % 2 or not 2 * H_MIN <= lo <= hi <= 2 * H_MAX:
        raise ValueError("start gap %r: needs even pixels with %d <= lo <= hi <= %d"
                         % (gap, 2 * H_MIN, 2 * H_MAX))
    return None if (lo, hi) == (2 * H_MAX, 2 * H_MAX) else (lo // 2, hi // 2)


def draw_start(rng, start):
    """The draw of a fresh row: rng (int64 array of uint32 values) -> (rng', h, y)."""
    lo, hi = start
    rng = frameskip.lcg(rng)
    r = rng >> 16
    return rng, lo + r % (hi - lo + 1), Y_MIN + 2 * ((r >> 8) % Y_DRAWS)


def initial_rows(n_games, seed=0, start=None):
    """[G,16] int32 rows of fresh games: boxing.initial_game's, and under a drawn start the
    first episodes' rows are drawn as every later one's."""
    game = initial_game(n_games, seed)
    start = check_start(start)
    if start != FIXED_START:
        rng, h, y = draw_start(game[:, RNG].astype(np.int64) & 0xFFFFFFFF, start)
        game[:, AX], game[:, AY], game[:, BX], game[:, BY] = CENTRE - h, y, CENTRE + h, y
        game[:, RNG] = rng.astype(np.uint32).view(np.int32)
    return game


def initial_aux(n_games, seed=0):
    """[G,8] int32 aux rows of fresh games: three of frameskip's generators, prev = NOOP."""
    G = int(n_games)
    aux = np.zeros((G, AUX_INTS), np.int32)
    e = np.arange(G, dtype=np.int64)
    for col, first in ((RNG_A, 0), (RNG_B, G), (RNG_K, 2 * G)):
        v = ((np.int64(seed) * 1000 + first + e) ^ frameskip.SEED_XOR) & 0xFFFFFFFF
        aux[:, col] = v.astype(np.uint32).view(np.int32)
    return aux


def mirror_aux(aux):
    """The aux rows as side B holds them: the sides' generators and prevs exchanged."""
    x = np.asarray(aux)
    m = np.zeros_like(x)
    m[..., RNG_K], m[..., RNG_A], m[..., RNG_B] = x[..., RNG_K], x[..., RNG_B], x[..., RNG_A]
    m[..., PREV_A], m[..., PREV_B] = x[..., PREV_B], x[..., PREV_A]
    return m


def step_numpy(game, actions, limit=DEFAULT_LIMIT, start=None):
    """One step of every row of `game` ([G,16] int32, updated in place) under `actions` [2G]
    (player order); start: the fresh rows' (h_lo, h_hi), None for the fixed start.  Returns
    (reward float64 [2G], over bool [2G], ep_score int32 [2G], 0 where not over)."""
    start = check_start(start)
    G = game.shape[0]
    act = np.asarray(actions).astype(np.int64).reshape(2 * G)
    g = game.astype(np.int64)
    ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t = (g[:, i].copy() for i in range(9))
    dx_a, dy_a, fire_a = _decode(act[:G])
    dx_b, dy_b, fire_b = _decode(act[G:])

    a_cd = np.maximum(a_cd - 1, 0)
    b_cd = np.maximum(b_cd - 1, 0)
    ax = _clamp(ax + STEP * dx_a, X_MIN, X_MAX)
    ay = _clamp(ay + STEP * dy_a, Y_MIN, Y_MAX)
    bx = _clamp(bx - STEP * dx_b, X_MIN, X_MAX)            # B's RIGHT is the world's left
    by = _clamp(by + STEP * dy_b, Y_MIN, Y_MAX)
    p = _pts(ax, ay, bx, by)                               # ONE judgement, after both moves
    b_right = bx >= ax
    punch_a = fire_a & (a_cd == 0)
    punch_b = fire_b & (b_cd == 0)
    a_cd = np.where(punch_a, COOLDOWN, a_cd)
    b_cd = np.where(punch_b, COOLDOWN, b_cd)
    pa = np.where(punch_a, p, 0)
    pb = np.where(punch_b, p, 0)
    a_score = a_score + pa
    b_score = b_score + pb
    bx = np.where(pa > 0, _clamp(bx + np.where(b_right, KNOCK, -KNOCK), X_MIN, X_MAX), bx)
    ax = np.where(pb > 0, _clamp(ax + np.where(b_right, -KNOCK, KNOCK), X_MIN, X_MAX), ax)
    t = t + 1
    over = (a_score >= KO) | (b_score >= KO) | (t >= CLOCK) | (t >= int(limit))
    ep = np.where(over, a_score - b_score, 0)

    fresh = (AX0, AY0, OX0, OY0, 0, 0, 0, 0, 0)
    if start != FIXED_START:                               # the only draw from the row's rng
        rng = g[:, RNG] & 0xFFFFFFFF
        drawn, h, y = draw_start(rng, start)
        fresh = (CENTRE - h, y, CENTRE + h, y, 0, 0, 0, 0, 0)
        game[:, RNG] = np.where(over, drawn, rng).astype(np.uint32).view(np.int32)
    cols = (ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t)
    for i, (v, f) in enumerate(zip(cols, fresh)):
        game[:, i] = np.where(over, f, v).astype(np.int32)
    game[:, RNG + 1:] = 0                                  # rng (column 9) is otherwise carried unchanged
    reward = (pa - pb).astype(np.float64)
    return (np.concatenate([reward, -reward]), np.concatenate([over, over]),
            np.concatenate([ep, -ep]).astype(np.int32))


def decide_numpy(game, aux, actions, limit=DEFAULT_LIMIT, lo=1, hi=1, q16=0, start=None):
    """One decision of every row of `game` ([G,16] int32) and `aux` ([G,8] int32), both updated
    in place, under `actions` [2G] (player order).  Returns step_numpy's triple: the rewards are
    summed over the executed sub-steps."""
    frameskip.check(lo, hi, q16)
    start = check_start(start)
    G = game.shape[0]
    act = np.asarray(actions).astype(np.int64).reshape(2 * G)
    act = np.where((act >= 0) & (act < frameskip.ACTION_BOUND), act, 0)
    chosen = (act[:G], act[G:])
    rng_k = frameskip.lcg(aux[:, RNG_K].astype(np.int64) & 0xFFFFFFFF)
    k = lo + ((rng_k >> 16) % (hi - lo + 1))
    rng = [aux[:, c].astype(np.int64) & 0xFFFFFFFF for c in (RNG_A, RNG_B)]
    prev = [aux[:, c].astype(np.int64) for c in (PREV_A, PREV_B)]
    R = np.zeros(G, np.float64)
    over = np.zeros(G, bool)
    ep_score = np.zeros(G, np.int64)
    for j in range(hi):
        live = (j < k) & ~over
        if not live.any():
            break
        eff = [None, None]
        for s in range(2):                                 # each side draws from its own generator
            rng[s] = np.where(live, frameskip.lcg(rng[s]), rng[s])
            eff[s] = np.where(((rng[s] >> 8) & 0xFFFF) < q16, prev[s], chosen[s])
        kept = game.copy()
        r, o, ep = step_numpy(game, np.concatenate(eff), limit, start)
        game[~live] = kept[~live]         # k exhausted or episode ended: that row did not step
        ended = live & o[:G]
        R += np.where(live, r[:G], 0.0)
        over |= ended
        ep_score = np.where(ended, ep[:G], ep_score)
        for s in range(2):
            prev[s] = np.where(ended, 0, np.where(live, eff[s], prev[s]))
    aux[:] = 0
    for c, v in ((RNG_K, rng_k), (RNG_A, rng[0]), (RNG_B, rng[1])):
        aux[:, c] = v.astype(np.uint32).view(np.int32)
    aux[:, PREV_A], aux[:, PREV_B] = prev[0].astype(np.int32), prev[1].astype(np.int32)
    return (np.concatenate([R, -R]), np.concatenate([over, over]),
            np.concatenate([ep_score, -ep_score]).astype(np.int32))


def render_numpy(game):
    """[2G,84,84] uint8 frames in player order: side A's frames of the rows, then side B's (the
    frames of the mirrored rows)."""
    return np.concatenate([boxing.render_numpy(game), boxing.render_numpy(mirror_rows(game))])


class BoxingDuelVec(GameVec):
    """G two-player GridBoxing games in HBM: E = 2G players with BoxingVec's interface
    (ba3c_amd.gamevec.GameVec), all over the E players in player order; `game` is [G,16].  Every
    step is one HIP launch (ba3c_boxing_duel_step).  No frame skip, no sticky actions, the fixed
    start: those are BoxingDuelDecisionVec's."""

    A = NUM_ACTIONS
    PALETTE = PALETTE
    PLAYERS, COUNT = 2, "n_games"
    STEP, DECIDE = "ba3c_boxing_duel_step", "ba3c_boxing_duel_decide"
    RENDER, VIEW = "ba3c_boxing_duel_render", "ba3c_boxing_view"
    initial_aux = staticmethod(initial_aux)

    def __init__(self, n_games, seed=0, limit=DEFAULT_LIMIT, device="cuda"):
        self._counts(n_games, limit)
        self._alloc(seed, device)

    def initial_game(self, n_games, seed):
        return initial_rows(n_games, seed, self.start)

    def mirrored_game(self):
        """mirror_rows of `game` as a new tensor on the device (a few tensor ops)."""
        m = self.game[:, [BX, BY, AX, AY, B_CD, A_CD, B_SCORE, A_SCORE] + list(range(T, 16))]
        m[:, AX] = MIRROR - m[:, AX]
        m[:, BX] = MIRROR - m[:, BX]
        m[:, RNG + 1:] = 0
        return m.contiguous()

    def view(self, scale=1, sel=None, hud=None, side="a"):
        """The colour view of the current GAMES, the world as side A sees it
        (ba3c_amd.view.view_numpy of the rows with GridBoxing's palette): torch.uint8
        [n, Hc*scale, 84*scale, 3] through ba3c_boxing_view; sel: game indices (None: all G).
        side="b": the world as side B sees it, the same view of the mirrored rows."""
        if side not in ("a", "b"):
            raise ValueError("side must be 'a' or 'b'")
        return GameVec.view(self, scale, sel, hud, self.mirrored_game() if side == "b" else None)


class BoxingDuelDecisionVec(BoxingDuelVec):
    """BoxingDuelVec whose step is one DECISION of `decide_numpy`: `frame_skip` / `sticky`
    (ba3c_amd.frameskip's arguments, per side) and `start`, a drawn start's (h_lo, h_hi).  One
    HIP launch per decision (ba3c_boxing_duel_decide), aux rows [G,8] in `aux`, the setting in
    `skip` (lo, hi, q16) and `start`.  With the defaults it is a BoxingDuelVec: no `aux`, the
    same rows, the same entry points, as BoxingVec is under ba3c_amd.frameskip."""

    def __init__(self, n_games, seed=0, limit=DEFAULT_LIMIT, device="cuda", frame_skip=1, sticky=0.0,
                 start=None):
        skip = frameskip.setting(frame_skip, sticky)
        start = check_start(start)
        if skip is not None or start != FIXED_START:
            self.skip, self.start = skip or (1, 1, 0), start
        BoxingDuelVec.__init__(self, n_games, seed, limit, device)


class _PolicySide(object):
    """What evaluate.EvalPlayers asks of an engine, for a side that is a bare policy callable."""

    num_actions = NUM_ACTIONS

    def __init__(self, device):
        import torch

        from .engine import greedy
        self.device = torch.device(device)
        self.greedy = greedy


def _play(side_a, side_b, n_games, episodes, seed, limit, device, frame_skip, sticky, start, watch=None):
    """The decision path `match` and `record_match` share.  watch (None for a match) is told of
    the env before the first decision (`begin(env)`), of every decision while the env still holds
    the rows it was made for (`decided(env, outs)`, outs = each side's (probs, value, act)) and
    of every step (`stepped(env, reward, over_h)`, side A's halves on the host).  -> scores."""
    import torch

    from .evaluate import EvalPlayers
    from .rollout import FrameHistory
    G = int(n_games)
    assert G >= 1 and episodes >= 1
    engines = [s for s in (side_a, side_b) if not callable(s)]
    if device is None:
        device = engines[0].device if engines else "cuda"
    players = []
    for i, side in enumerate((side_a, side_b)):
        rs = np.random.RandomState([int(seed), i])
        if callable(side):
            players.append(EvalPlayers(_PolicySide(device), G, rs, side))
        else:
            assert G <= side.max_batch and side.num_actions >= NUM_ACTIONS
            players.append(EvalPlayers(side, G, rs))
    env = BoxingDuelDecisionVec(G, seed=seed, limit=limit, device=device, frame_skip=frame_skip,
                                sticky=sticky, start=start)
    hist = FrameHistory(env.E, hist_len=4, channels=1, device=env.device)
    env.reset_history(hist)
    if watch is not None:
        watch.begin(env)
    scores = []
    while len(scores) < episodes:
        outs = [p.decide(s) for p, s in zip(players, (hist.state[:G], hist.state[G:]))]
        if watch is not None:
            watch.decided(env, outs)
        reward, over = env.step_into(torch.cat([o[2] for o in outs]), hist)
        players[0].ended(over[:G])
        players[1].ended(over[G:])
        over_h = over[:G].cpu().numpy()
        if watch is not None:
            watch.stepped(env, reward[:G].cpu().numpy(), over_h)
        if over_h.any():
            scores += env.ep_score[:G].cpu().numpy()[over_h].tolist()
    return scores


def match(side_a, side_b, n_games, episodes, seed=0, limit=DEFAULT_LIMIT, device=None, frame_skip=1,
          sticky=0.0, start=None):
    """Play side_a (side A of every game) against side_b on `n_games` games until `episodes`
    games have finished; those finishing in the same step as the last one are counted too (as
    eval_with_envs counts them).  A side is an engine or a policy(state) -> probs [G, A]
    callable; each decides from its own half of the stacked state along evaluation's path
    (greedy, eps = 0.001, PreventStuckPlayer(30, 1) per player, counting chosen actions, one per
    decision) with its own RandomState derived from `seed`.  frame_skip / sticky / start:
    BoxingDuelDecisionVec's.  Returns a dict: episodes, wins / draws / losses of side A (the sign of its
    ep_score), mean_score / max_score of side A's ep_score, and scores, one per episode in the
    order they finished."""
    return match_result(_play(side_a, side_b, n_games, episodes, seed, limit, device, frame_skip, sticky,
                              start))


def match_result(scores):
    """`match`'s dict of side A's episode scores."""
    s = np.array(scores, np.int64)
    return {"episodes": len(scores), "wins": int((s > 0).sum()), "draws": int((s == 0).sum()),
            "losses": int((s < 0).sum()), "mean_score": float(s.mean()), "max_score": int(s.max()),
            "scores": [int(v) for v in scores]}


def main(argv=None):
    import copy
    import json

    from .flags import GRID_BOXING, build_parser, resolve
    p = build_parser()
    p.description = ("a match of two policies on two-player GridBoxing: --load plays side A, "
                     "--load_b (or --random_b) side B; both networks share the model flags")
    p.set_defaults(environment=GRID_BOXING, num_actions=NUM_ACTIONS)
    p.add_argument("--load_b", default=None, help="side B's checkpoint")
    p.add_argument("--random_b", action="store_true", help="side B plays uniform-random actions")
    p.add_argument("--episodes", type=int, default=100)
    p.add_argument("--games", type=int, default=20, help="games played at once")
    p.add_argument("--limit", type=int, default=DEFAULT_LIMIT, help="LimitLengthPlayer's game steps")
    p.add_argument("--record", default=None, metavar="DIR",
                   help="record the match (ba3c_amd.record.record_match): one .npz (and .gif) per "
                        "episode in DIR")
    p.add_argument("--scale", type=int, default=3, help="--record: pixel scale of the frames, 1..8")
    p.add_argument("--every", type=int, default=1, help="--record: keep every N-th decision's frame")
    p.add_argument("--max_frames", type=int, default=2000, help="--record: frames kept per episode")
    p.add_argument("--side", default="a", choices=["a", "b"],
                   help="--record: whose view and whose policy output the frames show")
    args = resolve(p.parse_args(argv), duel_tool=True)
    if args.environment != GRID_BOXING or args.self_play:
        raise SystemExit("a match is played on -e %s, without --self_play" % GRID_BOXING)
    if not 1 <= args.scale <= 8 or args.every < 1 or args.max_frames < 0:
        raise SystemExit("--scale must be in [1, 8], --every >= 1 and --max_frames >= 0")
    if bool(args.load_b) == bool(args.random_b):
        raise SystemExit("pass side B: exactly one of --load_b CHECKPOINT and --random_b")
    if args.episodes < 1 or args.games < 1:
        raise SystemExit("--episodes and --games must be >= 1")
    from .evaluate import uniform_policy
    from .train import build
    args.simulator_procs = max(args.simulator_procs, args.games)       # the engines' max_batch
    side_a = build(args)[0].engine
    if args.random_b:
        side_b = uniform_policy(args.num_actions)
    else:
        args_b = copy.copy(args)
        args_b.load = args.load_b
        side_b = build(args_b)[0].engine
    how = dict(seed=0 if args.seed is None else args.seed, limit=args.limit, frame_skip=args.frame_skip,
               sticky=args.sticky, start=start_from_gap(args.duel_start))
    if args.record:
        import os

        from .record import record_match
        traces = record_match(side_a, side_b, args.episodes, args.games, scale=args.scale, every=args.every,
                              max_frames=args.max_frames, side=args.side, **how)
        out = match_result([t.score for t in traces])
        out["files"] = []
        for i, t in enumerate(traces):
            out["files"] += t.save(os.path.join(args.record, "match_%03d" % i))
    else:
        out = match(side_a, side_b, args.games, args.episodes, **how)
    out = dict(side_a=args.load, side_b=args.load_b or "random", games=args.games, **out)
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
