"""Two-player GridBoxing: a second way to run GridBoxing (ba3c_amd.boxing) in which BOTH boxers
are driven by actions and each side receives its own observation, for self-play training
(`python -m ba3c_amd.train -e GridBoxing-v0 --self_play`) and policy-vs-policy matches
(`match`, `python -m ba3c_amd.duel`).  This module holds the rules ONCE: `step_numpy`,
`render_numpy` and `mirror_rows` (the oracle of the HIP kernel in csrc/ba3c_duel.h) over
GridBoxing's constants, and `BoxingDuelVec`, G games = 2G players on the device with
BoxingVec's interface.

Row: GridBoxing's, `game[e] = [ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t, rng, 0, ...]`,
16 int32, side B in the scripted opponent's columns.  `rng` is carried unchanged: the duel draws
nothing.  A fresh episode is GridBoxing's: (20, 42, 58, 42), the rest zero.

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
"""
import ctypes

import numpy as np

from . import boxing
from .boxing import (AX, AX0, AY, AY0, A_CD, A_SCORE, CLOCK, COOLDOWN, DEFAULT_LIMIT, DOWN_MASK, FIRE_MASK,
                     H, KNOCK, KO, LEFT_MASK, NOOP, NUM_ACTIONS, OX, OX0, OY, OY0, O_CD, O_SCORE, PALETTE,
                     RIGHT_MASK, RNG, T, UP_MASK, W, X_MAX, X_MIN, Y_MAX, Y_MIN, _clamp, _pts,
                     initial_game)

STEP = 2                                 # both sides move 2 px per step
MIRROR = 78                              # x -> 78 - x: body top-lefts 4..74 map onto themselves
BX, BY, B_CD, B_SCORE = OX, OY, O_CD, O_SCORE


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


def step_numpy(game, actions, limit=DEFAULT_LIMIT):
    """One step of every row of `game` ([G,16] int32, updated in place) under `actions` [2G]
    (player order).  Returns (reward float64 [2G], over bool [2G], ep_score int32 [2G], 0 where
    not over)."""
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
    cols = (ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t)
    for i, (v, f) in enumerate(zip(cols, fresh)):
        game[:, i] = np.where(over, f, v).astype(np.int32)
    game[:, RNG + 1:] = 0                                  # rng (column 9) is carried unchanged
    reward = (pa - pb).astype(np.float64)
    return (np.concatenate([reward, -reward]), np.concatenate([over, over]),
            np.concatenate([ep, -ep]).astype(np.int32))


def render_numpy(game):
    """[2G,84,84] uint8 frames in player order: side A's frames of the rows, then side B's (the
    frames of the mirrored rows)."""
    return np.concatenate([boxing.render_numpy(game), boxing.render_numpy(mirror_rows(game))])


class BoxingDuelVec(object):
    """G two-player GridBoxing games in HBM: E = 2G players with BoxingVec's interface (`E`,
    `A`, `frames()`, `reset_history`, `step(actions) -> frames, reward, over`,
    `step_into(actions, hist)`, `last_over`, `last_ep_score`, `game`, `ep_score`), all over the
    E players in player order; `game` is [G,16].  Every step is one HIP launch
    (ba3c_boxing_duel_step).  No frame skip and no sticky actions."""

    A = NUM_ACTIONS

    def __init__(self, n_games, seed=0, limit=DEFAULT_LIMIT, device="cuda"):
        import torch

        from . import _lib
        self.lib = _lib.load()
        self._check = _lib.check
        self._torch = torch
        self.G = int(n_games)
        self.E = 2 * self.G
        self.limit = int(limit)
        if self.G < 1 or self.limit < 1:
            raise ValueError("n_games and limit must be >= 1")
        self.device = torch.device(device)
        dev = self.device
        self.game = torch.from_numpy(initial_game(self.G, seed)).to(dev)
        self.reward = torch.zeros(self.E, dtype=torch.float64, device=dev)
        self.over = torch.zeros(self.E, dtype=torch.uint8, device=dev)
        self.ep_score = torch.zeros(self.E, dtype=torch.int32, device=dev)
        self.frame = torch.zeros((self.E, H, W, 1), dtype=torch.uint8, device=dev)
        self._palette = None               # PALETTE on the device, uploaded by the first view()

    def _ptr(self, t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream().cuda_stream)

    def frames(self):
        """[E,84,84,1] uint8 frames of the current state, each player's own (a new tensor)."""
        out = self._torch.empty_like(self.frame)
        self._check(self.lib.ba3c_boxing_duel_render(self._stream(), self._ptr(self.game), self.G,
                                                     self._ptr(out), None))
        return out

    def reset_history(self, hist):
        """Start `hist` (FrameHistory 4x1 over the E players) from the current frames."""
        self._check_hist(hist)
        self._check(self.lib.ba3c_boxing_duel_render(self._stream(), self._ptr(self.game), self.G,
                                                     None, self._ptr(hist.state)))
        return hist.state

    def _check_hist(self, hist):
        if (hist.H, hist.c, hist.E) != (4, 1, self.E) or not hist.state.is_contiguous():
            raise ValueError("the fused push needs a FrameHistory(n_envs=%d, hist_len=4, channels=1)"
                             % self.E)

    def _step(self, actions, frame, state):
        a = actions.to(device=self.device, dtype=self._torch.int64).contiguous()
        assert a.shape == (self.E,)
        self._check(self.lib.ba3c_boxing_duel_step(
            self._stream(), self._ptr(self.game), self._ptr(a), self.G, self.limit,
            self._ptr(self.reward), self._ptr(self.over), self._ptr(self.ep_score),
            self._ptr(frame), self._ptr(state)))
        return self.reward, self.over.view(self._torch.bool)

    def step(self, actions):
        """-> (frames [E,84,84,1] uint8, reward float64 [E], over bool [E]); the tensors are
        this object's buffers, overwritten by the next step."""
        reward, over = self._step(actions, self.frame, None)
        return self.frame, reward, over

    def step_into(self, actions, hist):
        """Step and push every player's new frame into `hist.state` in the same launch.
        -> (reward float64 [E], over bool [E])."""
        self._check_hist(hist)
        return self._step(actions, None, hist.state)

    def view(self, scale=1, sel=None, hud=None):
        """The colour view of the current GAMES, the world as side A sees it
        (ba3c_amd.view.view_numpy of the rows with GridBoxing's palette): torch.uint8
        [n, Hc*scale, 84*scale, 3] through ba3c_boxing_view; sel: game indices (None: all G)."""
        from .view import device_view
        return device_view(self, self.lib.ba3c_boxing_view, PALETTE, scale, sel, hud, n_rows=self.G)

    @property
    def last_over(self):
        return self.over.view(self._torch.bool)

    @property
    def last_ep_score(self):
        """(ep_score int32 [E], over bool [E]) of the last step: ep_score[p] is player p's score
        of the finished episode where over[p], stale elsewhere."""
        return self.ep_score, self.last_over


class _PolicySide(object):
    """What evaluate.EvalPlayers asks of an engine, for a side that is a bare policy callable."""

    num_actions = NUM_ACTIONS

    def __init__(self, device):
        import torch

        from .engine import greedy
        self.device = torch.device(device)
        self.greedy = greedy


def match(side_a, side_b, n_games, episodes, seed=0, limit=DEFAULT_LIMIT, device=None):
    """Play side_a (side A of every game) against side_b on `n_games` games until `episodes`
    games have finished; those finishing in the same step as the last one are counted too (as
    eval_with_envs counts them).  A side is an engine or a policy(state) -> probs [G, A]
    callable; each decides from its own half of the stacked state along evaluation's path
    (greedy, eps = 0.001, PreventStuckPlayer(30, 1) per player) with its own RandomState derived
    from `seed`.  Returns a dict: episodes, wins / draws / losses of side A (the sign of its
    ep_score), mean_score / max_score of side A's ep_score, and scores, one per episode in the
    order they finished."""
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
    env = BoxingDuelVec(G, seed=seed, limit=limit, device=device)
    hist = FrameHistory(env.E, hist_len=4, channels=1, device=env.device)
    env.reset_history(hist)
    scores = []
    while len(scores) < episodes:
        acts = [p.decide(s)[2] for p, s in zip(players, (hist.state[:G], hist.state[G:]))]
        _, over = env.step_into(torch.cat(acts), hist)
        players[0].ended(over[:G])
        players[1].ended(over[G:])
        over_h = over[:G].cpu().numpy()
        if over_h.any():
            scores += env.ep_score[:G].cpu().numpy()[over_h].tolist()
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
    args = resolve(p.parse_args(argv))
    if args.environment != GRID_BOXING or args.self_play:
        raise SystemExit("a match is played on -e %s, without --self_play" % GRID_BOXING)
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
    out = match(side_a, side_b, args.games, args.episodes, seed=0 if args.seed is None else args.seed,
                limit=args.limit)
    out = dict(side_a=args.load, side_b=args.load_b or "random", games=args.games, **out)
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
