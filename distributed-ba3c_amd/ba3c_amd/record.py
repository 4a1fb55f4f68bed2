"""Record whole episodes of an on-device game (flags.GAMES) as checkable traces: the reference's
`record_model.py` over a vector of on-device simulators.

The players are `evaluate.EvalPlayers`, the decision path of `eval_with_envs` (greedy + eps +
PreventStuckPlayer(30, 1)) drawn from the same RandomState(seed), so a recording shows what an
evaluation with the same arguments plays.  An `Episode` keeps the row the episode started from
(and the aux row under frame skip), the actions handed to the env, the rewards, the policy's
output and colour frames (ba3c_amd.view, drawn on the GPU next to the games).  (row0, actions)
determines the episode exactly: `Episode.replay()` runs the CPU oracle (`step_numpy`, or
`frameskip.step_numpy`) over them and returns what must equal the recording bit for bit.

Frame j shows the game the policy saw at decision `frame_steps[j]`, i.e. `replay()`'s
rows[frame_steps[j]], with that decision's output in the HUD.

    python -m ba3c_amd.record --load CKPT -e GridBoxing-v0 --num_actions 18 --fc_neurons 128 \\
        --fc_splits 4 --episodes 3 --scale 3 --out DIR [--frame_skip 2-4 --sticky 0.25]
    python -m ba3c_amd.record --random -e GridBreakout-v0 --episodes 3 --out DIR

Matches of two-player GridBoxing (ba3c_amd.duel) are recorded by `record_match`, along
`duel.match`'s own decision path, as `MatchEpisode`s: the same trace with both sides' actions and
outputs, replayed through `duel.decide_numpy` / `duel.step_numpy`
(`python -m ba3c_amd.duel ... --record DIR`).
"""
import json
import os

import numpy as np

from . import boxing, breakout, duel, frameskip
from .breakout import DEFAULT_LIMIT
from .flags import GAMES, GRID_BOXING, GRID_BREAKOUT, build_parser, resolve

MODULES = {GRID_BREAKOUT: breakout, GRID_BOXING: boxing}
ARRAYS = ("row0", "aux0", "actions", "rewards", "probs", "values", "frames", "frame_steps")


class Episode(object):
    """One recorded episode of `game` (a key of flags.GAMES) under `limit` and `skip` ((lo, hi,
    q16) of ba3c_amd.frameskip, or None: plain steps).  row0 int32 [16]; aux0 int32 [2] (None
    without skip); actions int64 [T]; rewards float64 [T]; probs float32 [T, A]; values float32
    [T]; score, steps = T; frames uint8 [T', Hc*S, 84*S, 3]; frame_steps int64 [T']."""

    def __init__(self, game, limit, skip, row0, aux0, actions, rewards, probs, values, score,
                 frames, frame_steps):
        assert game in MODULES and (aux0 is not None) == (skip is not None)
        self.game, self.limit = game, int(limit)
        self.skip = tuple(int(v) for v in skip) if skip is not None else None
        self.row0 = np.asarray(row0, np.int32).reshape(16)
        self.aux0 = np.asarray(aux0, np.int32).reshape(frameskip.AUX_INTS) if skip is not None else None
        self.actions = np.asarray(actions, np.int64).reshape(-1)
        self.steps = int(self.actions.shape[0])
        self.rewards = np.asarray(rewards, np.float64).reshape(self.steps)
        self.probs = np.asarray(probs, np.float32).reshape(self.steps, -1)
        self.values = np.asarray(values, np.float32).reshape(self.steps)
        self.score = int(score)
        self.frames = np.asarray(frames, np.uint8)
        self.frame_steps = np.asarray(frame_steps, np.int64).reshape(-1)
        assert self.frames.shape[0] == self.frame_steps.shape[0]

    def replay(self):
        """Run the CPU oracle from row0 (and aux0) over `actions`.  -> (rows int32 [T+1, 16]
        with rows[0] = row0 and rows[t+1] the row after decision t, rewards float64 [T], score:
        the ep_score of the step that ended the episode, None if none did)."""
        K = MODULES[self.game]
        game = self.row0.reshape(1, 16).copy()
        aux = self.aux0.reshape(1, -1).copy() if self.skip is not None else None
        rows = np.zeros((self.steps + 1, 16), np.int32)
        rewards = np.zeros(self.steps, np.float64)
        rows[0], score = game[0], None
        for t in range(self.steps):
            a = self.actions[t:t + 1]
            if self.skip is None:
                r, over, ep = K.step_numpy(game, a, self.limit)
            else:
                r, over, ep = frameskip.step_numpy(K, game, aux, a, self.limit, *self.skip)
            rows[t + 1], rewards[t] = game[0], r[0]
            if over[0]:
                score = int(ep[0])
        return rows, rewards, score

    def save(self, path_stem, gif_ms=50):
        """Write <stem>.npz (plain arrays, no pickled objects) and, if PIL imports, <stem>.gif
        of the frames.  -> the files written."""
        d = os.path.dirname(path_stem)
        if d:
            os.makedirs(d, exist_ok=True)
        out = {k: getattr(self, k) for k in ARRAYS if getattr(self, k) is not None}
        out.update(game=np.array(self.game), limit=np.int64(self.limit), score=np.int64(self.score),
                   steps=np.int64(self.steps))
        if self.skip is not None:
            out["skip"] = np.asarray(self.skip, np.int64)
        np.savez_compressed(path_stem + ".npz", **out)
        files = [path_stem + ".npz"]
        try:
            from PIL import Image
        except ImportError:
            return files
        if self.frames.shape[0]:
            images = [Image.fromarray(f) for f in self.frames]
            images[0].save(path_stem + ".gif", save_all=True, append_images=images[1:],
                           duration=gif_ms, loop=0)
            files.append(path_stem + ".gif")
        return files

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as f:
            d = {k: f[k] for k in f.files}
        skip = tuple(d["skip"].tolist()) if "skip" in d else None
        return cls(str(d["game"]), int(d["limit"]), skip, d["row0"], d.get("aux0"), d["actions"],
                   d["rewards"], d["probs"], d["values"], int(d["score"]), d["frames"], d["frame_steps"])


class _Open(object):
    """An episode in progress on one simulator."""

    def __init__(self, row0, aux0):
        self.row0, self.aux0 = row0, aux0
        self.actions, self.rewards, self.probs, self.values = [], [], [], []
        self.frames, self.frame_steps = [], []


def record_episodes(engine, game, n_episodes, n_envs=None, seed=0, limit=DEFAULT_LIMIT, frame_skip=1,
                    sticky=0.0, policy=None, scale=3, hud=True, every=1, max_frames=2000):
    """Play `n_envs` evaluation players of `game` until `n_episodes` episodes have finished and
    return them as Episodes, in the order they finished (those finishing in the same step as the
    n_episodes-th included, as eval_with_envs counts them).  policy(state) -> probs [E, A]
    replaces the engine's forward (values are then recorded as 0).  Every `every`-th decision's
    frame is kept, at most `max_frames` per episode; hud: draw the policy's output under it."""
    import torch

    from .evaluate import EvalPlayers
    from .rollout import FrameHistory
    from .view import ACTIONS, HUD_H, W, check_scale, hud_from_policy
    n_envs = int(n_envs) if n_envs else max(1, min(int(n_episodes), 20, engine.max_batch))
    assert n_episodes >= 1 and 1 <= n_envs <= engine.max_batch and every >= 1 and max_frames >= 0
    scale = check_scale(scale)
    dev = engine.device
    env = GAMES[game][0](n_envs, seed=seed, limit=limit, device=dev, frame_skip=frame_skip,
                         sticky=sticky)
    assert env.A <= engine.num_actions
    hist = FrameHistory(n_envs, hist_len=4, channels=1, device=dev)
    env.reset_history(hist)
    players = EvalPlayers(engine, n_envs, np.random.RandomState(seed), policy)

    def start(which):
        rows = env.game.cpu().numpy()
        auxs = env.aux.cpu().numpy() if env.aux is not None else None
        for e in which:
            live[e] = _Open(rows[e].copy(), auxs[e].copy() if auxs is not None else None)

    def before_step(probs, value, act):
        probs_h, act_h = probs.cpu().numpy(), act.cpu().numpy()
        value_h = value.cpu().numpy() if value is not None else np.zeros(n_envs, np.float32)
        want = [e for e in range(n_envs)
                if len(live[e].actions) % every == 0 and len(live[e].frames) < max_frames]
        if want:
            sel = torch.tensor(want, dtype=torch.int32, device=dev)
            bytes_ = hud_from_policy(probs[:, :ACTIONS], act, value)[sel.long()] if hud else None
            frames = env.view(scale=scale, sel=sel, hud=bytes_).cpu().numpy()
            for j, e in enumerate(want):
                live[e].frame_steps.append(len(live[e].actions))
                live[e].frames.append(frames[j])
        for e in range(n_envs):
            ep = live[e]
            ep.actions.append(act_h[e])
            ep.probs.append(probs_h[e])
            ep.values.append(value_h[e])

    live, done = [None] * n_envs, []
    start(range(n_envs))
    hc = W + (HUD_H if hud else 0)
    while len(done) < n_episodes:
        reward, over = players.step(env, hist, before_step)
        reward_h, over_h = reward.cpu().numpy(), over.cpu().numpy()
        for e in range(n_envs):
            live[e].rewards.append(reward_h[e])
        if over_h.any():
            scores = env.ep_score.cpu().numpy()
            ended = np.nonzero(over_h)[0].tolist()
            for e in ended:
                ep = live[e]
                frames = (np.stack(ep.frames) if ep.frames
                          else np.zeros((0, hc * scale, W * scale, 3), np.uint8))
                done.append(Episode(game, limit, env.skip, ep.row0, ep.aux0, ep.actions, ep.rewards,
                                    np.stack(ep.probs), ep.values, scores[e], frames, ep.frame_steps))
            start(ended)                      # the rows have auto-reset: the next episodes' row0
    return done


MATCH_ARRAYS = ("row0", "aux0", "actions", "rewards", "probs", "values", "frames", "frame_steps")


class MatchEpisode(object):
    """One recorded episode of a two-player GridBoxing game (ba3c_amd.duel) under `limit`, `skip`
    ((lo, hi, q16), or None: plain steps) and `start` ((h_lo, h_hi) of a drawn start; with skip
    None it is None).  row0 int32 [16]; aux0 int32 [8] (None without skip); actions int64 [T, 2]
    (side A's, side B's, each in its own frame of reference); rewards float64 [T], side A's;
    probs float32 [T, 2, A]; values float32 [T, 2]; score: side A's ep_score; steps = T decisions;
    frames uint8 [T', Hc*S, 84*S, 3] as `side` sees the game, frame_steps int64 [T']."""

    def __init__(self, limit, skip, start, side, row0, aux0, actions, rewards, probs, values, score,
                 frames, frame_steps):
        assert (aux0 is not None) == (skip is not None) == (start is not None) and side in ("a", "b")
        self.limit, self.side = int(limit), side
        self.skip = tuple(int(v) for v in skip) if skip is not None else None
        self.start = tuple(int(v) for v in start) if start is not None else None
        self.row0 = np.asarray(row0, np.int32).reshape(16)
        self.aux0 = np.asarray(aux0, np.int32).reshape(duel.AUX_INTS) if skip is not None else None
        self.actions = np.asarray(actions, np.int64).reshape(-1, 2)
        self.steps = int(self.actions.shape[0])
        self.rewards = np.asarray(rewards, np.float64).reshape(self.steps)
        self.probs = np.asarray(probs, np.float32).reshape(self.steps, 2, -1)
        self.values = np.asarray(values, np.float32).reshape(self.steps, 2)
        self.score = int(score)
        self.frames = np.asarray(frames, np.uint8)
        self.frame_steps = np.asarray(frame_steps, np.int64).reshape(-1)
        assert self.frames.shape[0] == self.frame_steps.shape[0]

    def replay(self):
        """Run the CPU oracle (duel.decide_numpy, or duel.step_numpy without skip) from row0 (and
        aux0) over `actions`.  -> (rows int32 [T+1, 16] with rows[0] = row0 and rows[t+1] the row
        after decision t, side A's rewards float64 [T], score: side A's ep_score of the decision
        that ended the episode, None if none did)."""
        game = self.row0.reshape(1, 16).copy()
        aux = self.aux0.reshape(1, -1).copy() if self.skip is not None else None
        rows = np.zeros((self.steps + 1, 16), np.int32)
        rewards = np.zeros(self.steps, np.float64)
        rows[0], score = game[0], None
        for t in range(self.steps):
            if self.skip is None:
                r, over, ep = duel.step_numpy(game, self.actions[t], self.limit)
            else:
                r, over, ep = duel.decide_numpy(game, aux, self.actions[t], self.limit, *self.skip,
                                                start=self.start)
            rows[t + 1], rewards[t] = game[0], r[0]
            if over[0]:
                score = int(ep[0])
        return rows, rewards, score

    def save(self, path_stem, gif_ms=50):
        """Write <stem>.npz (plain arrays, no pickled objects) and, if PIL imports, <stem>.gif
        of the frames.  -> the files written."""
        d = os.path.dirname(path_stem)
        if d:
            os.makedirs(d, exist_ok=True)
        out = {k: getattr(self, k) for k in MATCH_ARRAYS if getattr(self, k) is not None}
        out.update(side=np.array(self.side), limit=np.int64(self.limit), score=np.int64(self.score),
                   steps=np.int64(self.steps))
        if self.skip is not None:
            out.update(skip=np.asarray(self.skip, np.int64), start=np.asarray(self.start, np.int64))
        np.savez_compressed(path_stem + ".npz", **out)
        files = [path_stem + ".npz"]
        try:
            from PIL import Image
        except ImportError:
            return files
        if self.frames.shape[0]:
            images = [Image.fromarray(f) for f in self.frames]
            images[0].save(path_stem + ".gif", save_all=True, append_images=images[1:],
                           duration=gif_ms, loop=0)
            files.append(path_stem + ".gif")
        return files

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as f:
            d = {k: f[k] for k in f.files}
        skip = tuple(d["skip"].tolist()) if "skip" in d else None
        start = tuple(d["start"].tolist()) if "start" in d else None
        return cls(int(d["limit"]), skip, start, str(d["side"]), d["row0"], d.get("aux0"), d["actions"],
                   d["rewards"], d["probs"], d["values"], int(d["score"]), d["frames"], d["frame_steps"])


class _MatchWatch(object):
    """duel._play's watcher: keeps every game's episode in progress and closes it on `over`."""

    def __init__(self, scale, hud, every, max_frames, side):
        self.scale, self.hud, self.every, self.max_frames, self.side = scale, hud, every, max_frames, side
        self.done = []

    def _start(self, env, which):
        rows = env.game.cpu().numpy()
        auxs = env.aux.cpu().numpy() if env.aux is not None else None
        for e in which:
            self.live[e] = _Open(rows[e].copy(), auxs[e].copy() if auxs is not None else None)

    def begin(self, env):
        self.live = [None] * env.G
        self._start(env, range(env.G))

    def decided(self, env, outs):
        import torch

        from .view import ACTIONS, hud_from_policy
        G, live = env.G, self.live
        zeros = np.zeros(G, np.float32)
        probs_h = np.stack([o[0].cpu().numpy() for o in outs], axis=1)                  # [G, 2, A]
        value_h = np.stack([o[1].cpu().numpy() if o[1] is not None else zeros for o in outs], axis=1)
        act_h = np.stack([o[2].cpu().numpy() for o in outs], axis=1)
        want = [e for e in range(G)
                if len(live[e].actions) % self.every == 0 and len(live[e].frames) < self.max_frames]
        if want:
            sel = torch.tensor(want, dtype=torch.int32, device=env.device)
            probs, value, act = outs[0 if self.side == "a" else 1]
            bytes_ = hud_from_policy(probs[:, :ACTIONS], act, value)[sel.long()] if self.hud else None
            frames = env.view(scale=self.scale, sel=sel, hud=bytes_, side=self.side).cpu().numpy()
            for j, e in enumerate(want):
                live[e].frame_steps.append(len(live[e].actions))
                live[e].frames.append(frames[j])
        for e in range(G):
            live[e].actions.append(act_h[e])
            live[e].probs.append(probs_h[e])
            live[e].values.append(value_h[e])

    def stepped(self, env, reward_h, over_h):
        from .view import HUD_H, W
        for e in range(env.G):
            self.live[e].rewards.append(reward_h[e])
        if not over_h.any():
            return
        scores = env.ep_score[:env.G].cpu().numpy()
        ended = np.nonzero(over_h)[0].tolist()
        hc = W + (HUD_H if self.hud else 0)
        for e in ended:
            ep = self.live[e]
            frames = (np.stack(ep.frames) if ep.frames
                      else np.zeros((0, hc * self.scale, W * self.scale, 3), np.uint8))
            self.done.append(MatchEpisode(env.limit, env.skip, env.start, self.side, ep.row0, ep.aux0,
                                          np.stack(ep.actions), ep.rewards, np.stack(ep.probs),
                                          np.stack(ep.values), scores[e], frames, ep.frame_steps))
        self._start(env, ended)               # the rows have auto-reset: the next episodes' row0


def record_match(side_a, side_b, n_episodes, n_games, seed=0, limit=DEFAULT_LIMIT, frame_skip=1, sticky=0.0,
                 start=None, scale=3, hud=True, every=1, max_frames=2000, side="a", device=None):
    """Play `duel.match(side_a, side_b, n_games, n_episodes, ...)` along its own decision path and
    return the episodes as MatchEpisodes, in the order they finished: a recording shows what a
    match with the same arguments plays, and its scores are that match's.  Every `every`-th
    decision's frame is kept, at most `max_frames` per episode, drawn as `side` sees the game
    (BoxingDuelVec.view) with that side's output in the HUD; frame_skip / sticky / start:
    BoxingDuelDecisionVec's."""
    from .view import check_scale
    assert every >= 1 and max_frames >= 0 and side in ("a", "b")
    watch = _MatchWatch(check_scale(scale), hud, every, max_frames, side)
    duel._play(side_a, side_b, n_games, n_episodes, seed, limit, device, frame_skip, sticky, start, watch)
    return watch.done


def main(argv=None):
    p = build_parser()
    p.description = "record episodes of an on-device game as replayable traces (and GIFs)"
    p.add_argument("--episodes", type=int, default=3)
    p.add_argument("--scale", type=int, default=3)
    p.add_argument("--out", default="recordings")
    p.add_argument("--random", action="store_true", help="a uniform-random policy: no --load needed")
    p.add_argument("--limit", type=int, default=DEFAULT_LIMIT, help="LimitLengthPlayer's game steps")
    p.add_argument("--every", type=int, default=1, help="keep every N-th decision's frame")
    p.add_argument("--max_frames", type=int, default=2000)
    args = resolve(p.parse_args(argv))
    if args.environment not in GAMES:
        raise SystemExit("recording needs an on-device game: pass -e %s" % " or -e ".join(sorted(GAMES)))
    if not args.random and not args.load:
        raise SystemExit("pass --load CHECKPOINT, or --random for a uniform-random policy")
    if not 1 <= args.scale <= 8 or args.episodes < 1:
        raise SystemExit("--scale must be in [1, 8] and --episodes >= 1")
    from .evaluate import uniform_policy
    from .train import build
    model, _, _ = build(args)
    policy = uniform_policy(args.num_actions) if args.random else None
    episodes = record_episodes(model.engine, args.environment, args.episodes,
                               seed=0 if args.seed is None else args.seed, limit=args.limit,
                               frame_skip=args.frame_skip, sticky=args.sticky, policy=policy,
                               scale=args.scale, every=args.every, max_frames=args.max_frames)
    files = []
    for i, ep in enumerate(episodes):
        files += ep.save(os.path.join(args.out, "episode_%03d" % i))
    out = {"game": args.environment, "scores": [ep.score for ep in episodes],
           "steps": [ep.steps for ep in episodes], "files": files}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
