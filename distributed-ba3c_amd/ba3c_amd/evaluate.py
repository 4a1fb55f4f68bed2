"""Evaluation on an on-device game (flags.GAMES: GridBreakout, GridBoxing): the reference's
`eval_with_funcs` / `play_one_episode` and its `Evaluator` callback (OpenAIGym/common.py:24-141)
over a vector of on-device simulators.

The reference runs NR_PROC evaluation players (get_player(train=False): HistoryFramePlayer,
PreventStuckPlayer(30, 1), LimitLengthPlayer) on threads that share one predictor; here the
players are the rows of one `BreakoutVec` / `BoxingVec`, all answered by ONE predictor forward
per step:

  state (FrameHistory) -> engine.forward -> greedy_actions (argmax, the action space's sample
  where random() < 0.001) -> PreventStuckPlayer(30, 1) per env -> fused step + history push

Evaluation is off the hot path: the PreventStuck bookkeeping is a few small torch ops and
every step fetches `over` / `ep_score` to the host to count the finished episodes.
"""
import numpy as np
import torch

from .breakout import DEFAULT_LIMIT
from .flags import GAMES, GRID_BREAKOUT
from .metrics import StatCounter
from .predict import greedy_actions
from .rollout import FrameHistory

STUCK_REPEAT, STUCK_ACTION = 30, 1     # PreventStuckPlayer(pl, 30, 1), train.py:126
GREEDY_EPS = 0.001                     # common.py:28


class EvalPlayers(object):
    """The decision path of n_envs evaluation players, shared by eval_with_envs,
    ba3c_amd.record and ba3c_amd.duel.match (one per side): greedy + eps from `rs` (a numpy RandomState) + PreventStuckPlayer(30, 1)."""

    def __init__(self, engine, n_envs, rs, policy=None):
        dev = engine.device
        self.engine, self.n_envs, self.rs, self.policy = engine, n_envs, rs, policy
        self.last = torch.full((n_envs,), -1, dtype=torch.int64, device=dev)
        self.run = torch.zeros(n_envs, dtype=torch.int64, device=dev)
        self.fire = torch.full((n_envs,), STUCK_ACTION, dtype=torch.int64, device=dev)

    def decide(self, state):
        """One decision of every player from `state` [n_envs,84,84,4]: forward, choose.
        -> (probs, value, act): the policy's output (value is None under a `policy`) and the
        actions to hand to the env (after PreventStuck).  Follow the env's step by `ended`."""
        engine, n_envs, rs, dev = self.engine, self.n_envs, self.rs, self.engine.device
        value = None
        if self.policy is None:
            probs, _, value = engine.forward(state)
        else:
            probs = self.policy(state)
        u = torch.from_numpy(rs.random_sample(n_envs)).to(dev)
        sample = torch.from_numpy(rs.randint(engine.num_actions, size=n_envs).astype(np.int64)).to(dev)
        act = greedy_actions(engine, probs, u, sample, GREEDY_EPS)
        # PreventStuckPlayer: the last STUCK_REPEAT chosen actions are all the same -> FIRE
        self.run = torch.where((act == self.last) & (self.run > 0), self.run + 1, torch.ones_like(self.run))
        self.last = act
        act = torch.where(self.run >= STUCK_REPEAT, self.fire, act)
        return probs, value, act

    def ended(self, over):
        """The players whose episode ended in the step that followed `decide` (bool [n_envs])."""
        self.run = torch.where(over, torch.zeros_like(self.run), self.run)      # act_que.clear()

    def step(self, env, hist, before_step=None):
        """One decision of every player: forward, choose, fused step + history push.
        before_step(probs, value, act) sees the policy's output and the actions handed to the
        env (after PreventStuck) while `env` still holds the state they were chosen for; value
        is None under a `policy`.  -> (reward, over) of env.step_into."""
        probs, value, act = self.decide(hist.state)
        if before_step is not None:
            before_step(probs, value, act)
        reward, over = env.step_into(act, hist)
        self.ended(over)
        return reward, over


def eval_with_envs(engine, nr_eval, n_envs, seed=0, limit=DEFAULT_LIMIT, policy=None,
                   game=GRID_BREAKOUT, frame_skip=1, sticky=0.0):
    """Play `n_envs` evaluation players of `game` (a key of flags.GAMES) with `engine`'s greedy
    policy until `nr_eval` episodes have finished; returns (mean, max) of their scores (common.py:42-86).
    Episodes that finish in the same step as the nr_eval-th are counted too (the reference
    also feeds the runs its workers were finishing).  `limit` is LimitLengthPlayer's.
    policy(state) -> probs [E,A] replaces the engine's forward (e.g. a uniform-random
    baseline); the argmax / eps / PreventStuck path is the same.  frame_skip / sticky: the
    vector's (ba3c_amd.frameskip); PreventStuck keeps counting chosen actions, one per decision,
    and `limit` counts game steps."""
    assert nr_eval >= 1 and 1 <= n_envs <= engine.max_batch
    dev, A = engine.device, engine.num_actions
    rs = np.random.RandomState(seed)
    env = GAMES[game][0](n_envs, seed=seed, limit=limit, device=dev, frame_skip=frame_skip,
                         sticky=sticky)
    assert env.A <= A
    hist = FrameHistory(n_envs, hist_len=4, channels=1, device=dev)
    env.reset_history(hist)
    players = EvalPlayers(engine, n_envs, rs, policy)
    stat = StatCounter()
    while stat.count < nr_eval:
        _, over = players.step(env, hist)
        over_h = over.cpu().numpy()
        if over_h.any():
            for s in env.ep_score.cpu().numpy()[over_h]:
                stat.feed(float(s))
    return float(stat.average), float(stat.max)


def uniform_policy(num_actions):
    """policy= for eval_with_envs: a fresh U(0,1) row per state, so the argmax is a uniform
    random action (the score of a policy that knows nothing)."""
    def f(state):
        return torch.rand(state.shape[0], num_actions, dtype=torch.float32, device=state.device)
    return f


class Evaluator(object):
    """The Evaluator callback (common.py:94-141): calling it plays `nr_eval` episodes and
    writes `mean_score` / `max_score` (trainer.write_scalar_summary) and the ('score', mean,
    max) message to the metrics client."""

    def __init__(self, engine, nr_eval, client=None, n_envs=None, seed=0, limit=DEFAULT_LIMIT,
                 worker_id=0, game=GRID_BREAKOUT, frame_skip=1, sticky=0.0):
        self.engine, self.nr_eval, self.client = engine, int(nr_eval), client
        # NR_PROC = min(cpu_count // 2, 20) players in the reference (common.py:118)
        self.n_envs = int(n_envs) if n_envs else max(1, min(self.nr_eval, 20, engine.max_batch))
        self.seed, self.limit, self.worker_id, self.game = seed, limit, worker_id, game
        self.frame_skip, self.sticky = frame_skip, sticky
        self.calls = 0
        self.history = []

    def __call__(self):
        mean, mx = eval_with_envs(self.engine, self.nr_eval, self.n_envs,
                                  seed=self.seed + self.calls, limit=self.limit,
                                  game=self.game, frame_skip=self.frame_skip, sticky=self.sticky)
        self.calls += 1
        self.history.append((mean, mx))
        if self.client is not None:
            self.client.write_scalar("mean_score", mean)
            self.client.write_scalar("max_score", mx)
            self.client.send((self.worker_id, ("score", mean, mx)))
        return mean, mx
