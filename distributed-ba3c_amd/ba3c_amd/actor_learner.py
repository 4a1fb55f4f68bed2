"""End-to-end BA3C actor-learner loop on one GPU (BASELINE configs[0] "plumbing": the
reference's 1 worker + 1 PS Breakout run, with a synthetic environment in place of gym/ALE,
which are not installable here).

One iteration is the reference's per-simulator message cycle (RL/simulator.py:95-109,
:160-185 and MySimulatorMaster, OpenAIGym/train.py:364-437) for every simulator at once:

  state (FrameHistory, RL/history.py) -> predictor forward ('logitsT', 'pred_value') ->
  action = np.random.choice semantics on the GPU from host MT19937 draws (train.py:382) ->
  RolloutBuffer.on_state -> env step -> FrameHistory.push -> RolloutBuffer.on_reward
  (n-step returns, train.py:408-437) -> a consumer of the datapoints

The consumer is a BatchTrainer (BatchQueue (BatchData) -> Ba3cTrainer.train_step: the reference's
loop) or, with a PPO setting (ActorLearner(ppo=...), ba3c_amd.ppo), a PoolTrainer: a replay pool
whose every minibatch is trained for several passes with the clipped-surrogate loss.

The synthetic environment is NOT part of the reference's hot path; it only produces frames,
rewards and episode ends with the shapes and value ranges of the Atari pipeline (84x84
grayscale frames, integer rewards incl. values outside [-1, 1] that the returns clip).
"""
import numpy as np
import torch

from . import ppo as ppo_rules
from .rollout import GAMMA, LOCAL_TIME_MAX, BatchQueue, FrameHistory, RolloutBuffer


class SyntheticAtari(object):
    """E simulators on the device: frame_e(t) is a moving byte pattern, the reward is 1 when
    the action matches a per-step target (3 every 7th step: clipped by the returns), episodes
    last 20..80 steps."""

    def __init__(self, n_envs, num_actions=4, seed=0, device="cuda"):
        self.E, self.A = int(n_envs), int(num_actions)
        self.device = torch.device(device)
        self.g = torch.Generator(device=self.device).manual_seed(seed)
        self.t = torch.zeros(self.E, dtype=torch.int64, device=self.device)
        self.L = self._lengths()
        yy = torch.arange(84, device=self.device).view(1, 84, 1)
        xx = torch.arange(84, device=self.device).view(1, 1, 84)
        self._base = (3 * xx + 5 * yy)                       # [1,84,84]
        self._eid = torch.arange(self.E, device=self.device).view(-1, 1, 1)

    def _lengths(self):
        return torch.randint(20, 81, (self.E,), generator=self.g, device=self.device)

    def frames(self):
        f = (self._base + 7 * self.t.view(-1, 1, 1) + 11 * self._eid) & 255
        return f.to(torch.uint8).unsqueeze(-1).contiguous()     # [E,84,84,1]

    def step(self, actions):
        target = (self.t + torch.arange(self.E, device=self.device)) % self.A
        hit = (actions.to(torch.int64) == target).to(torch.float64)
        reward = torch.where(self.t % 7 == 6, 3.0 * hit, hit)
        self.t += 1
        over = self.t >= self.L
        if bool(over.any()):
            newL = self._lengths()
            self.L = torch.where(over, newL, self.L)
            self.t = torch.where(over, torch.zeros_like(self.t), self.t)
        return self.frames(), reward, over


class BatchTrainer(object):
    """The A3C consumer: BatchData(B) over the datapoints, one learner step per complete batch."""

    def __init__(self, trainer, batch_size, after_step):
        self.trainer, self.after_step = trainer, after_step
        self.queue = BatchQueue(batch_size)

    def consume(self, dps):
        self.queue.put(dps)
        while True:
            b = self.queue.get()
            if b is None:
                break
            self.trainer.train_step(b[0].contiguous(), b[1].contiguous(), b[2].contiguous())
            self.after_step()


class PoolTrainer(object):
    """The PPO consumer: a ppo.Pool of minibatches * batch_size datapoints, every minibatch it
    yields trained with the clipped-surrogate loss of `setting` (a ppo.Setting).
    last_ratio: the last step's per-sample ratio, on the device.
    last_adv_stats: with norm_adv, the {mean, std} of the last minibatch normalised, two doubles on
      the device (the pool's own rows keep 0 in column 3); None without.
    pool_epochs: per pool left, the epochs it ran (steps / minibatches).
    epoch_kls: with target_kl > 0, every epoch's mean of ppo.stop_kl over its minibatches, read
      once per epoch (the only host synchronisation added); ppo.should_stop on it abandons the
      pool's remaining epochs.
    stop_at (None: off): a pool ends early once the trainer's global_step reaches it."""

    def __init__(self, trainer, setting, batch_size, seed, after_step, stop_at=None):
        self.trainer, self.setting, self.after_step = trainer, setting, after_step
        self.stop_at = stop_at
        self.pool = ppo_rules.Pool(batch_size, minibatches=setting.minibatches,
                                   epochs=setting.epochs, seed=seed)
        self.last_ratio = None
        self.last_adv_stats = torch.zeros(
            2, dtype=torch.float64, device=trainer.engine.device) if setting.norm_adv else None
        self.pool_epochs = []
        self.epoch_kls = []
        self._kl = None                   # the running epoch's sum of step KLs, on the device

    def consume(self, dps):
        self.pool.put(dps)
        while True:
            batches = self.pool.get()
            if batches is None:
                break
            self.pool_epochs.append(self._train(batches) / float(self.pool.M))

    def _train(self, batches):
        """The steps run on one pool's minibatches."""
        ran, self._kl = 0, None
        for st, ac, rows in batches:
            if self._cut_off():
                break
            self._normalise(rows)
            self._step(st, ac, rows)
            ran += 1
            if self._kl_stops(ran):
                break
        return ran

    def _cut_off(self):
        return self.stop_at is not None and self.trainer.global_step >= self.stop_at

    def _normalise(self, rows):
        if self.setting.norm_adv:
            self.trainer.engine.ppo_norm_adv(rows, self.last_adv_stats)    # the gathered copy, in place

    def _step(self, st, ac, rows):
        s = self.setting
        self.trainer.train_step(st, ac, None, rows=rows, clip=s.clip, vclip=s.vclip,
                                adv_from_row=s.norm_adv)
        self.last_ratio = self.trainer.model.ratio
        self.after_step()

    def _kl_stops(self, ran):
        """Adds the step's KL to the epoch's sum; at an epoch's end (the one host read) whether
        its mean stops the pool."""
        if not self.setting.target_kl > 0:
            return False
        step_kl = ppo_rules.stop_kl_device(self.last_ratio)
        self._kl = step_kl if self._kl is None else self._kl + step_kl
        if ran % self.pool.M:
            return False
        self.epoch_kls.append(float((self._kl / self.pool.M).item()))
        self._kl = None
        return ppo_rules.should_stop(self.epoch_kls[-1], self.setting.target_kl)


class ActorLearner(object):
    """The loop above around an existing Ba3cTrainer (whose model engine also serves as the
    predictor: the reference's towerp0 reads the same variables, train.py:355-362)."""

    def __init__(self, trainer, n_envs, batch_size, seed=0, rs=None, on_train_step=None,
                 dummy_predictor=False, env=None, local_time_max=LOCAL_TIME_MAX, gamma=GAMMA,
                 gae_lambda=1.0, ppo=None, stop_at=None, episodes=None):
        """trainer: the Ba3cTrainer that takes the learner steps.
        n_envs, batch_size: simulators stepped per iteration, datapoints per learner step.
        seed, rs: of the synthetic environment and the PPO pool; the host stream of the action
          draws (None: RandomState(seed)).
        on_train_step(trainer): called after every learner step (callbacks / metrics).
        dummy_predictor: --dummy_predictor 1 (predict/base.py:94-105), a uniform policy and
          U(0,1) values instead of the network forward.
        env: the vector of simulators (None: SyntheticAtari); one with `step_into(actions, hist)`
          (BreakoutVec, BoxingVec) has the frame-history push fused into its launch.
        local_time_max, gamma, gae_lambda: the RolloutBuffer's rollout length, discount and GAE
          lambda (the defaults are the reference's 5-step, 0.99, n-step recipe).
        ppo: None is the A3C loop (`queue`, a BatchTrainer's); a ppo.Setting records each action's
          log-probability under the policy that drew it and feeds a PoolTrainer (`pool_trainer`,
          whose Pool is `pool`).
        stop_at: the PoolTrainer's; unused without ppo.
        episodes: an episodes.EpisodeLog over the n_envs simulators (for a two-player vector its
          E = 2G players, player p of game g at p * G + g): one more launch per iteration, right
          after the environment step, logs the episodes that step finished; no host read.  None:
          no call differs."""
        eng = trainer.engine
        assert eng.channels == 4, "synthetic loop is grayscale x FRAME_HISTORY=4"
        self.trainer = trainer
        self.engine = eng
        if env is None:
            env = SyntheticAtari(n_envs, eng.num_actions, seed=seed, device=eng.device)
        assert env.E == n_envs and env.A <= eng.num_actions
        self.env = env
        self._fused = hasattr(env, "step_into")
        self.hist = FrameHistory(n_envs, hist_len=4, channels=1, device=eng.device)
        self.ppo = ppo
        if ppo is not None and trainer.model.explore_factor != 1.0:
            raise ValueError("PPO records log pi of the policy it samples from: explore_factor must be 1")
        self.buf = RolloutBuffer(n_envs, channels=4, local_time_max=local_time_max, gamma=gamma,
                                 gae_lambda=gae_lambda, device=eng.device, logp=ppo is not None)
        if ppo is None:
            self.consumer = BatchTrainer(trainer, batch_size, self._after_step)
            self.queue, self.pool_trainer, self.pool = self.consumer.queue, None, None
        else:
            self.consumer = PoolTrainer(trainer, ppo, batch_size, seed, self._after_step, stop_at)
            self.queue, self.pool_trainer, self.pool = None, self.consumer, self.consumer.pool
        self.rs = rs if rs is not None else np.random.RandomState(seed)
        self.hist.push(self.env.frames(), torch.ones(n_envs, dtype=torch.bool, device=eng.device))
        self.steps = 0
        self.train_steps = 0
        self.last_scalars = None
        self.on_train_step = on_train_step
        self.dummy_predictor = dummy_predictor
        if episodes is not None and episodes.E != n_envs:
            raise ValueError("the episode log is of %d simulators, the loop of %d" % (episodes.E, n_envs))
        self.episodes = episodes

    def _predict(self, state):
        """(sampled_from, recorded, value): the distribution the action is drawn from, the one
        whose log is kept (PPO) and the value."""
        eng = self.engine
        if self.dummy_predictor:
            E, A = self.env.E, eng.num_actions
            probs = torch.full((E, A), 1.0 / A, dtype=torch.float32, device=eng.device)
            value = torch.from_numpy(self.rs.uniform(size=E).astype(np.float32)).to(eng.device)
            return probs, probs, value
        probs, probsT, value = eng.forward(state, explore_factor=self.trainer.model.explore_factor)
        return probsT, probs, value

    def _after_step(self):
        self.train_steps += 1
        self.last_scalars = self.trainer.model.scalars
        if self.on_train_step is not None:
            self.on_train_step(self.trainer)

    def iterate(self):
        eng = self.engine
        state = self.hist.state
        sampled_from, recorded, value = self._predict(state)
        u = torch.from_numpy(self.rs.random_sample(self.env.E)).to(eng.device)
        if self.ppo is not None:
            actions, logp, flag = eng.sample_logp(sampled_from, recorded, u)
            self.buf.on_state(state, actions, value, logp=logp)
        else:
            actions, flag = eng.sample(sampled_from, u)
            self.buf.on_state(state, actions, value)
        if self._fused:
            reward, over = self.env.step_into(actions, self.hist)
        else:
            frames, reward, over = self.env.step(actions)
            self.hist.push(frames, over)
        if self.episodes is not None:
            self.episodes.update(reward, over)
        self.consumer.consume(self.buf.on_reward(reward, over))
        self.steps += 1
        if int(flag.item()) & 1:
            raise AssertionError("non-finite action distribution (train.py:381)")

    def run(self, n):
        for _ in range(n):
            self.iterate()
        return self
