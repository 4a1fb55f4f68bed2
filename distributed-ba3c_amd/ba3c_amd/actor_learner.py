"""End-to-end BA3C actor-learner loop on one GPU (BASELINE configs[0] "plumbing": the
reference's 1 worker + 1 PS Breakout run, with a synthetic environment in place of gym/ALE,
which are not installable here).

One iteration is the reference's per-simulator message cycle (RL/simulator.py:95-109,
:160-185 and MySimulatorMaster, OpenAIGym/train.py:364-437) for every simulator at once:

  state (FrameHistory, RL/history.py) -> predictor forward ('logitsT', 'pred_value') ->
  action = np.random.choice semantics on the GPU from host MT19937 draws (train.py:382) ->
  RolloutBuffer.on_state -> env step -> FrameHistory.push -> RolloutBuffer.on_reward
  (n-step returns, train.py:408-437) -> BatchQueue (BatchData) -> Ba3cTrainer.train_step

With a PPO setting (ActorLearner(ppo=...), ba3c_amd.ppo) the datapoints go to a replay pool
instead of the BatchQueue and every pool is trained for several passes with the clipped-surrogate
loss; without one the loop is the reference's.

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


class ActorLearner(object):
    """The loop above around an existing Ba3cTrainer (whose model engine also serves as the
    predictor: the reference's towerp0 reads the same variables, train.py:355-362)."""

    def __init__(self, trainer, n_envs, batch_size, seed=0, rs=None, on_train_step=None,
                 dummy_predictor=False, env=None, local_time_max=LOCAL_TIME_MAX, gamma=GAMMA,
                 gae_lambda=1.0, ppo=None):
        """ppo: None is the A3C loop; a ppo.Setting(clip, epochs, minibatches) records each action's
        log-probability under the policy that drew it (sample_logp on the forward's 'logitsT' /
        'logits'), feeds a ppo.Pool of minibatches * batch_size datapoints instead of the
        BatchQueue, trains every minibatch the pool yields with the clipped-surrogate loss and
        keeps the last step's per-sample ratio on the device (last_ratio).  stop_at (an attribute, None: off) ends a pool early once the trainer's
        global_step reaches it.
        The setting's norm_adv normalises each gathered minibatch's advantages on the device
        before its step (the pool's own rows keep 0 in column 3) and keeps the batch's {mean, std}
        on the device (last_adv_stats); vclip > 0 is the clipped value loss; target_kl > 0 reads
        the mean of ppo.stop_kl (mean((rho - 1) - log rho)) over an epoch's minibatches once per
        epoch — the only host synchronisation it adds — and abandons the pool's remaining epochs
        when ppo.should_stop says so.  pool_epochs lists, per pool left, the epochs it ran
        (steps / minibatches), epoch_kls every epoch mean that was read.
        local_time_max, gamma, gae_lambda: the rollout length, discount and GAE lambda of the
        RolloutBuffer's returns (--local_time_max, --gamma, --gae_lambda; the defaults are the
        reference's 5-step, 0.99, n-step recipe).
        env: the vector of simulators (None: SyntheticAtari, as before); an env with
        `step_into(actions, hist)` (BreakoutVec, BoxingVec) is stepped through it, the
        frame-history push fused into the env's launch.
        on_train_step(trainer): called after every learner step (callbacks / metrics);
        dummy_predictor: --dummy_predictor 1 (predict/base.py:94-105) — uniform policy and
        U(0,1) values instead of the network forward."""
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
        self.queue = BatchQueue(batch_size)
        self.pool = None if ppo is None else ppo_rules.Pool(
            batch_size, minibatches=ppo.minibatches, epochs=ppo.epochs, seed=seed)
        self.last_ratio = None
        self.last_adv_stats = None
        self._adv_stats = None
        self.pool_epochs = []
        self.epoch_kls = []               # every epoch mean read for the KL stop, in order
        self.stop_at = None
        self.rs = rs if rs is not None else np.random.RandomState(seed)
        self.hist.push(self.env.frames(), torch.ones(n_envs, dtype=torch.bool, device=eng.device))
        self.steps = 0
        self.train_steps = 0
        self.last_scalars = None
        self.on_train_step = on_train_step
        self.dummy_predictor = dummy_predictor

    def _predict(self, state):
        eng = self.engine
        if self.dummy_predictor:
            E, A = self.env.E, eng.num_actions
            probs = torch.full((E, A), 1.0 / A, dtype=torch.float32, device=eng.device)
            value = torch.from_numpy(self.rs.uniform(size=E).astype(np.float32)).to(eng.device)
            return probs, value
        _, probsT, value = eng.forward(state, explore_factor=self.trainer.model.explore_factor)
        return probsT, value

    def _predict_both(self, state):
        """(probsT, probs, value): the distribution sampled from and the one whose log is kept."""
        eng = self.engine
        if self.dummy_predictor:
            probs, value = self._predict(state)
            return probs, probs, value
        probs, probsT, value = eng.forward(state, explore_factor=self.trainer.model.explore_factor)
        return probsT, probs, value

    def _after_step(self):
        self.train_steps += 1
        self.last_scalars = self.trainer.model.scalars
        if self.on_train_step is not None:
            self.on_train_step(self.trainer)

    def _iterate_ppo(self):
        eng, clip = self.engine, self.ppo.clip
        state = self.hist.state
        probsT, probs, value = self._predict_both(state)
        u = torch.from_numpy(self.rs.random_sample(self.env.E)).to(eng.device)
        actions, logp, flag = eng.sample_logp(probsT, probs, u)
        self.buf.on_state(state, actions, value, logp=logp)
        if self._fused:
            reward, over = self.env.step_into(actions, self.hist)
        else:
            frames, reward, over = self.env.step(actions)
            self.hist.push(frames, over)
        self.pool.put(self.buf.on_reward(reward, over))
        while True:
            batches = self.pool.get()
            if batches is None:
                break
            M, kl, ran = self.pool.M, None, 0
            for st, ac, rows in batches:
                if self.stop_at is not None and self.trainer.global_step >= self.stop_at:
                    break
                if self.ppo.norm_adv:
                    if self._adv_stats is None:
                        self._adv_stats = torch.zeros(2, dtype=torch.float64, device=eng.device)
                    eng.ppo_norm_adv(rows, self._adv_stats)       # the gathered copy, in place
                    self.last_adv_stats = self._adv_stats
                self.trainer.train_step(st, ac, None, rows=rows, clip=clip, vclip=self.ppo.vclip,
                                        adv_from_row=self.ppo.norm_adv)
                self.last_ratio = self.trainer.model.ratio
                self._after_step()
                ran += 1
                if self.ppo.target_kl > 0:
                    rho = self.last_ratio.double()
                    step_kl = ((rho - 1.0) - torch.log(rho)).mean()      # ppo.stop_kl, on the device
                    kl = step_kl if kl is None else kl + step_kl
                    if ran % M == 0:                              # an epoch's end: the one host read
                        self.epoch_kls.append(float((kl / M).item()))
                        if ppo_rules.should_stop(self.epoch_kls[-1], self.ppo.target_kl):
                            break
                        kl = None
            self.pool_epochs.append(ran / float(M))
        self.steps += 1
        if int(flag.item()) & 1:
            raise AssertionError("non-finite action distribution (train.py:381)")

    def iterate(self):
        if self.ppo is not None:
            return self._iterate_ppo()
        eng = self.engine
        state = self.hist.state
        probsT, value = self._predict(state)
        u = torch.from_numpy(self.rs.random_sample(self.env.E)).to(eng.device)
        actions, flag = eng.sample(probsT, u)
        self.buf.on_state(state, actions, value)
        if self._fused:
            reward, over = self.env.step_into(actions, self.hist)
        else:
            frames, reward, over = self.env.step(actions)
            self.hist.push(frames, over)
        self.queue.put(self.buf.on_reward(reward, over))
        while True:
            b = self.queue.get()
            if b is None:
                break
            self.trainer.train_step(b[0].contiguous(), b[1].contiguous(), b[2].contiguous())
            self._after_step()
        self.steps += 1
        if int(flag.item()) & 1:
            raise AssertionError("non-finite action distribution (train.py:381)")

    def run(self, n):
        for _ in range(n):
            self.iterate()
        return self
