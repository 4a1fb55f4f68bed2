"""Training metrics with the reference's scalar names and CSV channels.

DebugLogCallback (OpenAIGym/common.py:172-288) averages the step dictionaries (`TfDictOp`
results, train/multigpu.py:193-205) over --send_debug_every steps and sends the reference's
message tuples ('loss', cost, policy_loss, xentropy_loss, value_loss, advantage, pred_reward,
max_logit), ('other', active_relus, dp_per_s) and ('delays', (mean, max, min)); the
CsvChannels sink replaces the Neptune metrics server's _dump_to_channels
(neptune_mp_server.py:169-233) writing one `<channel>.csv` ("x,y" rows, x = hours since start)
per channel as utils/neptune_utils.py:38-57 does.  StepMetrics is the launcher's per-step
callback in front of both, PpoMetrics its PPO channels; the channels of the training simulators'
episodes (`online_score`, the reference's ('online', ...) message) are episodes.EpisodeMetrics'.
ScheduleMetrics sends the reference's ('schedule', learning_rate, entropy_beta) message
(common.py:221-224, neptune_mp_server.py:204-206) and GradClipMetrics writes the global-norm clip's
grad_norm / grad_clip_fraction channels.
"""
import os
import time

import numpy as np
import torch


class StatCounter(object):
    """utils/stat.py:8-39."""

    def __init__(self):
        self.reset()

    def feed(self, v):
        self._values.append(v)

    def reset(self):
        self._values = []

    @property
    def count(self):
        return len(self._values)

    @property
    def average(self):
        assert len(self._values)
        return np.mean(self._values)

    @property
    def sum(self):
        assert len(self._values)
        return np.sum(self._values)

    @property
    def max(self):
        assert len(self._values)
        return max(self._values)


class CsvChannels(object):
    """The chief's metrics sink: Server._dump_to_channels onto `<name>.csv` channel files."""

    LOSS = ["cost", "policy_loss", "xentropy_loss", "value_loss", "advantage", "pred_reward",
            "max_logit"]

    def __init__(self, experiment_dir):
        self.dir = experiment_dir
        os.makedirs(experiment_dir, exist_ok=True)
        self.start = time.time()
        self._fd = {}

    def _send(self, name, x, y):
        fd = self._fd.get(name)
        if fd is None:
            fd = self._fd[name] = open(os.path.join(self.dir, name + ".csv"), "w")
            fd.write("x,y\n")
        fd.write("{},{}\n".format(x, y))
        fd.flush()

    def write_scalar(self, name, value):
        """trainer.write_scalar_summary(name, value) (the Evaluator's mean_score / max_score,
        common.py:131-132) as one more channel."""
        self._send(name, (time.time() - self.start) / 3600.0, value)

    def send(self, message):
        _, content = message
        x = (time.time() - self.start) / 3600.0
        kind = content[0]
        if kind == "loss":
            for name, v in zip(self.LOSS, content[1:]):
                self._send(name, x, v)
        elif kind == "other":
            self._send("active_relus", x, content[1])
            self._send("dp_per_s", x, content[2])
        elif kind == "delays":
            mean, mx, mn = content[1]
            self._send("mean_delay", x, mean)
            self._send("max_delay", x, mx)
            self._send("min_delay", x, mn)
        elif kind == "score":
            self._send("score_mean", x, content[1])
            self._send("score_max", x, content[2])
        elif kind == "online":
            self._send("online_score", x, content[1])
        elif kind == "schedule":
            self._send("learning_rate", x, content[1])
            self._send("entropy_beta", x, content[2])

    def close(self):
        for fd in self._fd.values():
            fd.close()
        self._fd = {}


class DebugLogCallback(object):
    """OpenAIGym/common.py:172-288 (the default, non-debug-chart messages)."""

    def __init__(self, client, worker_id=0, nr_send=100):
        self.client, self.worker_id, self.send_every = client, worker_id, int(nr_send)
        self.dp_per_s = StatCounter()
        self.lists = None
        self.delays = []
        self.counter = 0
        self.step_counter = 0

    def trigger_step(self, session_result, dp_per_s, delay=None):
        if self.lists is None:
            self.lists = {name: StatCounter() for name in session_result}
        for name in session_result:
            self.lists.setdefault(name, StatCounter()).feed(session_result[name])
        self.dp_per_s.feed(dp_per_s)
        if delay is not None:
            self.delays.append(delay)
        self.counter += 1
        self.step_counter += 1
        if self.counter < self.send_every:
            return False
        L = self.lists
        self.client.send((self.worker_id, ("loss",) + tuple(
            float(L[k].average) for k in CsvChannels.LOSS)))
        self.client.send((self.worker_id, ("other", float(L["active_relus"].average),
                                           float(self.dp_per_s.average))))
        if self.delays:
            d = np.asarray(self.delays, np.float64)
            self.client.send((self.worker_id, ("delays", (float(np.mean(d)), float(np.max(d)),
                                                          float(np.min(d))))))
        self.counter = 0
        for s in self.lists.values():
            s.reset()
        self.dp_per_s.reset()
        self.delays = []
        return True


class PpoMetrics(object):
    """The PPO channels of a StepMetrics, from the ratios a PoolTrainer's steps leave on the device.
    Per flushed batch of steps: ppo_clip_fraction = mean(|rho - 1| > clip), ppo_approx_kl =
    mean(-log rho) and, when the consumer normalises advantages, ppo_adv_mean / ppo_adv_std: the
    means of its {mean, std} over the flushed steps.
    ppo_epochs_run (with a target KL only) is not a per-step channel: it is the mean epochs per
    pool over the pools left since the last flush, and a pool is left after its last step's
    callback.  So flush_epochs writes it at every flush before which a pool was left, pending
    steps or not, and flush_steps never does; last_ppo carries the latest of both."""

    def __init__(self, clip, consumer, client=None):
        self.clip, self.consumer, self.client = clip, consumer, client
        self.ratios = []
        self.adv_stats = []
        self.pools_seen = 0
        self.epochs_run = None
        self.last_ppo = None

    def on_step(self, trainer):
        if trainer.model.ratio is not None:
            self.ratios.append(trainer.model.ratio.clone())
            if self.consumer.last_adv_stats is not None:
                self.adv_stats.append(self.consumer.last_adv_stats.clone())

    def flush_epochs(self):
        left = self.consumer.pool_epochs
        if not self.consumer.setting.target_kl > 0 or len(left) == self.pools_seen:
            return
        self.epochs_run = float(np.mean(left[self.pools_seen:]))
        self.pools_seen = len(left)
        if self.last_ppo is not None:
            self.last_ppo["ppo_epochs_run"] = self.epochs_run
        if self.client is not None:
            self.client.write_scalar("ppo_epochs_run", self.epochs_run)

    def flush_steps(self):
        if not self.ratios:
            return
        from . import ppo
        rho = torch.cat(self.ratios).cpu().numpy()
        self.ratios = []
        per_step = {"ppo_clip_fraction": ppo.clip_fraction(rho, self.clip),
                    "ppo_approx_kl": ppo.approx_kl(rho)}
        if self.adv_stats:
            m = torch.stack(self.adv_stats).cpu().numpy().mean(axis=0)
            self.adv_stats = []
            per_step.update(ppo_adv_mean=float(m[0]), ppo_adv_std=float(m[1]))
        if self.client is not None:
            for name, v in per_step.items():
                self.client.write_scalar(name, v)
        self.last_ppo = per_step
        if self.epochs_run is not None:
            self.last_ppo["ppo_epochs_run"] = self.epochs_run


class ScheduleMetrics(object):
    """The learning_rate and entropy_beta channels: each step's values (host numbers, as the step
    took them) are kept and one ('schedule', mean lr, mean beta) message is sent per flush, the
    means over the flushed steps, as the reference averages them.  last: the last step's values."""

    def __init__(self, client=None, worker_id=0):
        self.client, self.worker_id = client, worker_id
        self.values = []
        self.last = None

    def on_step(self, trainer):
        self.values.append((float(trainer.optimizer.learning_rate), float(trainer.model.entropy_beta)))

    def flush(self):
        if not self.values:
            return
        v = np.asarray(self.values, np.float64)
        self.values = []
        self.last = {"learning_rate": float(v[-1, 0]), "entropy_beta": float(v[-1, 1])}
        if self.client is not None:
            self.client.send((self.worker_id, ("schedule", float(v[:, 0].mean()),
                                               float(v[:, 1].mean()))))


class GradClipMetrics(object):
    """The channels of the global-norm clip (model_desc.ClipByGlobalNorm `proc`): each step's
    {norm, f} is cloned on the device (no host read per step); a flush writes grad_norm, the mean
    norm over the flushed steps, and grad_clip_fraction, the share of them with f < 1."""

    def __init__(self, proc, client=None):
        self.proc, self.client = proc, client
        self.stats = []
        self.last = None

    def on_step(self, trainer):
        if self.proc.last_stats is not None:
            self.stats.append(self.proc.last_stats.clone())

    def flush(self):
        if not self.stats:
            return
        v = torch.stack(self.stats).cpu().numpy()
        self.stats = []
        self.last = {"max_norm": self.proc.max_norm, "grad_norm": float(v[:, 0].mean()),
                     "clip_fraction": float((v[:, 1] < 1.0).mean())}
        if self.client is not None:
            self.client.write_scalar("grad_norm", self.last["grad_norm"])
            self.client.write_scalar("grad_clip_fraction", self.last["clip_fraction"])


class StepMetrics(object):
    """DebugLogCallback over device-resident step scalars: each learner step's 8 scalars are
    kept on the GPU and fetched once per `every` (--send_debug_every) steps (no per-step host
    sync).  ppo: a PpoMetrics fed and flushed along (None: off).  episodes: an
    episodes.EpisodeMetrics flushed after the fetch, when the host has synchronised (None: off).
    gradclip / schedule: a GradClipMetrics / ScheduleMetrics fed and flushed along (None: off)."""

    def __init__(self, trainer, batch_size, every, client, ppo=None, episodes=None, gradclip=None,
                 schedule=None):
        self.trainer, self.B, self.ppo, self.episodes = trainer, batch_size, ppo, episodes
        self.extra = [m for m in (gradclip, schedule) if m is not None]
        self.gradclip, self.schedule = gradclip, schedule
        self.every = max(1, int(every))
        self.cb = DebugLogCallback(client, worker_id=0, nr_send=self.every) if client else None
        self.pending = []
        self.t0 = time.time()
        self.last = None

    @property
    def last_ppo(self):
        return self.ppo.last_ppo if self.ppo is not None else None

    def __call__(self, trainer):
        self.pending.append(trainer.model.scalars.clone())
        if self.ppo is not None:
            self.ppo.on_step(trainer)
        for m in self.extra:
            m.on_step(trainer)
        if len(self.pending) >= self.every:
            self.flush()

    def flush(self):
        if self.ppo is not None:
            self.ppo.flush_epochs()
        if not self.pending:
            return
        from ._lib import SCALAR_NAMES
        vals = torch.stack(self.pending).cpu().numpy()
        self.trainer.check_device_errors()           # the host has synchronised anyway
        dt = time.time() - self.t0
        dp_per_s = len(self.pending) * self.B / max(dt, 1e-9)      # multigpu.py:307-313
        for row in vals:
            d = dict(zip(SCALAR_NAMES, row.tolist()))
            self.last = d
            if self.cb is not None:
                self.cb.trigger_step(d, dp_per_s)
        self.pending = []
        if self.ppo is not None:
            self.ppo.flush_steps()
        for m in self.extra:
            m.flush()
        if self.episodes is not None:
            self.episodes.flush()
        self.t0 = time.time()
