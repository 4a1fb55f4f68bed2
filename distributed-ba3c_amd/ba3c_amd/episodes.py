"""The episodes the training simulators finish (`--online_score`), once: the rules, their log on
the device and the channels made of it.

MySimulatorMaster keeps a reward sum per simulator (`self.stats[ident]`, OpenAIGym/train.py:394-412),
feeds it to `self.games` at every episode end and sends `('online', self.games.average)` every 10
finished games.  Here every simulator's sum and length live on the GPU and one launch per actor
iteration (`ba3c_episode_stats`) advances them all; the finished episodes go to a ring that the
host drains where it synchronises anyway.  One launch, for every simulator e in [0, E):

    ret[e] = ret[e] + reward[e]          # float64, one rounding; the RAW reward, not the clipped one
    len[e] = len[e] + 1
    if over[e]:
        k = number of e' < e with over[e'] in THIS launch
        slot = (head + k) mod cap
        log_score[slot], log_len[slot], log_env[slot] = ret[e], len[e], e
        ret[e] = +0.0; len[e] = 0
    head = head + (number of e with over[e])

The episodes of one launch are logged in increasing e; `online_score` averages consecutive groups,
so that order is part of the rules.  The reward of the step that ends an episode counts towards it
(the games' own `ep_score` counts it too); the reference's `_on_episode_over` leaves that last
reward out of `stats[ident]`.

`update_numpy` is that statement and the kernel's bit-exact oracle; `EpisodeLog` holds the device
buffers; `OnlineScore` is `self.games`; `Summary` the whole run's figures; `EpisodeMetrics` couples
the three for `metrics.StepMetrics`.
"""
import ctypes

import numpy as np

ONLINE_EVERY = 10         # train.py:402
MIN_CAP = 1024


def default_cap(n_envs):
    return max(4 * int(n_envs), MIN_CAP)


def update_numpy(ret, length, reward, over, log_score, log_len, log_env, head):
    """The statement above, in place: ret float64 [E], length int32 [E], the three rings
    (float64 / int32 / int32 [cap], cap >= E); reward float64 [E], over [E].  Returns the new head."""
    E, cap = len(ret), len(log_score)
    assert ret.dtype == np.float64 and log_score.dtype == np.float64
    assert length.dtype == np.int32 and log_len.dtype == np.int32 and log_env.dtype == np.int32
    assert len(length) == len(reward) == len(over) == E and len(log_len) == len(log_env) == cap
    assert 1 <= E <= cap
    reward = np.asarray(reward, dtype=np.float64)
    head = int(head)
    k = 0
    for e in range(E):
        ret[e] = ret[e] + reward[e]
        length[e] = length[e] + 1
        if over[e]:
            slot = (head + k) % cap
            log_score[slot], log_len[slot], log_env[slot] = ret[e], length[e], e
            ret[e] = 0.0
            length[e] = 0
            k += 1
    return head + k


def ring_window(head, seen, cap):
    """What a drain at `head` returns after one at `seen`: (ring slots oldest first, dropped)."""
    n = head - seen
    dropped = max(n - cap, 0)
    return [i % cap for i in range(head - (n - dropped), head)], dropped


class EpisodeLog(object):
    """The device buffers of the statement above for n_envs simulators and a ring of `cap` entries
    (default max(4 * n_envs, 1024)).  update() is one launch and no host read; drain() reads
    `head` once."""

    def __init__(self, n_envs, cap=None, device="cuda"):
        import torch

        from . import _lib
        self.E = int(n_envs)
        self.cap = default_cap(self.E) if cap is None else int(cap)
        if self.E < 1 or self.cap < self.E:
            raise ValueError("an episode log needs n_envs >= 1 and cap >= n_envs, got %d and %d"
                             % (self.E, self.cap))
        self.lib = _lib.load()
        self._check = _lib.check
        self._torch = torch
        self.device = dev = torch.device(device)
        self.ret = torch.zeros(self.E, dtype=torch.float64, device=dev)
        self.len = torch.zeros(self.E, dtype=torch.int32, device=dev)
        self.log_score = torch.zeros(self.cap, dtype=torch.float64, device=dev)
        self.log_len = torch.zeros(self.cap, dtype=torch.int32, device=dev)
        self.log_env = torch.zeros(self.cap, dtype=torch.int32, device=dev)
        self.head = torch.zeros(1, dtype=torch.int64, device=dev)
        self.seen = 0                      # the head of the last drain

    def update(self, reward, over):
        """reward: the float64 [E] tensor the environments produce; over: bool or uint8 [E]."""
        torch = self._torch
        if reward.dtype != torch.float64 or reward.shape != (self.E,) or not reward.is_contiguous():
            raise ValueError("reward must be a contiguous float64 [%d] tensor" % self.E)
        if over.dtype == torch.bool:
            over = over.view(torch.uint8)
        if over.dtype != torch.uint8 or over.shape != (self.E,) or not over.is_contiguous():
            raise ValueError("over must be a contiguous bool or uint8 [%d] tensor" % self.E)
        if reward.device != self.ret.device or over.device != self.ret.device:
            raise ValueError("reward and over must be on %s" % self.ret.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        self._check(self.lib.ba3c_episode_stats(
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(reward), p(over), self.E,
            p(self.ret), p(self.len), p(self.log_score), p(self.log_len), p(self.log_env), self.cap,
            p(self.head)))

    def drain(self):
        """-> (scores float64 [n], lengths int32 [n], envs int32 [n], dropped): the entries logged
        since the last drain, oldest first; when more than cap arrived only the newest cap, and
        `dropped` counts the lost ones."""
        head = int(self.head.item())       # the one synchronisation
        slots, dropped = ring_window(head, self.seen, self.cap)
        self.seen = head
        if not slots:
            return (np.zeros(0, np.float64), np.zeros(0, np.int32), np.zeros(0, np.int32), dropped)
        idx = self._torch.as_tensor(slots, dtype=self._torch.int64, device=self.device)
        return (self.log_score[idx].cpu().numpy(), self.log_len[idx].cpu().numpy(),
                self.log_env[idx].cpu().numpy(), dropped)


class OnlineScore(object):
    """`self.games` (train.py:399-404): the mean of every `every` consecutive finished episodes."""

    def __init__(self, every=ONLINE_EVERY):
        self.every = int(every)
        if self.every < 1:
            raise ValueError("OnlineScore averages groups of at least one episode")
        self._games = []

    def feed(self, scores):
        """-> the np.mean of each group completed by `scores`; a partial group waits."""
        out = []
        for s in scores:
            self._games.append(float(s))
            if len(self._games) == self.every:
                out.append(float(np.mean(self._games)))
                self._games = []
        return out


class Summary(object):
    """A whole run's episodes: count, score mean / max / min, mean length, dropped."""

    def __init__(self):
        self.count = self.dropped = 0
        self._score = self._length = 0.0
        self.score_max = self.score_min = None

    def feed(self, scores, lengths, dropped=0):
        self.dropped += int(dropped)
        if len(scores) == 0:
            return
        self.count += len(scores)
        self._score += float(np.sum(scores))
        self._length += float(np.sum(lengths))
        hi, lo = float(np.max(scores)), float(np.min(scores))
        self.score_max = hi if self.score_max is None else max(self.score_max, hi)
        self.score_min = lo if self.score_min is None else min(self.score_min, lo)

    def as_dict(self):
        n = self.count
        return {"count": n, "score_mean": self._score / n if n else None,
                "score_max": self.score_max, "score_min": self.score_min,
                "length_mean": self._length / n if n else None, "dropped": self.dropped}


class EpisodeMetrics(object):
    """The episode channels of a StepMetrics: a log, an OnlineScore over it and the run's Summary.
    flush() drains the log (call it where the host has synchronised) and, with a client, sends one
    (0, ('online', mean)) per complete group and, when an episode finished since the last flush,
    writes train_score_mean / train_score_max / train_episode_length / train_episodes over the
    drained entries.  Without a client (ranks above 0) it still drains and keeps the summary."""

    def __init__(self, log, every=ONLINE_EVERY, client=None):
        self.log, self.client = log, client
        self.online = OnlineScore(every)
        self.summary = Summary()
        self.online_score_last = None

    def flush(self):
        scores, lengths, _, dropped = self.log.drain()
        self.summary.feed(scores, lengths, dropped)
        for mean in self.online.feed(scores):
            self.online_score_last = mean
            if self.client is not None:
                self.client.send((0, ("online", mean)))
        if len(scores) and self.client is not None:
            w = self.client.write_scalar
            w("train_score_mean", float(np.mean(scores)))
            w("train_score_max", float(np.max(scores)))
            w("train_episode_length", float(np.mean(lengths)))
            w("train_episodes", len(scores))

    def as_dict(self):
        return dict(self.summary.as_dict(), online_score_last=self.online_score_last)
