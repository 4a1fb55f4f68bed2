"""The rules of the training simulators' episode log (ba3c_amd.episodes), on the host:
update_numpy against a scalar mirror of the reference's bookkeeping, the ring, OnlineScore, the
--online_score flag and the channels a StepMetrics flush writes."""
import numpy as np
import pytest
import torch

from ba3c_amd import episodes as EP
from episode_host import HostLog, MasterMirror


def crafted_rewards(rs, steps, E):
    """Multiples of 0.1 of both signs; simulator 0 (and E - 1) also sees 1e15 followed by 1.0, after
    which an add of 0.1 rounds to the spacing of 1e15 (0.125): per-add rounding shows."""
    r = rs.randint(-30, 31, size=(steps, E)) * 0.1
    r[2, 0], r[3, 0] = 1e15, 1.0
    r[5, E - 1], r[6, E - 1] = 1e15, 1.0
    return r


@pytest.mark.parametrize("E,cap", [(1, 1), (5, 5), (7, 16), (64, 64), (65, 1024)])
def test_update_numpy_is_the_reference_bookkeeping(E, cap):
    rs = np.random.RandomState(E)
    steps = 60
    rewards = crafted_rewards(rs, steps, E)
    overs = rs.random_sample((steps, E)) < 0.1
    overs[:5, 0] = False                   # the 1e15 episode lasts long enough to show rounding
    mirror, log = MasterMirror(), HostLog(E, cap)
    got = []
    for t in range(steps):
        for e in range(E):
            mirror.on_message(e, rewards[t, e], overs[t, e])
        log.update(rewards[t], overs[t])
        s, n, who, dropped = log.drain()
        assert dropped == 0                # drained every launch and cap >= E
        got += list(zip(s.tolist(), n.tolist(), who.tolist()))
    assert len(got) == int(overs.sum()) == log.head
    assert [g[1:] for g in got] == [m[1:] for m in mirror.games]
    # bit for bit: the same float64 adds in the same order
    assert np.array([g[0] for g in got]).tobytes() == np.array([m[0] for m in mirror.games]).tobytes()
    big = [g[0] for g in got if g[0] > 1e14]
    assert big and any(b != 1e15 + 1.0 for b in big)
    # what is left is the running episodes
    for e in range(E):
        assert log.len[e] == len(mirror.stats.get(e, []))


def test_a_finished_episode_leaves_plus_zero():
    log = HostLog(2, 2)
    log.update(np.array([-1.5, 2.0]), np.array([True, False]))
    assert log.ret.tobytes() == np.array([0.0, 2.0]).tobytes() and list(log.len) == [0, 1]
    assert not np.signbit(log.ret[0])


def test_ring_wraps_at_cap_equal_to_the_simulators():
    E = 4
    log = HostLog(E, E)
    one = np.ones(E)
    log.update(one, np.array([0, 1, 0, 1], bool))        # slots 0, 1
    log.update(one, np.array([1, 0, 0, 0], bool))        # slot 2
    assert log.drain()[2].tolist() == [1, 3, 0]
    log.update(one, np.array([0, 1, 1, 1], bool))        # slots 3, 0, 1: wraps
    assert log.head == 6
    assert log.log_env.tolist() == [2, 3, 0, 1]
    s, n, who, dropped = log.drain()
    assert (who.tolist(), s.tolist(), n.tolist(), dropped) == ([1, 2, 3], [2.0, 3.0, 2.0], [2, 3, 2], 0)


def test_all_over_at_once_and_none_over():
    E = 6
    log = HostLog(E, E)
    r = np.arange(E) * 0.5
    log.update(r, np.zeros(E, bool))
    assert log.head == 0 and log.drain()[0].size == 0 and log.len.tolist() == [1] * E
    log.update(r, np.ones(E, bool))
    assert log.head == E
    s, n, who, dropped = log.drain()
    assert who.tolist() == list(range(E)) and s.tolist() == (2 * r).tolist() and n.tolist() == [2] * E
    assert dropped == 0 and not log.ret.any() and not log.len.any()
    log.update(r, np.ones(E, bool))                      # a full ring overwritten in place, in order
    assert log.drain()[0].tolist() == r.tolist()


def test_an_undrained_overflow_counts_the_dropped():
    E = 3
    log = HostLog(E, E)
    for t in range(4):                                   # 4 * 3 = 12 entries into 3 slots
        log.update(np.full(E, float(t)), np.ones(E, bool))
    s, n, who, dropped = log.drain()
    assert dropped == 9 and s.tolist() == [3.0] * 3 and who.tolist() == [0, 1, 2]
    assert log.drain()[3] == 0 and log.drain()[0].size == 0
    log.update(np.ones(E), np.array([0, 1, 0], bool))
    log.update(np.ones(E), np.ones(E, bool))             # 4 entries since the drain, 3 kept
    s, n, who, dropped = log.drain()
    assert dropped == 1 and who.tolist() == [0, 1, 2] and s.tolist() == [2.0, 1.0, 2.0]


def test_default_cap():
    assert EP.default_cap(100) == 1024 and EP.default_cap(256) == 1024 and EP.default_cap(4096) == 16384


def test_online_score_carries_a_partial_group():
    o = EP.OnlineScore(every=3)
    assert o.feed([1.0, 2.0]) == []
    assert o.feed([6.0, 10.0]) == [3.0]
    assert o.feed([]) == []
    assert o.feed([20.0, 30.0, 1.0, 1.0, 1.0, 5.0]) == [20.0, 1.0]
    assert o.feed([5.0, 5.0]) == [5.0]
    assert EP.OnlineScore().every == 10                  # the reference's


def test_online_score_of_every_episode():
    o = EP.OnlineScore(every=1)
    assert o.feed([4.0, -2.5]) == [4.0, -2.5] and o.feed([]) == [] and o.feed([7.0]) == [7.0]
    with pytest.raises(ValueError):
        EP.OnlineScore(every=0)


def test_summary():
    s = EP.Summary()
    assert s.as_dict() == {"count": 0, "score_mean": None, "score_max": None, "score_min": None,
                           "length_mean": None, "dropped": 0}
    s.feed(np.array([1.0, -3.0]), np.array([10, 20], np.int32))
    s.feed(np.zeros(0), np.zeros(0, np.int32), dropped=2)
    s.feed(np.array([8.0]), np.array([30], np.int32))
    assert s.as_dict() == {"count": 3, "score_mean": 2.0, "score_max": 8.0, "score_min": -3.0,
                           "length_mean": 20.0, "dropped": 2}


def _resolve(argv):
    from ba3c_amd.flags import build_parser, resolve
    return resolve(build_parser().parse_args(argv))


def test_flag():
    assert _resolve([]).online_score == 0
    assert _resolve(["--online_score", "10"]).online_score == 10
    assert _resolve(["--online_score", "2", "-e", "GridBoxing-v0", "--num_actions", "18",
                     "--self_play", "--ppo_clip", "0.2"]).online_score == 2
    with pytest.raises(SystemExit) as e:
        _resolve(["--online_score", "10", "--dummy", "1"])
    assert "--dummy" in str(e.value)
    with pytest.raises(SystemExit) as e:
        _resolve(["--online_score", "-1"])
    assert "--online_score" in str(e.value) and ">= 0" in str(e.value)
    assert _resolve(["--dummy", "1"]).online_score == 0   # --dummy alone is as it was


class FakeClient(object):
    def __init__(self):
        self.events = []

    def send(self, message):
        self.events.append(("send", message))

    def write_scalar(self, name, value):
        self.events.append(("scalar", name, value))


class FakeTrainer(object):
    class model(object):
        scalars = torch.zeros(8)

    def check_device_errors(self):
        pass


def _episode_events(client):
    names = ("train_score_mean", "train_score_max", "train_episode_length", "train_episodes")
    return [ev for ev in client.events
            if (ev[0] == "send" and ev[1][1][0] == "online") or (ev[0] == "scalar" and ev[1] in names)]


def test_a_flush_sends_the_online_groups_in_order_and_the_four_scalars():
    from ba3c_amd.metrics import StepMetrics
    client, log = FakeClient(), HostLog(4, 8)
    em = EP.EpisodeMetrics(log, every=2, client=client)
    sm = StepMetrics(FakeTrainer(), batch_size=8, every=1, client=client, episodes=em)

    log.update(np.array([1.0, 2.0, 3.0, 4.0]), np.zeros(4, bool))
    sm(FakeTrainer())                                    # flushes: no episode finished
    assert _episode_events(client) == [] and em.as_dict()["count"] == 0
    assert any(ev[0] == "send" and ev[1][1][0] == "loss" for ev in client.events)

    log.update(np.array([1.0, 2.0, 3.0, 4.0]), np.array([1, 1, 1, 0], bool))   # scores 2, 4, 6
    log.update(np.array([0.5, 0.5, 0.5, 0.5]), np.array([0, 0, 1, 1], bool))   # scores .5, 8.5
    sm(FakeTrainer())
    assert _episode_events(client) == [
        ("send", (0, ("online", 3.0))), ("send", (0, ("online", 3.25))),
        ("scalar", "train_score_mean", 4.2), ("scalar", "train_score_max", 8.5),
        ("scalar", "train_episode_length", 2.0), ("scalar", "train_episodes", 5)]
    del client.events[:]

    log.update(np.array([1.0, 0.0, 0.0, 0.0]), np.array([1, 0, 0, 0], bool))   # completes (8.5, 1.5)
    sm(FakeTrainer())
    assert _episode_events(client)[0] == ("send", (0, ("online", 5.0)))
    assert em.as_dict() == {"count": 6, "score_mean": 22.5 / 6, "score_max": 8.5, "score_min": 0.5,
                            "length_mean": 2.0, "dropped": 0, "online_score_last": 5.0}


def test_without_a_client_a_flush_still_drains():
    from ba3c_amd.metrics import StepMetrics
    log = HostLog(2, 2)
    em = EP.EpisodeMetrics(log, every=1, client=None)
    sm = StepMetrics(FakeTrainer(), batch_size=8, every=1, client=None, episodes=em)
    log.update(np.array([1.0, 5.0]), np.ones(2, bool))
    sm(FakeTrainer())
    assert log.seen == 2 and em.as_dict()["count"] == 2 and em.online_score_last == 5.0


def test_online_messages_reach_the_online_score_channel(tmp_path):
    from ba3c_amd.metrics import CsvChannels
    client, log = CsvChannels(str(tmp_path)), HostLog(3, 3)
    em = EP.EpisodeMetrics(log, every=2, client=client)
    log.update(np.array([1.0, 2.0, 4.0]), np.ones(3, bool))
    em.flush()
    client.close()
    rows = (tmp_path / "online_score.csv").read_text().strip().split("\n")
    assert rows[0] == "x,y" and len(rows) == 2 and float(rows[1].split(",")[1]) == 1.5
    assert (tmp_path / "train_episodes.csv").read_text().strip().split("\n")[1].endswith(",3")
