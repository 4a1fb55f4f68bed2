"""ba3c_episode_stats on the GPU: the kernel against episodes.update_numpy bit for bit, the log next
to the games' own ep_score, the two-player vector's +- pairs, the ActorLearner with and without a
log, and the launcher's --online_score."""
import json

import numpy as np
import pytest
import torch

from episode_host import HostLog
from oracle import ba3c_oracle as O

pytestmark = pytest.mark.gpu

LAUNCHES = 40
# the wave edge, the edge of a workgroup's 1024 threads, and the edge of one pass (kEpisodeChunk =
# 4096 simulators, ba3c_episodes.h) with a size of three passes: the wave totals' buffers alternate
SIZES = [1, 3, 37, 64, 65, 1024, 1025, 4096, 4097, 8200]


def crafted_rewards(rs, E):
    """Multiples of 0.1 of both signs, and 1e15 followed by 1.0 for a few simulators: after them an
    add of 0.1 rounds to the spacing of 1e15, so a sum kept in another order or width shows."""
    r = rs.randint(-30, 31, size=(LAUNCHES, E)) * 0.1
    r[2, ::7], r[3, ::7] = 1e15, 1.0
    return r


def _same(log, host):
    """Every buffer of the device log against the host statement's, bit for bit."""
    pairs = [(log.ret, host.ret), (log.len, host.len), (log.log_score, host.log_score),
             (log.log_len, host.log_len), (log.log_env, host.log_env)]
    for name, (dev, ref) in zip(("ret", "len", "log_score", "log_len", "log_env"), pairs):
        got = dev.cpu().numpy()
        assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), name
    assert int(log.head.item()) == host.head


@pytest.mark.parametrize("p_over,whole_ring", [(0.3, True), (0.3, False), (0.02, False)])
@pytest.mark.parametrize("E", SIZES)
def test_kernel_is_update_numpy_bit_for_bit(E, p_over, whole_ring):
    """cap == E: the ring wraps within a few launches; else the default cap."""
    from ba3c_amd.episodes import EpisodeLog, default_cap
    cap = E if whole_ring else default_cap(E)
    rs = np.random.RandomState(E + int(1000 * p_over))
    rewards = crafted_rewards(rs, E)
    overs = rs.random_sample((LAUNCHES, E)) < p_over
    log, host = EpisodeLog(E, cap=cap), HostLog(E, cap)
    dev_r = torch.from_numpy(rewards).cuda()
    dev_o = torch.from_numpy(overs).cuda()
    for t in range(LAUNCHES):
        log.update(dev_r[t], dev_o[t] if t % 2 else dev_o[t].view(torch.uint8))   # bool and uint8
        host.update(rewards[t], overs[t])
        if E <= 1025 or t % 8 == 7:
            _same(log, host)
    _same(log, host)
    assert host.head == int(overs.sum()) and (E < 64 or host.head > 0)
    if whole_ring and E > 1:
        assert host.head > cap                       # it did wrap


@pytest.mark.parametrize("E", [1, 65, 1025, 4097])
def test_every_flag_set_and_none(E):
    from ba3c_amd.episodes import EpisodeLog
    log, host = EpisodeLog(E, cap=E), HostLog(E, E)
    r = np.arange(E) * 0.3 - 7.0
    for flags in (np.zeros(E, bool), np.ones(E, bool), np.zeros(E, bool), np.ones(E, bool)):
        log.update(torch.from_numpy(r).cuda(), torch.from_numpy(flags).cuda())
        host.update(r, flags)
        _same(log, host)
    s, n, who, dropped = log.drain()
    assert dropped == E and who.tolist() == list(range(E)) and n.tolist() == [2] * E
    assert s.tobytes() == (r + r).tobytes()
    assert not np.signbit(log.ret.cpu().numpy()).any()       # +0.0 after an episode


def test_drain_reports_what_an_undrained_ring_lost():
    from ba3c_amd.episodes import EpisodeLog
    log = EpisodeLog(3, cap=4)
    one = torch.ones(3, dtype=torch.float64, device="cuda")
    every = torch.ones(3, dtype=torch.bool, device="cuda")
    assert log.drain()[0].size == 0
    for t in range(3):                               # 9 entries into 4 slots: scores 1, 2, 3
        log.update(one * (t + 1), every)
    s, n, who, dropped = log.drain()
    assert dropped == 5 and who.tolist() == [2, 0, 1, 2] and s.tolist() == [2.0, 3.0, 3.0, 3.0]
    assert log.drain()[3] == 0
    with pytest.raises(ValueError):
        log.update(one.float(), every)               # the environments' float64, nothing else
    with pytest.raises(ValueError):
        EpisodeLog(8, cap=7)


def _game_case(Vec, A, **skip):
    """100 random decisions of Vec(37, limit=40): per step the logged scores are the game's own
    ep_score of the finished episodes in index order, the lengths the decisions counted here."""
    from ba3c_amd.episodes import EpisodeLog
    E = 37
    vec = Vec(E, seed=3, limit=40, **skip)
    log = EpisodeLog(E)
    g = torch.Generator(device="cuda").manual_seed(5)
    decisions = np.zeros(E, np.int64)
    finished = 0
    for _ in range(100):
        vec.step(torch.randint(0, A, (E,), generator=g, device="cuda"))
        log.update(vec.reward, vec.last_over)
        decisions += 1
        over = vec.last_over.cpu().numpy()
        s, n, who, dropped = log.drain()
        assert dropped == 0 and who.tolist() == np.flatnonzero(over).tolist()
        assert s.tolist() == vec.ep_score.cpu().numpy()[over].astype(np.float64).tolist()
        assert n.tolist() == decisions[over].tolist()
        decisions[over] = 0
        finished += len(s)
    assert finished >= E                             # limit=40: every simulator finished at least once
    assert log.len.cpu().numpy().tolist() == decisions.tolist()


@pytest.mark.parametrize("skip", [{}, {"frame_skip": "2-4", "sticky": 0.25}], ids=["plain", "skip"])
def test_breakout_scores_are_the_games_own(skip):
    from ba3c_amd.breakout import BreakoutVec
    _game_case(BreakoutVec, 4, **skip)


@pytest.mark.parametrize("skip", [{}, {"frame_skip": "2-4", "sticky": 0.25}], ids=["plain", "skip"])
def test_boxing_scores_are_the_games_own(skip):
    from ba3c_amd.boxing import BoxingVec
    _game_case(BoxingVec, 18, **skip)


def test_the_two_sides_of_a_duel_log_opposite_scores():
    from ba3c_amd.duel import BoxingDuelDecisionVec, start_from_gap
    from ba3c_amd.episodes import EpisodeLog
    G = 5
    vec = BoxingDuelDecisionVec(G, seed=1, limit=30, frame_skip="2-4", sticky=0.25,
                                start=start_from_gap("8-14"))
    log = EpisodeLog(2 * G)
    g = torch.Generator(device="cuda").manual_seed(9)
    for _ in range(60):
        vec.step(torch.randint(0, 18, (2 * G,), generator=g, device="cuda"))
        log.update(vec.reward, vec.last_over)
    s, n, who, dropped = log.drain()
    assert dropped == 0 and len(s) >= 2 * G and len(s) % 2 == 0
    entries = {}
    for i, (score, length, e) in enumerate(zip(s.tolist(), n.tolist(), who.tolist())):
        entries.setdefault(e, []).append((score, length, i))
    for game in range(G):
        a, b = entries[game], entries[G + game]      # player p of game g is simulator p * G + g
        assert len(a) == len(b) >= 1
        for (sa, la, _), (sb, lb, _) in zip(a, b):
            assert sa == -sb and la == lb


def _loop(episodes, E=8, B=8):
    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    m = Model(num_actions=4, fc_neurons=128, fc_splits=4, batch_size=B, max_batch=max(B, E))
    m.engine.load_params(O.init_params(128, 4, 4, seed=0, dtype=np.float32))
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    return ActorLearner(tr, n_envs=E, batch_size=B, seed=1, episodes=episodes), tr, m


def test_actor_learner_with_a_log_trains_the_same_and_logs_the_replay():
    from ba3c_amd.episodes import EpisodeLog
    E = 8
    plain, tr0, m0 = _loop(None)
    plain.run(100)
    log = EpisodeLog(E)
    logged, tr1, m1 = _loop(log)
    seen = []
    step = logged.env.step

    def tapped(actions):                             # SyntheticAtari: the unfused path
        frames, reward, over = step(actions)
        seen.append((reward.cpu().numpy().copy(), over.cpu().numpy().copy()))
        return frames, reward, over
    logged.env.step = tapped
    logged.run(100)
    torch.cuda.synchronize()
    assert tr0.global_step == tr1.global_step >= 50
    assert torch.equal(m0.engine.params.view(torch.int32), m1.engine.params.view(torch.int32))

    host = HostLog(E, log.cap)
    for reward, over in seen:
        host.update(reward, over)
    assert len(seen) == 100 and host.head >= E       # episodes last 20..80 steps
    s, n, who, dropped = log.drain()
    hs, hn, hwho, _ = host.drain()
    assert dropped == 0 and s.tobytes() == hs.tobytes()
    assert n.tolist() == hn.tolist() and who.tolist() == hwho.tolist()
    assert all(20 <= k <= 80 for k in n.tolist())


def test_a_games_fused_step_feeds_the_log_too():
    """step_into (the fused path): the loop's log is the game's own ep_score."""
    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.breakout import BreakoutVec
    from ba3c_amd.episodes import EpisodeLog
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    E, B = 8, 8
    m = Model(num_actions=4, fc_neurons=128, fc_splits=4, batch_size=B, max_batch=B)
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    log, vec = EpisodeLog(E), BreakoutVec(E, seed=0, limit=10)
    loop = ActorLearner(tr, n_envs=E, batch_size=B, seed=0, env=vec, episodes=log)
    want = []
    for _ in range(25):
        loop.iterate()
        over = vec.last_over.cpu().numpy()
        want += vec.ep_score.cpu().numpy()[over].astype(np.float64).tolist()
    s, n, who, dropped = log.drain()
    assert len(want) >= 2 * E and s.tolist() == want and set(n.tolist()) <= set(range(1, 11))
    with pytest.raises(ValueError):
        ActorLearner(tr, n_envs=E, batch_size=B, episodes=EpisodeLog(E + 1))


ARGV = ("-o adam -l 0.001 -b 8 --fc_neurons 128 --fc_splits 4 --epsilon 1e-8 --beta1 0.8 "
        "--beta2 0.75 --simulator_procs 8 --max_steps 90 --send_debug_every 5").split()


def test_launcher_writes_online_score(tmp_path, monkeypatch, capsys):
    from ba3c_amd import episodes as EP
    from ba3c_amd.train import main
    logs, base = [], EP.EpisodeLog

    class Kept(base):
        def __init__(self, *a, **k):
            base.__init__(self, *a, **k)
            logs.append(self)
    monkeypatch.setattr(EP, "EpisodeLog", Kept)
    out = main(ARGV + ["--online_score", "2", "--experiment_dir", str(tmp_path / "on")])
    line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
    ep = out["episodes"]
    assert line["episodes"] == ep
    assert set(ep) == {"count", "score_mean", "score_max", "score_min", "length_mean", "dropped",
                       "online_score_last"}
    assert len(logs) == 1 and ep["count"] == int(logs[0].head.item()) >= 4 and ep["dropped"] == 0
    rows = (tmp_path / "on" / "online_score.csv").read_text().strip().split("\n")
    assert rows[0] == "x,y" and len(rows) - 1 == ep["count"] // 2
    assert float(rows[-1].split(",")[1]) == ep["online_score_last"]
    assert ep["score_min"] <= ep["score_mean"] <= ep["score_max"] and 20 <= ep["length_mean"] <= 80
    counted = (tmp_path / "on" / "train_episodes.csv").read_text().strip().split("\n")[1:]
    assert sum(int(r.split(",")[1]) for r in counted) == ep["count"]
    for name in ("train_score_mean", "train_score_max", "train_episode_length"):
        assert len((tmp_path / "on" / (name + ".csv")).read_text().strip().split("\n")) == len(counted) + 1

    off = main(ARGV + ["--experiment_dir", str(tmp_path / "off")])
    assert "episodes" not in off and len(logs) == 1
    assert "episodes" not in json.loads(capsys.readouterr().out.strip().split("\n")[-1])
    written = sorted(p.name for p in (tmp_path / "off").iterdir())
    assert "online_score.csv" not in written and not [w for w in written if w.startswith("train_")]
    assert sorted(p.name for p in (tmp_path / "on").iterdir()) == sorted(
        written + ["online_score.csv", "train_episode_length.csv", "train_episodes.csv",
                   "train_score_max.csv", "train_score_mean.csv"])
    assert off["global_step"] == out["global_step"] and off["last"] == out["last"]
