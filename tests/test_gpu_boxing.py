"""GridBoxing on the MI355X: the fused step + render + history-push kernel (ba3c_boxing_step /
ba3c_boxing_render) equals the CPU statement of the rules (ba3c_amd.boxing.step_numpy /
render_numpy) bit for bit, the fused history push equals ba3c_history_push, and the game runs
through the actor-learner loop with an 18-way policy, the launcher and the evaluator.  No test
asserts that the agent learns and none asserts a time."""
import numpy as np
import pytest
import torch

from boxing_policy import PUNCH, QUIET, history_push_numpy, make_row, player_from_row, trajectory
from loop_mirror import LoopMirror
from oracle import ba3c_oracle as O

pytestmark = pytest.mark.gpu


def _env_and_hist(E, seed, limit):
    from ba3c_amd.boxing import BoxingVec
    from ba3c_amd.rollout import FrameHistory
    env = BoxingVec(E, seed=seed, limit=limit)
    hist = FrameHistory(E, hist_len=4, channels=1)
    env.reset_history(hist)
    return env, hist


def _state_ref(K, tr, s):
    """HistoryFramePlayer's state after step s (s = -1: the initial state) from the recorded
    rows: channel 3 is the frame after step s, channel 3-k the frame k steps earlier unless an
    episode ended since (or the run is younger than that)."""
    E = tr.games.shape[1]
    st = np.zeros((E, 84, 84, 4), np.uint8)
    live = np.ones(E, bool)
    for k in range(4):
        if s + 1 - k < 0:
            break
        st[live, :, :, 3 - k] = K.render_numpy(tr.games[s + 1 - k])[live]
        if s - k < 0:
            break
        live = live & ~tr.over[s - k]
    return st


def _check_against_oracle(env, hist, tr, every=1):
    """Replay tr.actions on the device, one launch per step writing BOTH frame and state, and
    compare everything the kernel writes with the CPU statement of the rules."""
    from ba3c_amd import boxing as K
    E = env.E
    assert (env.game.cpu().numpy() == tr.games[0]).all()
    assert (env.frames().cpu().numpy()[..., 0] == K.render_numpy(tr.games[0])).all()
    state = _state_ref(K, tr, -1)
    assert (hist.state.cpu().numpy() == state).all()
    ep = torch.full((E,), -777, dtype=torch.int32, device=env.device)
    env.ep_score = ep
    for s in range(tr.actions.shape[0]):
        ep.fill_(-777)
        reward, over = env._step(torch.from_numpy(tr.actions[s].copy()).cuda(), env.frame, hist.state)
        assert (env.game.cpu().numpy() == tr.games[s + 1]).all(), s
        assert reward.dtype == torch.float64 and (reward.cpu().numpy() == tr.reward[s]).all(), s
        assert (over.cpu().numpy() == tr.over[s]).all(), s
        # ep_score: the finished episode's score where over, untouched elsewhere
        assert (ep.cpu().numpy() == np.where(tr.over[s], tr.ep_score[s], -777)).all(), s
        if every == 1:
            frames = K.render_numpy(tr.games[s + 1])
            state = history_push_numpy(state, frames, tr.over[s])
        elif s % every == every - 1:
            frames = K.render_numpy(tr.games[s + 1])
            state = _state_ref(K, tr, s)
        else:
            continue
        assert (env.frame.cpu().numpy()[..., 0] == frames).all(), s
        assert (hist.state.cpu().numpy() == state).all(), s


@pytest.mark.parametrize("E,steps,limit,seed,every", [(1, 400, 150, 1, 1), (37, 1200, 400, 2, 1),
                                                      (300, 200, 150, 1, 10)])
def test_kernel_equals_the_cpu_rules_bit_for_bit(E, steps, limit, seed, every):
    tr = trajectory(E, steps, limit, seed, E == 37)
    if E == 37:
        # the CPU player's own event log (not the kernel's output) shows what the run covered
        missing = [n for n in ("hit1", "hit2", "miss", "got1", "got2", "over_limit") if tr.events[n] == 0]
        assert not missing, (missing, tr.events)
        assert set(np.unique(tr.actions).tolist()) == set(range(18))
    assert tr.over.any() and (tr.reward > 0).any() and (tr.reward < 0).any()
    env, hist = _env_and_hist(E, seed, limit)
    _check_against_oracle(env, hist, tr, every)


def test_crafted_rows_cover_knock_outs_clock_corners_and_clamped_knock_backs():
    """Rows written into the game tensor, each compared with the oracle and with BoxingPlayer:
    a knock-out win and loss one punch away, the clock at t = 1679, the agent in all four
    corners pushing outwards, and a knock-back into either rope for either boxer."""
    from ba3c_amd import boxing as K
    q, p = dict(rng=QUIET), dict(rng=PUNCH)      # the first step's draw: no wander; no punch / punch
    rows = np.stack([
        make_row(ax=40, ox=49, a_score=99, o_score=37, t=500, **q),        # 0: FIRE wins
        make_row(ax=40, ox=49, a_score=10, o_score=99, t=500, **p),        # 1: NOOP loses
        make_row(a_score=5, o_score=3, t=1679, **q),                       # 2: clock
        make_row(ax=4, ay=14, ox=40, oy=60, **q), make_row(ax=74, ay=14, ox=40, oy=60, **q),
        make_row(ax=4, ay=70, ox=40, oy=20, **q), make_row(ax=74, ay=70, ox=40, oy=20, **q),  # 3..6
        make_row(ax=63, ox=73, **q), make_row(ax=15, ox=5, **q),           # 7, 8: ox clamped
        make_row(ax=5, ox=15, **p), make_row(ax=73, ox=63, **p),           # 9, 10: ax clamped
    ]).astype(np.int32)
    first = np.array([1, 0, 0, 7, 6, 9, 8, 1, 1, 0, 0], np.int64)          # 7 UPLEFT .. 8 DOWNRIGHT
    E, steps, limit = rows.shape[0], 40, 2000
    players = [player_from_row(r, limit=limit) for r in rows]
    env, hist = _env_and_hist(E, 0, limit)
    env.game.copy_(torch.from_numpy(rows))
    env.reset_history(hist)
    game = rows.copy()
    state = np.zeros((E, 84, 84, 4), np.uint8)
    state[..., 3] = K.render_numpy(game)
    assert (hist.state.cpu().numpy() == state).all()
    seen = set()
    rs = np.random.RandomState(0)
    for s in range(steps):
        a = first if s == 0 else rs.randint(18, size=E).astype(np.int64)
        reward, over, ep = K.step_numpy(game, a, limit)
        for e, p in enumerate(players):
            assert p.action(int(a[e])) == (reward[e], bool(over[e])) and p.game_row() == game[e].tolist()
            seen |= {(e, n) for n in p.last_events}
        if s == 0:                               # the CPU side met what the rows were crafted for
            assert seen == {(0, "hit2"), (0, "ko_win"), (1, "got2"), (1, "ko_loss"), (2, "over_clock"),
                            (7, "hit1"), (8, "hit1"), (9, "got1"), (10, "got1")}
            assert over.tolist() == [True] * 3 + [False] * 8 and ep[:3].tolist() == [101 - 37, 10 - 101, 2]
            assert game[3:7, :2].tolist() == [[4, 14], [74, 14], [4, 70], [74, 70]]
            assert game[7:11, [0, 2]].tolist() == [[63, 74], [15, 4], [4, 15], [74, 63]]
        g_reward, g_over = env._step(torch.from_numpy(a).cuda(), env.frame, hist.state)
        assert (env.game.cpu().numpy() == game).all(), s
        assert (g_reward.cpu().numpy() == reward).all() and (g_over.cpu().numpy() == over).all(), s
        assert (env.ep_score.cpu().numpy()[over] == ep[over]).all(), s
        frames = K.render_numpy(game)
        state = history_push_numpy(state, frames, over)
        assert (env.frame.cpu().numpy()[..., 0] == frames).all(), s
        assert (hist.state.cpu().numpy() == state).all(), s
    assert {n for _, n in seen} >= {"hit1", "hit2", "miss", "got1", "got2"}


def test_fused_push_equals_step_then_history_push():
    E, steps, limit, seed = 37, 60, 20, 5
    tr = trajectory(E, steps, limit, seed)
    assert tr.over.sum() >= 2 * E
    fused, hist_f = _env_and_hist(E, seed, limit)
    plain, hist_p = _env_and_hist(E, seed, limit)
    assert torch.equal(hist_f.state, hist_p.state) and hist_f.state.any()
    for s in range(steps):
        a = torch.from_numpy(tr.actions[s].copy()).cuda()
        r_f, o_f = fused.step_into(a, hist_f)
        frames, r_p, o_p = plain.step(a)
        hist_p.push(frames, o_p)                                  # ba3c_history_push
        assert torch.equal(hist_f.state, hist_p.state), s
        assert torch.equal(fused.game, plain.game) and torch.equal(r_f, r_p) and torch.equal(o_f, o_p)
    assert (fused.game.cpu().numpy() == tr.games[-1]).all()


def test_actions_outside_the_18_are_noop():
    """int64 actions outside [0, 18) are NOOP: same rows, frames and rewards as action 0."""
    E, steps, limit, seed = 8, 80, 60, 7
    odd = np.array([18, -1, (1 << 32) + 1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 1 << 40,
                    -(1 << 62), (1 << 32) + 17], np.int64)        # low dword 1 / 17 fire if truncated
    weird, hist_w = _env_and_hist(E, seed, limit)
    noop, hist_n = _env_and_hist(E, seed, limit)
    rs = np.random.RandomState(seed)
    for s in range(steps):
        legal = rs.randint(18, size=E).astype(np.int64)
        use_odd = rs.random_sample(E) < 0.5
        a_w = np.where(use_odd, np.roll(odd, s), legal)
        a_n = np.where(use_odd, 0, legal)
        r_w, o_w = weird.step_into(torch.from_numpy(a_w).cuda(), hist_w)
        r_n, o_n = noop.step_into(torch.from_numpy(a_n).cuda(), hist_n)
        assert torch.equal(weird.game, noop.game) and torch.equal(r_w, r_n) and torch.equal(o_w, o_n), s
        assert torch.equal(hist_w.state, hist_n.state), s
    assert int(noop.game[:, 8].max()) > 0                         # t ran


def test_actor_learner_on_boxing_samples_18_actions_and_feeds_the_reference_datapoints():
    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.boxing import BoxingVec
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    E, B, A = 24, 32, 18
    m = Model(num_actions=A, fc_neurons=128, fc_splits=4, batch_size=B, max_batch=max(B, E))
    m.engine.load_params(O.init_params(128, 4, A, seed=0, dtype=np.float32))
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    p0 = m.engine.params.clone()
    env = BoxingVec(E, seed=1, limit=25)
    loop = ActorLearner(tr, n_envs=E, batch_size=B, seed=1, env=env)
    assert loop.env is env and loop.hist.state[..., 3].any() and not loop.hist.state[..., :3].any()

    taps = LoopMirror(loop, O.SimulatorMasterMirror())

    loop.run(90)
    torch.cuda.synchronize()
    assert loop.train_steps >= 4 and taps.episodes_over() == 3 * E      # every env hit limit 25 thrice
    sc = loop.last_scalars.cpu().numpy()
    assert np.all(np.isfinite(sc))
    assert not torch.equal(m.engine.params, p0)
    want = taps.queued()
    assert taps.consumed == want and len(want) >= B * loop.train_steps
    assert int(env.game[:, 8].max()) == 15                        # t = 90 - 75
    sampled = np.concatenate([a for a, _, _ in taps.drawn])
    assert 0 <= min(sampled) and max(sampled) < A and max(sampled) >= 4
    assert np.stack(taps.rewards).min() < 0


def test_launcher_trains_on_boxing_and_writes_mean_score(tmp_path):
    from ba3c_amd.train import main
    argv = ("-e GridBoxing-v0 --num_actions 18 -o adam -l 0.001 -b 32 --fc_neurons 128 --fc_splits 4 "
            "--epsilon 1e-8 --beta1 0.8 --beta2 0.75 --simulator_procs 64 --max_steps 6 "
            "--nr_eval 4 --steps_per_epoch 3 --send_debug_every 3").split()
    argv += ["--models_dir", str(tmp_path / "models"), "--experiment_dir", str(tmp_path / "exp")]
    out = main(argv)
    assert out["global_step"] >= 6 and np.isfinite(out["last"]["cost"])
    assert len(out["eval"]) == out["global_step"] // 3 >= 2      # every --steps_per_epoch steps
    rows = (tmp_path / "exp" / "mean_score.csv").read_text().strip().splitlines()
    assert rows[0] == "x,y" and len(rows) == 1 + len(out["eval"])
    for line, (mean, mx) in zip(rows[1:], out["eval"]):
        assert float(line.split(",")[1]) == mean and -101 <= mean <= mx <= 101
    assert (tmp_path / "exp" / "max_score.csv").exists()


def test_evaluator_on_fresh_weights_is_repeatable():
    from ba3c_amd.evaluate import Evaluator, eval_with_envs, uniform_policy
    from ba3c_amd.flags import GRID_BOXING
    from ba3c_amd.model import Model
    m = Model(num_actions=18, fc_neurons=128, fc_splits=4, batch_size=32, max_batch=32, seed=0)
    mean, mx = eval_with_envs(m.engine, nr_eval=6, n_envs=6, seed=0, limit=300, game=GRID_BOXING)
    assert np.isfinite(mean) and -101 <= mean <= mx <= 101
    assert eval_with_envs(m.engine, nr_eval=6, n_envs=6, seed=0, limit=300, game=GRID_BOXING) == (mean, mx)
    torch.manual_seed(0)
    r_mean, r_max = eval_with_envs(m.engine, 6, 6, seed=0, limit=300, policy=uniform_policy(18),
                                   game=GRID_BOXING)
    assert np.isfinite(r_mean) and -101 <= r_mean <= r_max <= 101

    class Sink(object):
        def __init__(self):
            self.scalars, self.msgs = [], []

        def write_scalar(self, name, v):
            self.scalars.append((name, v))

        def send(self, msg):
            self.msgs.append(msg)
    sink = Sink()
    ev = Evaluator(m.engine, 3, sink, limit=300, game=GRID_BOXING)
    got = ev()
    assert [n for n, _ in sink.scalars] == ["mean_score", "max_score"]
    assert sink.msgs == [(0, ("score",) + got)] and ev.n_envs == 3 and -101 <= got[0] <= got[1] <= 101
