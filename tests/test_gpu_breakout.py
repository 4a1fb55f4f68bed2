"""GridBreakout on the MI355X: the fused step + render + history-push kernel
(ba3c_breakout_step / ba3c_breakout_render) equals the CPU statement of the rules
(ba3c_amd.breakout.step_numpy / render_numpy) bit for bit, the fused history push equals
ba3c_history_push, and the game runs through the actor-learner loop, the launcher and the
evaluator.  No test asserts that the agent learns and none asserts a time."""
import numpy as np
import pytest
import torch

from breakout_policy import (EVENTS, history_push_numpy, make_row, player_from_row, trajectory)
from loop_mirror import LoopMirror
from oracle import ba3c_oracle as O

pytestmark = pytest.mark.gpu


def _env_and_hist(E, seed, limit):
    from ba3c_amd.breakout import BreakoutVec
    from ba3c_amd.rollout import FrameHistory
    env = BreakoutVec(E, seed=seed, limit=limit)
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
    from ba3c_amd import breakout as K
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
        missing = [n for n in EVENTS if n not in ("ceiling", "over_clear") and tr.events[n] == 0]
        assert not missing, (missing, tr.events)
    assert tr.over.any() and tr.reward.sum() > 0
    env, hist = _env_and_hist(E, seed, limit)
    _check_against_oracle(env, hist, tr, every)


def test_crafted_rows_cover_ceiling_and_clear():
    """Rows written into the game tensor: the last brick about to go, a cleared column with
    the ball rising through it to the ceiling, a side wall and the ceiling in one step (both
    sides), and the last life about to be lost."""
    from ba3c_amd import breakout as K
    gap = 0x3FFF & ~(0x3F << 4)                                   # columns 4..9 cleared
    rows = np.stack([
        make_row(bx=19, by=37, vx=1, vy=-2, in_play=1, score=100, b0=0, b1=0, b2=0, b3=0, b4=0, b5=1 << 3),
        make_row(bx=26, by=37, vx=1, vy=-2, in_play=1, **{"b%d" % r: gap for r in range(6)}),
        make_row(bx=0, by=1, vx=-1, vy=-2, in_play=1),
        make_row(bx=82, by=1, vx=1, vy=-2, in_play=1),
        make_row(bx=30, by=82, vx=1, vy=2, in_play=1, lives=1, score=9),
    ]).astype(np.int32)
    E, steps, limit = rows.shape[0], 60, 50
    players = [player_from_row(r, limit=limit) for r in rows]
    env, hist = _env_and_hist(E, 0, limit)
    env.game.copy_(torch.from_numpy(rows))
    env.reset_history(hist)
    game = rows.copy()
    state = np.zeros((E, 84, 84, 4), np.uint8)
    state[..., 3] = K.render_numpy(game)
    assert (hist.state.cpu().numpy() == state).all()
    seen, first = set(), None
    rs = np.random.RandomState(0)
    for s in range(steps):
        a = np.where(rs.random_sample(E) < 0.3, 1, rs.randint(4, size=E)).astype(np.int64)
        reward, over, ep = K.step_numpy(game, a, limit)
        ev = set()
        for e, p in enumerate(players):
            assert p.action(int(a[e])) == (reward[e], bool(over[e])) and p.game_row() == game[e].tolist()
            ev |= {(e, n) for n in p.last_events}
        seen |= ev
        first = ev if first is None else first
        g_reward, g_over = env._step(torch.from_numpy(a).cuda(), env.frame, hist.state)
        assert (env.game.cpu().numpy() == game).all(), s
        assert (g_reward.cpu().numpy() == reward).all() and (g_over.cpu().numpy() == over).all(), s
        assert (env.ep_score.cpu().numpy()[over] == ep[over]).all(), s
        frames = K.render_numpy(game)
        state = history_push_numpy(state, frames, over)
        assert (env.frame.cpu().numpy()[..., 0] == frames).all(), s
        assert (hist.state.cpu().numpy() == state).all(), s
    assert {(0, "brick1"), (0, "over_clear"), (2, "wall"), (2, "ceiling"), (3, "wall"),
            (3, "ceiling"), (4, "lost"), (4, "over_lives")} <= first
    assert (1, "ceiling") in seen and "over_limit" in {n for _, n in seen}


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


def test_actions_are_compared_never_used_as_indices():
    """int64 actions outside [0, 4) are NOOP: same rows, frames and rewards as action 0."""
    E, steps, limit, seed = 8, 80, 60, 7
    odd = np.array([17, -1, 4, 1 << 40, -(1 << 62), np.iinfo(np.int64).min, np.iinfo(np.int64).max,
                    (1 << 32) + 1], np.int64)                     # low dword 1 = FIRE if truncated
    weird, hist_w = _env_and_hist(E, seed, limit)
    noop, hist_n = _env_and_hist(E, seed, limit)
    rs = np.random.RandomState(seed)
    for s in range(steps):
        legal = rs.randint(4, size=E).astype(np.int64)
        legal[rs.random_sample(E) < 0.3] = 1
        use_odd = rs.random_sample(E) < 0.5
        a_w = np.where(use_odd, np.roll(odd, s), legal)
        a_n = np.where(use_odd, 0, legal)
        r_w, o_w = weird.step_into(torch.from_numpy(a_w).cuda(), hist_w)
        r_n, o_n = noop.step_into(torch.from_numpy(a_n).cuda(), hist_n)
        assert torch.equal(weird.game, noop.game) and torch.equal(r_w, r_n) and torch.equal(o_w, o_n), s
        assert torch.equal(hist_w.state, hist_n.state), s
    assert int(noop.game[:, 8].max()) > 0 and bool(noop.game[:, 5].any())    # t ran, balls in play


def test_actor_learner_on_breakout_feeds_the_reference_datapoints():
    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.breakout import BreakoutVec
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    E, B = 24, 32
    m = Model(num_actions=4, fc_neurons=128, fc_splits=4, batch_size=B, max_batch=max(B, E))
    m.engine.load_params(O.init_params(128, 4, 4, seed=0, dtype=np.float32))
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    p0 = m.engine.params.clone()
    env = BreakoutVec(E, seed=1, limit=25)
    loop = ActorLearner(tr, n_envs=E, batch_size=B, seed=1, env=env)
    assert loop.env is env and loop.hist.state[..., 3].any() and not loop.hist.state[..., :3].any()

    taps = LoopMirror(loop, O.SimulatorMasterMirror())

    loop.run(40)
    torch.cuda.synchronize()
    assert loop.train_steps >= 4 and taps.episodes_over() == E      # every env hit limit 25 once
    sc = loop.last_scalars.cpu().numpy()
    assert np.all(np.isfinite(sc))
    assert not torch.equal(m.engine.params, p0)
    want = taps.queued()
    assert taps.consumed == want and len(want) >= B * loop.train_steps
    assert int(env.game[:, 8].max()) == 15                        # t = 40 - 25


def test_launcher_trains_on_breakout_and_writes_mean_score(tmp_path):
    from ba3c_amd.train import main
    argv = ("-e GridBreakout-v0 -o adam -l 0.001 -b 32 --fc_neurons 128 --fc_splits 4 "
            "--epsilon 1e-8 --beta1 0.8 --beta2 0.75 --simulator_procs 64 --max_steps 6 "
            "--nr_eval 4 --steps_per_epoch 3 --send_debug_every 3").split()
    argv += ["--models_dir", str(tmp_path / "models"), "--experiment_dir", str(tmp_path / "exp")]
    out = main(argv)
    assert out["global_step"] >= 6 and np.isfinite(out["last"]["cost"])
    assert len(out["eval"]) == out["global_step"] // 3 >= 2      # every --steps_per_epoch steps
    rows = (tmp_path / "exp" / "mean_score.csv").read_text().strip().splitlines()
    assert rows[0] == "x,y" and len(rows) == 1 + len(out["eval"])
    for line, (mean, mx) in zip(rows[1:], out["eval"]):
        assert float(line.split(",")[1]) == mean and 0 <= mean <= mx <= 336
    assert (tmp_path / "exp" / "max_score.csv").exists()


def test_evaluator_on_fresh_weights():
    from ba3c_amd.evaluate import Evaluator, eval_with_envs, uniform_policy
    from ba3c_amd.model import Model
    m = Model(num_actions=4, fc_neurons=128, fc_splits=4, batch_size=32, max_batch=32, seed=0)
    mean, mx = eval_with_envs(m.engine, nr_eval=6, n_envs=6, seed=0, limit=600)
    assert np.isfinite(mean) and 0 <= mean <= mx <= 336
    assert eval_with_envs(m.engine, nr_eval=6, n_envs=6, seed=0, limit=600) == (mean, mx)
    r_mean, r_max = eval_with_envs(m.engine, 6, 6, seed=0, limit=600, policy=uniform_policy(4))
    assert np.isfinite(r_mean) and 0 <= r_mean <= r_max <= 336

    class Sink(object):
        def __init__(self):
            self.scalars, self.msgs = [], []

        def write_scalar(self, name, v):
            self.scalars.append((name, v))

        def send(self, msg):
            self.msgs.append(msg)
    sink = Sink()
    ev = Evaluator(m.engine, 3, sink, limit=600)
    got = ev()
    assert [n for n, _ in sink.scalars] == ["mean_score", "max_score"]
    assert sink.msgs == [(0, ("score",) + got)] and ev.n_envs == 3
