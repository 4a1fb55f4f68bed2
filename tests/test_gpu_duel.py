"""Two-player GridBoxing on the MI355X: the fused step + two renders + two history pushes of
ba3c_boxing_duel_step / ba3c_boxing_duel_render equal the CPU statement of the rules
(ba3c_amd.duel.step_numpy / render_numpy) bit for bit and keep the mirror invariant exactly, the
fused push equals ba3c_history_push, and the game runs through the colour view, the
actor-learner loop (self-play), `match` and the launcher.  No test asserts that a policy learns
and none asserts a time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from boxing_policy import history_push_numpy
from duel_policy import ODD_ACTIONS, crafted_rows, hit_and_run_policy, noop_policy, trajectory
from loop_mirror import LoopMirror
from oracle import ba3c_oracle as O

pytestmark = pytest.mark.gpu


def _env_and_hist(G, limit, rows=None, seed=0):
    from ba3c_amd.duel import BoxingDuelVec
    from ba3c_amd.rollout import FrameHistory
    env = BoxingDuelVec(G, seed=seed, limit=limit)
    if rows is not None:
        env.game.copy_(torch.from_numpy(np.array(rows)))              # (a writable copy)
    hist = FrameHistory(2 * G, hist_len=4, channels=1)
    env.reset_history(hist)
    return env, hist


@pytest.mark.parametrize("G,steps,limit,seed", [(1, 300, 60, 1), (3, 300, 60, 2), (37, 300, 60, 3)])
def test_kernel_equals_the_cpu_rules_bit_for_bit(G, steps, limit, seed):
    """One launch per step writing BOTH frame and state; every output of every player, at
    every step."""
    from ba3c_amd import duel as D
    tr = trajectory(G, steps, limit, seed)
    # what the CPU run covered: the step limit, and (beyond one game) hits, knock-outs before the
    # limit and out-of-range actions
    t_before = tr.games[:-1, :, 8]
    assert (tr.over[:, :G] & (t_before + 1 >= limit)).any()
    if G > 1:
        assert (tr.reward > 0).any() and (tr.over[:, :G] & (t_before + 1 < limit)).any()
        assert np.isin(tr.actions, ODD_ACTIONS).any()
    env, hist = _env_and_hist(G, limit, tr.games[0])
    assert env.E == 2 * G and env.G == G and tuple(env.game.shape) == (G, 16)
    state = np.zeros((2 * G, 84, 84, 4), np.uint8)
    state[..., 3] = D.render_numpy(tr.games[0])
    assert (env.frames().cpu().numpy()[..., 0] == state[..., 3]).all()
    assert (hist.state.cpu().numpy() == state).all()
    ep = torch.full((2 * G,), -777, dtype=torch.int32, device=env.device)
    env.ep_score = ep
    for s in range(steps):
        ep.fill_(-777)
        reward, over = env._step(torch.from_numpy(tr.actions[s].copy()).cuda(), env.frame, hist.state)
        assert (env.game.cpu().numpy() == tr.games[s + 1]).all(), s
        assert reward.dtype == torch.float64 and (reward.cpu().numpy() == tr.reward[s]).all(), s
        assert over.dtype == torch.bool and (over.cpu().numpy() == tr.over[s]).all(), s
        # ep_score: the finished episode's score where over, untouched elsewhere
        assert (ep.cpu().numpy() == np.where(tr.over[s], tr.ep_score[s], -777)).all(), s
        frames = D.render_numpy(tr.games[s + 1])
        state = history_push_numpy(state, frames, tr.over[s])
        assert (env.frame.cpu().numpy()[..., 0] == frames).all(), s
        assert (hist.state.cpu().numpy() == state).all(), s


def test_argument_combinations_write_the_same_step():
    """state only, frame only, both and neither: the same rows and per-player outputs, and each
    buffer that is given is written; ba3c_boxing_duel_render with and without state."""
    from ba3c_amd import duel as D
    G, steps, limit, seed = 3, 40, 12, 4
    tr = trajectory(G, steps, limit, seed)
    both, h_both = _env_and_hist(G, limit, tr.games[0])
    s_only, h_s = _env_and_hist(G, limit, tr.games[0])
    f_only, h_f = _env_and_hist(G, limit, tr.games[0])
    none, h_n = _env_and_hist(G, limit, tr.games[0])
    start = h_f.state.clone()
    for s in range(steps):
        a = torch.from_numpy(tr.actions[s].copy()).cuda()
        both._step(a, both.frame, h_both.state)
        s_only.step_into(a, h_s)
        frames, _, _ = f_only.step(a)
        none._step(a, None, None)
        for env in (both, s_only, f_only, none):
            assert (env.game.cpu().numpy() == tr.games[s + 1]).all(), s
            assert (env.reward.cpu().numpy() == tr.reward[s]).all(), s
            assert (env.last_over.cpu().numpy() == tr.over[s]).all(), s
        assert torch.equal(h_s.state, h_both.state) and torch.equal(frames, both.frame), s
        assert (frames.cpu().numpy()[..., 0] == D.render_numpy(tr.games[s + 1])).all(), s
    assert torch.equal(h_f.state, start) and torch.equal(h_n.state, start)     # never given: untouched
    assert not s_only.frame.any() and not none.frame.any()
    # render: frames of the current rows; with state the histories start; the rows are not written
    rows = tr.games[steps]
    want = D.render_numpy(rows)
    assert (both.frames().cpu().numpy()[..., 0] == want).all()
    assert torch.equal(both.reset_history(h_both)[..., 3], both.frames()[..., 0])
    assert not h_both.state[..., :3].any() and (both.game.cpu().numpy() == rows).all()
    fr, st = torch.zeros_like(both.frame), torch.ones_like(h_both.state)
    both._check(both.lib.ba3c_boxing_duel_render(both._stream(), both._ptr(both.game), G, both._ptr(fr),
                                                 both._ptr(st)))
    assert (fr.cpu().numpy()[..., 0] == want).all() and torch.equal(st, h_both.state)


def test_fused_push_equals_step_then_history_push():
    G, steps, limit, seed = 37, 60, 20, 5
    tr = trajectory(G, steps, limit, seed)
    assert tr.over[:, :G].sum() >= 2 * G
    fused, hist_f = _env_and_hist(G, limit, tr.games[0])
    plain, hist_p = _env_and_hist(G, limit, tr.games[0])
    assert torch.equal(hist_f.state, hist_p.state) and hist_f.state.any()
    for s in range(steps):
        a = torch.from_numpy(tr.actions[s].copy()).cuda()
        r_f, o_f = fused.step_into(a, hist_f)
        frames, r_p, o_p = plain.step(a)
        hist_p.push(frames, o_p)                                  # ba3c_history_push on the 2G frames
        assert torch.equal(hist_f.state, hist_p.state), s
        assert torch.equal(fused.game, plain.game) and torch.equal(r_f, r_p) and torch.equal(o_f, o_p)
    assert (fused.game.cpu().numpy() == tr.games[-1]).all()


def test_the_mirror_invariant_holds_exactly_on_the_device():
    """The kernel on `rows` with (a, b) and on mirror_rows(rows) with (b, a): every output of
    the second run is the first's with the player halves swapped, rewards and ep_scores negated
    and rows mirrored."""
    from ba3c_amd import duel as D
    G, steps, limit, seed = 37, 120, 40, 6
    tr = trajectory(G, steps, limit, seed)
    assert (tr.reward > 0).any() and tr.over.any()
    one, hist_1 = _env_and_hist(G, limit, tr.games[0])
    two, hist_2 = _env_and_hist(G, limit, D.mirror_rows(tr.games[0]))
    swap = lambda t: torch.cat([t[G:], t[:G]])
    assert torch.equal(hist_2.state, swap(hist_1.state))
    for s in range(steps):
        a = torch.from_numpy(tr.actions[s].copy()).cuda()
        one.ep_score.fill_(0)
        two.ep_score.fill_(0)
        r1, o1 = one._step(a, one.frame, hist_1.state)
        r2, o2 = two._step(swap(a), two.frame, hist_2.state)
        assert (two.game.cpu().numpy() == D.mirror_rows(one.game.cpu().numpy())).all(), s
        assert torch.equal(r2, swap(r1)) and torch.equal(r2, -r1) and torch.equal(o2, swap(o1)), s
        assert torch.equal(two.ep_score, swap(one.ep_score)) and torch.equal(two.ep_score, -one.ep_score), s
        assert torch.equal(two.frame, swap(one.frame)) and torch.equal(hist_2.state, swap(hist_1.state)), s
    assert (one.game.cpu().numpy() == tr.games[-1]).all()


def test_view_shows_the_games_as_side_a_sees_them():
    from ba3c_amd import boxing as K
    from ba3c_amd.view import view_numpy
    G = 5
    rows = trajectory(G, 40, 60, 7).games[40]
    env, _ = _env_and_hist(G, 60, rows)
    sel = [4, 0, 0, 7, -1, 2]                                     # 7 and -1: no such game
    hud = np.random.RandomState(0).randint(0, 256, size=(len(sel), 20)).astype(np.uint8)
    got = env.view(scale=2, sel=sel, hud=torch.from_numpy(hud))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(sel), 208, 168, 3)
    assert (got.cpu().numpy() == view_numpy(rows, K.PALETTE, 2, hud, sel)).all()
    assert not got[3].any() and not got[4].any()
    assert (env.view().cpu().numpy() == view_numpy(rows, K.PALETTE)).all() and env.view().shape[0] == G
    assert (env.game.cpu().numpy() == rows).all()


def test_self_play_through_the_actor_learner_feeds_each_player_its_own_rewards():
    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.duel import BoxingDuelVec
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    G, B, A = 4, 32, 18
    E = 2 * G
    m = Model(num_actions=A, fc_neurons=128, fc_splits=4, batch_size=B, max_batch=B)
    m.engine.load_params(O.init_params(128, 4, A, seed=0, dtype=np.float32))
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    p0 = m.engine.params.clone()
    env = BoxingDuelVec(G, seed=1, limit=25)
    env.game.copy_(torch.from_numpy(crafted_rows(G, 1)))          # within reach: rewards flow at once
    loop = ActorLearner(tr, n_envs=E, batch_size=B, seed=1, env=env)
    assert loop.env is env and loop.hist.state[..., 3].any() and not loop.hist.state[..., :3].any()
    assert torch.equal(loop.hist.state[..., 3], env.frames()[..., 0])

    def zero_sum(r, o):
        assert (r[:G] == -r[G:]).all() and (o[:G] == o[G:]).all()  # zero-sum, one clock per game
    taps = LoopMirror(loop, O.SimulatorMasterMirror(), on_step=zero_sum)   # player e's OWN rewards

    loop.run(90)
    torch.cuda.synchronize()
    assert loop.train_steps >= 4 and taps.episodes_over() >= 3 * E      # limit 25: at least thrice each
    assert np.all(np.isfinite(loop.last_scalars.cpu().numpy()))
    assert not torch.equal(m.engine.params, p0)
    want = taps.queued()
    assert taps.consumed == want and len(want) >= B * loop.train_steps
    assert np.abs(np.stack(taps.rewards)).max() > 0               # punches landed


def test_match_is_won_by_the_better_script_from_either_side():
    from ba3c_amd.duel import match
    won = match(hit_and_run_policy, noop_policy, n_games=4, episodes=4, seed=0)
    assert won["episodes"] == len(won["scores"]) >= 4
    assert (won["wins"], won["draws"], won["losses"]) == (won["episodes"], 0, 0)
    assert min(won["scores"]) >= 90 and won["max_score"] == max(won["scores"])
    assert won["mean_score"] == float(np.mean(won["scores"]))
    lost = match(noop_policy, hit_and_run_policy, n_games=4, episodes=4, seed=0)
    assert (lost["wins"], lost["draws"], lost["losses"]) == (0, 0, lost["episodes"])
    assert sorted(lost["scores"]) == sorted(-s for s in won["scores"])
    assert lost["mean_score"] == -won["mean_score"]


def test_match_of_one_fresh_engine_against_itself_is_repeatable():
    from ba3c_amd.duel import match
    from ba3c_amd.model import Model
    m = Model(num_actions=18, fc_neurons=128, fc_splits=4, batch_size=32, max_batch=32, seed=0)
    a = match(m.engine, m.engine, n_games=3, episodes=3, seed=5, limit=200)
    assert a["episodes"] >= 3 and a["wins"] + a["draws"] + a["losses"] == a["episodes"]
    assert all(-101 <= s <= 101 for s in a["scores"])
    assert match(m.engine, m.engine, n_games=3, episodes=3, seed=5, limit=200) == a


def test_launcher_trains_by_self_play_in_a_child_process(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(root, "distributed-ba3c_amd"), env.get("PYTHONPATH", "")])
    argv = ("-e GridBoxing-v0 --num_actions 18 --self_play --simulator_procs 8 -o adam -l 0.001 -b 32 "
            "--fc_neurons 128 --fc_splits 4 --epsilon 1e-8 --beta1 0.8 --beta2 0.75 --max_steps 5 "
            "--nr_eval 2 --steps_per_epoch 5 --send_debug_every 5").split()
    argv += ["--models_dir", str(tmp_path / "models"), "--experiment_dir", str(tmp_path / "exp")]
    r = subprocess.run([sys.executable, "-m", "ba3c_amd.train"] + argv, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["global_step"] >= 5 and np.isfinite(out["last"]["cost"])
    assert len(out["eval"]) == out["global_step"] // 5 >= 1       # against the scripted opponent
    rows = (tmp_path / "exp" / "mean_score.csv").read_text().strip().splitlines()
    assert rows[0] == "x,y" and len(rows) == 1 + len(out["eval"])
    for line, (mean, mx) in zip(rows[1:], out["eval"]):
        assert float(line.split(",")[1]) == mean and -101 <= mean <= mx <= 101
