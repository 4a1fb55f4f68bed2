"""Two-player GridBoxing's decisions on the MI355X: one launch of ba3c_boxing_duel_decide (frame
skip, sticky actions per side, drawn starts, two renders, two history pushes) equals the CPU
statement of the rules (ba3c_amd.duel.decide_numpy) bit for bit, equals ba3c_boxing_duel_step at
the default setting, keeps the mirror invariant exactly, and runs through the colour view of
either side, the actor-learner loop (self-play) and the launcher.  No test asserts that a policy
learns and none asserts a time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from boxing_policy import history_push_numpy
from duel_decision import SKIPS, STARTS, assert_covered, trajectory
from duel_policy import crafted_rows
from duel_policy import trajectory as step_trajectory
from loop_mirror import LoopMirror
from oracle import ba3c_oracle as O

pytestmark = pytest.mark.gpu

STEPS, LIMIT = 60, 23


def _env_and_hist(G, limit, rows, aux, skip, start):
    """A vector on the decision launch under exactly (skip, start) -- (1, 1, 0) with the fixed
    start included, which the constructor would hand to the one-step launch -- from the given
    rows and aux rows."""
    from ba3c_amd.duel import FIXED_START, BoxingDuelDecisionVec
    from ba3c_amd.rollout import FrameHistory
    env = BoxingDuelDecisionVec(G, seed=0, limit=limit, frame_skip=2)
    env.skip, env.start = tuple(skip), tuple(start) if start is not None else FIXED_START
    env.game.copy_(torch.from_numpy(np.array(rows)))                  # (writable copies)
    env.aux.copy_(torch.from_numpy(np.array(aux)))
    hist = FrameHistory(2 * G, hist_len=4, channels=1)
    env.reset_history(hist)
    return env, hist


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("skip", SKIPS)
@pytest.mark.parametrize("G,seed", [(1, 1), (3, 4), (37, 3)])
def test_kernel_equals_the_cpu_rules_bit_for_bit(G, seed, skip, start):
    """One launch per decision writing BOTH frame and state; every output of every player, the
    rows and the aux rows, after every decision."""
    from ba3c_amd import duel as D
    tr = trajectory(G, STEPS, LIMIT, seed, skip, start)
    assert_covered(tr, G, LIMIT, skip, start)
    env, hist = _env_and_hist(G, LIMIT, tr.games[0], tr.auxs[0], skip, start)
    assert tuple(env.aux.shape) == (G, 8) and env.aux.dtype == torch.int32
    state = np.zeros((2 * G, 84, 84, 4), np.uint8)
    state[..., 3] = D.render_numpy(tr.games[0])
    assert (hist.state.cpu().numpy() == state).all()
    ep = torch.full((2 * G,), -777, dtype=torch.int32, device=env.device)
    env.ep_score = ep
    for s in range(STEPS):
        ep.fill_(-777)
        reward, over = env._step(torch.from_numpy(tr.actions[s].copy()).cuda(), env.frame, hist.state)
        assert (env.game.cpu().numpy() == tr.games[s + 1]).all(), s
        assert (env.aux.cpu().numpy() == tr.auxs[s + 1]).all(), s
        assert reward.dtype == torch.float64 and (reward.cpu().numpy() == tr.reward[s]).all(), s
        assert over.dtype == torch.bool and (over.cpu().numpy() == tr.over[s]).all(), s
        # ep_score: the finished episode's score where over, untouched elsewhere
        assert (ep.cpu().numpy() == np.where(tr.over[s], tr.ep_score[s], -777)).all(), s
        frames = D.render_numpy(tr.games[s + 1])
        state = history_push_numpy(state, frames, tr.over[s])
        assert (env.frame.cpu().numpy()[..., 0] == frames).all(), s
        assert (hist.state.cpu().numpy() == state).all(), s


@pytest.mark.parametrize("G,seed", [(1, 1), (3, 2), (37, 3)])
def test_the_default_decision_equals_the_one_step_launch(G, seed):
    """(1, 1, 0) with the fixed start against ba3c_boxing_duel_step, from the same rows and
    actions: every output, and rng untouched."""
    from ba3c_amd import duel as D
    from ba3c_amd.duel import BoxingDuelDecisionVec, BoxingDuelVec
    from ba3c_amd.rollout import FrameHistory
    tr = step_trajectory(G, STEPS, LIMIT, seed)
    assert tr.over.any() and (G == 1 or (tr.reward != 0).any())
    plain = BoxingDuelDecisionVec(G, seed=seed, limit=LIMIT)      # the defaults: a BoxingDuelVec
    assert plain.aux is None and plain.skip is None and plain.start is None
    assert torch.equal(plain.game, BoxingDuelVec(G, seed=seed, limit=LIMIT).game)
    assert (plain.game.cpu().numpy() == D.initial_game(G, seed)).all()           # today's rows
    plain.game.copy_(torch.from_numpy(np.array(tr.games[0])))
    hist_p = FrameHistory(2 * G, hist_len=4, channels=1)
    plain.reset_history(hist_p)
    dec, hist_d = _env_and_hist(G, LIMIT, tr.games[0], D.initial_aux(G, seed), (1, 1, 0), None)
    assert torch.equal(hist_p.state, hist_d.state)
    for s in range(STEPS):
        a = torch.from_numpy(tr.actions[s].copy()).cuda()
        plain.ep_score.fill_(-777)
        dec.ep_score.fill_(-777)
        r_p, o_p = plain._step(a, plain.frame, hist_p.state)
        r_d, o_d = dec._step(a, dec.frame, hist_d.state)
        assert (plain.game.cpu().numpy() == tr.games[s + 1]).all(), s
        assert torch.equal(dec.game, plain.game) and torch.equal(r_d, r_p) and torch.equal(o_d, o_p), s
        assert torch.equal(dec.ep_score, plain.ep_score) and torch.equal(dec.frame, plain.frame), s
        assert torch.equal(hist_d.state, hist_p.state), s
    assert torch.equal(dec.game[:, 9], torch.from_numpy(np.array(tr.games[0][:, 9])).cuda())


def test_argument_combinations_write_the_same_decision():
    """state only, frame only, both and neither: the same rows, aux rows and per-player
    outputs, and each buffer that is given is written."""
    from ba3c_amd import duel as D
    G, seed, skip, start = 3, 4, (2, 4, 16384), (4, 7)
    tr = trajectory(G, STEPS, LIMIT, seed, skip, start)
    both, h_both = _env_and_hist(G, LIMIT, tr.games[0], tr.auxs[0], skip, start)
    s_only, h_s = _env_and_hist(G, LIMIT, tr.games[0], tr.auxs[0], skip, start)
    f_only, h_f = _env_and_hist(G, LIMIT, tr.games[0], tr.auxs[0], skip, start)
    none, h_n = _env_and_hist(G, LIMIT, tr.games[0], tr.auxs[0], skip, start)
    first = h_f.state.clone()
    for s in range(STEPS):
        a = torch.from_numpy(tr.actions[s].copy()).cuda()
        both._step(a, both.frame, h_both.state)
        s_only.step_into(a, h_s)
        frames, _, _ = f_only.step(a)
        none._step(a, None, None)
        for env in (both, s_only, f_only, none):
            assert (env.game.cpu().numpy() == tr.games[s + 1]).all(), s
            assert (env.aux.cpu().numpy() == tr.auxs[s + 1]).all(), s
            assert (env.reward.cpu().numpy() == tr.reward[s]).all(), s
            assert (env.last_over.cpu().numpy() == tr.over[s]).all(), s
        assert torch.equal(h_s.state, h_both.state) and torch.equal(frames, both.frame), s
        assert (frames.cpu().numpy()[..., 0] == D.render_numpy(tr.games[s + 1])).all(), s
    assert tr.over.any()
    assert torch.equal(h_f.state, first) and torch.equal(h_n.state, first)       # never given: untouched
    assert not s_only.frame.any() and not none.frame.any()


def test_the_mirror_invariant_of_a_decision_holds_exactly_on_the_device():
    """The kernel on (rows, aux) with (a, b) and on their mirrors with (b, a): every output of
    the second run is the first's with the player halves swapped, rewards and ep_scores negated
    and the rows and aux rows mirrored."""
    from ba3c_amd import duel as D
    G, seed, skip, start = 37, 5, (2, 4, 16384), (4, 7)
    tr = trajectory(G, STEPS, LIMIT, seed, skip, start)
    assert_covered(tr, G, LIMIT, skip, start)
    one, hist_1 = _env_and_hist(G, LIMIT, tr.games[0], tr.auxs[0], skip, start)
    two, hist_2 = _env_and_hist(G, LIMIT, D.mirror_rows(tr.games[0]), D.mirror_aux(tr.auxs[0]), skip, start)
    swap = lambda t: torch.cat([t[G:], t[:G]])
    assert torch.equal(hist_2.state, swap(hist_1.state))
    for s in range(STEPS):
        a = torch.from_numpy(tr.actions[s].copy()).cuda()
        one.ep_score.fill_(0)
        two.ep_score.fill_(0)
        r1, o1 = one._step(a, one.frame, hist_1.state)
        r2, o2 = two._step(swap(a), two.frame, hist_2.state)
        assert (two.game.cpu().numpy() == D.mirror_rows(one.game.cpu().numpy())).all(), s
        assert (two.aux.cpu().numpy() == D.mirror_aux(one.aux.cpu().numpy())).all(), s
        assert torch.equal(r2, swap(r1)) and torch.equal(r2, -r1) and torch.equal(o2, swap(o1)), s
        assert torch.equal(two.ep_score, swap(one.ep_score)) and torch.equal(two.ep_score, -one.ep_score), s
        assert torch.equal(two.frame, swap(one.frame)) and torch.equal(hist_2.state, swap(hist_1.state)), s
    assert (one.game.cpu().numpy() == tr.games[-1]).all()


def test_view_of_side_b_is_the_view_of_the_mirrored_rows():
    from ba3c_amd import boxing as K
    from ba3c_amd import duel as D
    from ba3c_amd.view import view_numpy
    G = 5
    rows = trajectory(G, STEPS, LIMIT, 7, (2, 4, 16384), (4, 19)).games[40]
    env, _ = _env_and_hist(G, LIMIT, rows, D.initial_aux(G, 7), (2, 4, 16384), (4, 19))
    assert (env.mirrored_game().cpu().numpy() == D.mirror_rows(rows)).all()
    sel = [4, 0, 0, 7, -1, 2]                                     # 7 and -1: no such game
    hud = np.random.RandomState(0).randint(0, 256, size=(len(sel), 20)).astype(np.uint8)
    got = env.view(scale=2, sel=sel, hud=torch.from_numpy(hud), side="b")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(sel), 208, 168, 3)
    assert (got.cpu().numpy() == view_numpy(D.mirror_rows(rows), K.PALETTE, 2, hud, sel)).all()
    assert not (got.cpu().numpy() == view_numpy(rows, K.PALETTE, 2, hud, sel)).all()
    assert (env.view(side="b").cpu().numpy() == view_numpy(D.mirror_rows(rows), K.PALETTE)).all()
    assert (env.view(side="a").cpu().numpy() == view_numpy(rows, K.PALETTE)).all()
    assert torch.equal(env.view(), env.view(side="a")) and (env.game.cpu().numpy() == rows).all()
    with pytest.raises(ValueError):
        env.view(side="c")


def test_self_play_with_frame_skip_and_drawn_starts_feeds_each_player_its_own_rewards():
    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.duel import BoxingDuelDecisionVec
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    G, B, A = 4, 32, 18
    E = 2 * G
    m = Model(num_actions=A, fc_neurons=128, fc_splits=4, batch_size=B, max_batch=B)
    m.engine.load_params(O.init_params(128, 4, A, seed=0, dtype=np.float32))
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    p0 = m.engine.params.clone()
    env = BoxingDuelDecisionVec(G, seed=1, limit=25, frame_skip=(2, 4), sticky=0.25, start=(4, 7))
    assert env.skip == (2, 4, 16384) and env.start == (4, 7) and tuple(env.aux.shape) == (G, 8)
    rows0 = env.game.cpu().numpy()
    assert ((rows0[:, 2] - rows0[:, 0]) <= 14).all() and (rows0[:, 1] == rows0[:, 3]).all()   # drawn
    env.game.copy_(torch.from_numpy(crafted_rows(G, 1)))          # scores 90..99: episodes end early too
    loop = ActorLearner(tr, n_envs=E, batch_size=B, seed=1, env=env)
    assert loop.env is env and torch.equal(loop.hist.state[..., 3], env.frames()[..., 0])

    gaps = []

    def zero_sum(r, o):
        assert (r[:G] == -r[G:]).all() and (o[:G] == o[G:]).all()  # zero-sum, one clock per game
        g = env.game.cpu().numpy()
        gaps.extend((g[o[:G], 2] - g[o[:G], 0]).tolist())          # the fresh rows: drawn
    taps = LoopMirror(loop, O.SimulatorMasterMirror(), on_step=zero_sum)   # player e's OWN rewards

    loop.run(90)
    torch.cuda.synchronize()
    assert loop.train_steps >= 4 and taps.episodes_over() >= 3 * E      # limit 25, k >= 2: often
    assert np.all(np.isfinite(loop.last_scalars.cpu().numpy()))
    assert not torch.equal(m.engine.params, p0)
    want = taps.queued()
    assert taps.consumed == want and len(want) >= B * loop.train_steps
    assert np.abs(np.stack(taps.rewards)).max() > 0               # punches landed
    assert gaps and set(gaps) <= {8, 10, 12, 14} and len(set(gaps)) > 1


def test_launcher_trains_by_self_play_with_the_new_flags_in_a_child_process(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(root, "distributed-ba3c_amd"), env.get("PYTHONPATH", "")])
    argv = ("-e GridBoxing-v0 --num_actions 18 --self_play --duel_frame_skip 2-4 --duel_sticky 0.25 --duel_start 8-14 "
            "--simulator_procs 8 -o adam -l 0.001 -b 32 --fc_neurons 128 --fc_splits 4 --epsilon 1e-8 "
            "--beta1 0.8 --beta2 0.75 --max_steps 5 --nr_eval 2 --steps_per_epoch 5 "
            "--send_debug_every 5").split()
    argv += ["--models_dir", str(tmp_path / "models"), "--experiment_dir", str(tmp_path / "exp")]
    r = subprocess.run([sys.executable, "-m", "ba3c_amd.train"] + argv, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["global_step"] >= 5 and np.isfinite(out["last"]["cost"])
    assert len(out["eval"]) == out["global_step"] // 5 >= 1       # against the scripted opponent
    for mean, mx in out["eval"]:
        assert -101 <= mean <= mx <= 101
