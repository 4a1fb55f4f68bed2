"""Frame skip and sticky actions on the MI355X: one launch of ba3c_breakout_step_skip /
ba3c_boxing_step_skip (k game steps in registers, one render, one history push) equals the CPU
statement of a decision (ba3c_amd.frameskip.step_numpy over the games' own step_numpy /
render_numpy) bit for bit, and the skip vectors run through the actor-learner loop, the launcher
and the evaluation.  No test asserts that the agent learns and none asserts a time."""
import functools

import numpy as np
import pytest
import torch

from boxing_policy import history_push_numpy
from oracle import ba3c_oracle as O

pytestmark = pytest.mark.gpu

E, DECISIONS, LIMIT, SEED = 37, 60, 23, 3          # limit 23: episodes end mid-skip constantly
SETTINGS = [(1, 1, 0), (4, 4, 0), (2, 4, 16384), (1, 16, 58982)]
GAME_NAMES = ["breakout", "boxing"]
T = 8                                              # the column of t in both games' rows


def _game(name):
    from ba3c_amd import boxing, breakout
    return {"breakout": (breakout, breakout.BreakoutVec), "boxing": (boxing, boxing.BoxingVec)}[name]


class Trajectory(object):
    """actions [S,E], games [S+1,E,16], auxs [S+1,E,2] (index 0: the initial rows), reward [S,E]
    float64, over [S,E] bool, ep_score [S,E] int32: DECISIONS decisions of the oracle."""


@functools.lru_cache(maxsize=None)
def trajectory(name, setting):
    from ba3c_amd import frameskip as F
    K, _ = _game(name)
    lo, hi, q16 = setting
    rs = np.random.RandomState(SEED)
    odd = np.array([-1, 32, 1 << 40, (1 << 32) + 1, K.NUM_ACTIONS, 31, np.iinfo(np.int64).min], np.int64)
    game, aux = K.initial_game(E, SEED), F.initial_aux(E, SEED)
    if name == "breakout":
        # limit 23 ends an episode before a served ball can reach the bricks: every other row
        # starts with the ball in play just below them, moving up, so that rewards are summed
        odd_rows = np.arange(E) % 2 == 1
        game[odd_rows, K.BX] = 4 + 2 * np.arange(E)[odd_rows]
        game[odd_rows, K.BY], game[odd_rows, K.VY], game[odd_rows, K.IN_PLAY] = 38, -2, 1
        game[odd_rows, K.VX] = np.where(np.arange(E)[odd_rows] % 4 == 1, 1, -1)
    tr = Trajectory()
    tr.actions = np.zeros((DECISIONS, E), np.int64)
    tr.games = np.zeros((DECISIONS + 1, E, 16), np.int32)
    tr.auxs = np.zeros((DECISIONS + 1, E, 2), np.int32)
    tr.reward = np.zeros((DECISIONS, E), np.float64)
    tr.over = np.zeros((DECISIONS, E), bool)
    tr.ep_score = np.zeros((DECISIONS, E), np.int32)
    tr.games[0], tr.auxs[0] = game, aux
    for s in range(DECISIONS):
        a = rs.randint(K.NUM_ACTIONS, size=E).astype(np.int64)
        a[rs.random_sample(E) < 0.25] = 1                          # FIRE: serves, punches
        use_odd = rs.random_sample(E) < 0.2
        a = np.where(use_odd, odd[rs.randint(odd.size, size=E)], a)
        tr.actions[s] = a
        tr.reward[s], tr.over[s], tr.ep_score[s] = F.step_numpy(K, game, aux, a, LIMIT, lo, hi, q16)
        tr.games[s + 1], tr.auxs[s + 1] = game, aux
    for v in (tr.actions, tr.games, tr.auxs, tr.reward, tr.over, tr.ep_score):
        v.setflags(write=False)
    return tr


def _vec(name, setting, seed=SEED, limit=LIMIT, n_envs=E, rows=None):
    """A skip vector and its history.  (1, 1, 0) is the vector classes' plain path, so for that
    setting the aux rows are attached by hand: the skip entry point is what is under test."""
    from ba3c_amd import frameskip as F
    from ba3c_amd.rollout import FrameHistory
    _, Vec = _game(name)
    lo, hi, q16 = setting
    if setting == (1, 1, 0):
        env = Vec(n_envs, seed=seed, limit=limit)
        assert env.aux is None and env.skip is None
        env.skip = setting
        env.aux = torch.from_numpy(F.initial_aux(n_envs, seed)).cuda()
    else:
        env = Vec(n_envs, seed=seed, limit=limit, frame_skip=(lo, hi), sticky=q16 / 65536.0)
        assert env.skip == setting
    if rows is not None:
        env.game.copy_(torch.from_numpy(rows.copy()))
    hist = FrameHistory(n_envs, hist_len=4, channels=1)
    env.reset_history(hist)
    return env, hist


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "%d-%d-%d" % s)
@pytest.mark.parametrize("name", GAME_NAMES)
def test_skip_kernel_equals_the_oracle_bit_for_bit(name, setting):
    K, Vec = _game(name)
    tr = trajectory(name, setting)
    lo, hi, q16 = setting
    steps = tr.games[1:, :, T].astype(np.int64) - tr.games[:-1, :, T]
    assert tr.over.sum() >= E and (tr.actions < 0).any() and (tr.actions >= 32).any()
    if hi > 1:                                  # episodes ended with sub-steps left over
        assert (tr.over & (LIMIT - tr.games[:-1, :, T] < hi)).sum() >= E
        assert steps[~tr.over].max() == hi and steps[~tr.over].min() == lo
    assert (tr.reward != 0).any()
    fused, hist_f = _vec(name, setting, rows=tr.games[0])         # step_into: the fused push
    plain, hist_p = _vec(name, setting, rows=tr.games[0])         # step, then ba3c_history_push
    twin = None
    if setting == (1, 1, 0):
        twin = Vec(E, seed=SEED, limit=LIMIT)
        twin.game.copy_(fused.game)
    assert (fused.game.cpu().numpy() == tr.games[0]).all() and (fused.aux.cpu().numpy() == tr.auxs[0]).all()
    state = np.zeros((E, 84, 84, 4), np.uint8)
    state[..., 3] = K.render_numpy(tr.games[0])
    assert (hist_f.state.cpu().numpy() == state).all()
    ep = torch.full((E,), -777, dtype=torch.int32, device=fused.device)
    fused.ep_score = ep
    for s in range(DECISIONS):
        a = torch.from_numpy(tr.actions[s].copy()).cuda()
        ep.fill_(-777)
        reward, over = fused.step_into(a, hist_f)
        assert (fused.game.cpu().numpy() == tr.games[s + 1]).all(), s
        assert (fused.aux.cpu().numpy() == tr.auxs[s + 1]).all(), s
        assert reward.dtype == torch.float64 and (reward.cpu().numpy() == tr.reward[s]).all(), s
        assert (over.cpu().numpy() == tr.over[s]).all(), s
        # ep_score: the finished episode's score where over, untouched elsewhere
        assert (ep.cpu().numpy() == np.where(tr.over[s], tr.ep_score[s], -777)).all(), s
        frames = K.render_numpy(tr.games[s + 1])
        state = history_push_numpy(state, frames, tr.over[s])
        assert (hist_f.state.cpu().numpy() == state).all(), s
        got_frames, r_p, o_p = plain.step(a)
        assert (got_frames.cpu().numpy()[..., 0] == frames).all(), s
        hist_p.push(got_frames, o_p)
        assert torch.equal(hist_p.state, hist_f.state), s
        assert torch.equal(plain.game, fused.game) and torch.equal(plain.aux, fused.aux), s
        assert torch.equal(r_p, reward) and torch.equal(o_p, over), s
        assert (plain.ep_score.cpu().numpy()[tr.over[s]] == tr.ep_score[s][tr.over[s]]).all(), s
        if twin is not None:                    # the existing one-step entry point
            t_frames, t_reward, t_over = twin.step(a)
            assert torch.equal(twin.game, fused.game) and torch.equal(t_frames, got_frames), s
            assert torch.equal(t_reward, reward) and torch.equal(t_over, over), s
            assert (twin.ep_score.cpu().numpy()[tr.over[s]] == tr.ep_score[s][tr.over[s]]).all(), s


def test_default_vectors_allocate_no_aux_and_refuse_bad_settings():
    from ba3c_amd.boxing import BoxingVec
    from ba3c_amd.breakout import BreakoutVec
    for Vec in (BreakoutVec, BoxingVec):
        for kw in ({}, dict(frame_skip=1, sticky=0.0), dict(frame_skip=(1, 1))):
            env = Vec(3, **kw)
            assert env.aux is None and env.skip is None
        env = Vec(3, seed=2, frame_skip=4)
        assert env.skip == (4, 4, 0) and env.aux.shape == (3, 2) and env.aux.dtype == torch.int32
        assert env.aux[:, 0].cpu().numpy().view(np.uint32).tolist() == [(2000 + e) ^ 0x9E3779B9 for e in range(3)]
        for bad in (dict(frame_skip=0), dict(frame_skip=(5, 2)), dict(frame_skip=17), dict(sticky=1.5)):
            with pytest.raises(ValueError):
                Vec(3, **bad)


def test_actor_learner_runs_on_a_skip_vector():
    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.boxing import BoxingVec
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    n, B, A, iters = 24, 32, 18, 30
    m = Model(num_actions=A, fc_neurons=128, fc_splits=4, batch_size=B, max_batch=max(B, n))
    m.engine.load_params(O.init_params(128, 4, A, seed=0, dtype=np.float32))
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    p0 = m.engine.params.clone()
    env = BoxingVec(n, seed=1, limit=10 ** 6, frame_skip=(2, 4), sticky=0.25)
    aux0 = env.aux.clone()
    loop = ActorLearner(tr, n_envs=n, batch_size=B, seed=1, env=env)
    assert loop.env is env and loop.hist.state[..., 3].any() and not loop.hist.state[..., :3].any()
    loop.run(iters)
    torch.cuda.synchronize()
    assert loop.steps == iters and loop.train_steps >= 4
    assert np.all(np.isfinite(loop.last_scalars.cpu().numpy()))
    assert not torch.equal(m.engine.params, p0)
    t = env.game[:, T].cpu().numpy()            # no Boxing episode can end within 120 game steps
    assert (t >= 2 * iters).all() and (t <= 4 * iters).all() and t.min() < t.max()
    assert not torch.equal(env.aux[:, 0], aux0[:, 0]) and 0 <= int(env.aux[:, 1].min())
    assert int(env.aux[:, 1].max()) < A


def test_launcher_trains_and_evaluates_under_frame_skip(tmp_path):
    from ba3c_amd.train import main
    argv = ("-e GridBreakout-v0 -o adam -l 0.001 -b 32 --fc_neurons 128 --fc_splits 4 "
            "--epsilon 1e-8 --beta1 0.8 --beta2 0.75 --simulator_procs 64 --max_steps 6 "
            "--frame_skip 2-4 --sticky 0.25 --nr_eval 2 --steps_per_epoch 3 --send_debug_every 3").split()
    argv += ["--models_dir", str(tmp_path / "models"), "--experiment_dir", str(tmp_path / "exp")]
    out = main(argv)
    assert out["global_step"] >= 6 and np.isfinite(out["last"]["cost"])
    assert len(out["eval"]) == out["global_step"] // 3 >= 2
    rows = (tmp_path / "exp" / "mean_score.csv").read_text().strip().splitlines()
    assert rows[0] == "x,y" and len(rows) == 1 + len(out["eval"])
    for line, (mean, mx) in zip(rows[1:], out["eval"]):
        assert float(line.split(",")[1]) == mean and 0 <= mean <= mx <= 336


@pytest.mark.parametrize("name,A,lo_score,hi_score", [("breakout", 4, 0, 336), ("boxing", 18, -101, 101)])
def test_eval_with_envs_under_frame_skip(name, A, lo_score, hi_score):
    from ba3c_amd.evaluate import Evaluator, eval_with_envs, uniform_policy
    from ba3c_amd.flags import GRID_BOXING, GRID_BREAKOUT
    from ba3c_amd.model import Model
    game = GRID_BOXING if name == "boxing" else GRID_BREAKOUT
    m = Model(num_actions=A, fc_neurons=128, fc_splits=4, batch_size=32, max_batch=32, seed=0)
    kw = dict(seed=0, limit=300, policy=uniform_policy(A), game=game)
    torch.manual_seed(0)
    mean, mx = eval_with_envs(m.engine, 6, 6, frame_skip=(2, 4), sticky=0.25, **kw)
    assert np.isfinite(mean) and lo_score <= mean <= mx <= hi_score
    torch.manual_seed(0)
    assert eval_with_envs(m.engine, 6, 6, frame_skip=(2, 4), sticky=0.25, **kw) == (mean, mx)
    ev = Evaluator(m.engine, 3, None, limit=300, game=game, frame_skip=4, sticky=0.5)
    got = ev()
    assert (ev.frame_skip, ev.sticky) == (4, 0.5) and lo_score <= got[0] <= got[1] <= hi_score
