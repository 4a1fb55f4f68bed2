"""The colour view and the episode recorder on the MI355X: one launch of ba3c_breakout_view /
ba3c_boxing_view equals `ba3c_amd.view.view_numpy` of the rows read back bit for bit and writes
nothing but its output, and `ba3c_amd.record` writes episodes that the CPU oracle replays bit
for bit.  No test asserts a time."""
import functools

import numpy as np
import pytest
import torch

import boxing_policy
import breakout_policy

pytestmark = pytest.mark.gpu

E, LIMIT, STEPS, SEED = 5, 60, 40, 3
GAME_NAMES = ["breakout", "boxing"]
SEL = [4, 0, 0, 7, -1, 2]
SKIP = (2, 4, 16384)                      # frame_skip=(2, 4), sticky=0.25


def _game(name):
    from ba3c_amd import boxing, breakout
    from ba3c_amd.flags import GRID_BOXING, GRID_BREAKOUT
    return {"breakout": (breakout, breakout.BreakoutVec, breakout_policy, GRID_BREAKOUT),
            "boxing": (boxing, boxing.BoxingVec, boxing_policy, GRID_BOXING)}[name]


def _hud(n):
    """uint8 [n, 20] holding every clamp case: random bytes over the whole range (heights above
    16, actions 18..255, value bars above 84) and hand-written rows in front."""
    hud = np.random.RandomState(n).randint(0, 256, size=(n, 20)).astype(np.uint8)
    hud[0, :4], hud[0, 18], hud[0, 19] = (0, 1, 16, 200), 2, 0
    hud[1, :4], hud[1, 18], hud[1, 19] = (0, 1, 16, 200), 255, 84
    hud[2, 17], hud[2, 18], hud[2, 19] = 16, 17, 255
    return hud


@functools.lru_cache(maxsize=None)
def advanced(name):
    """The rows of E simulators after STEPS steps of the scripted policy, and the views the
    oracle gives of them: {(S, with_sel, with_hud): image}."""
    from ba3c_amd.view import view_numpy
    K, _, P, _ = _game(name)
    rows = P.trajectory(E, STEPS, LIMIT, SEED).games[STEPS].copy()
    want = {}
    for S in (1, 2, 3):
        for sel in (None, SEL):
            n = E if sel is None else len(sel)
            for hud in (None, _hud(n)):
                want[(S, sel is not None, hud is not None)] = view_numpy(rows, K.PALETTE, S, hud, sel)
    rows.setflags(write=False)
    return rows, want


@pytest.mark.parametrize("with_hud", [False, True], ids=["plain", "hud"])
@pytest.mark.parametrize("with_sel", [False, True], ids=["all", "sel"])
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("name", GAME_NAMES)
def test_view_equals_the_oracle_bit_for_bit(name, S, with_sel, with_hud):
    _, Vec, _, _ = _game(name)
    rows, want = advanced(name)
    env = Vec(E, seed=SEED, limit=LIMIT)
    env.game.copy_(torch.from_numpy(rows.copy()))
    n = len(SEL) if with_sel else E
    sel = torch.tensor(SEL, dtype=torch.int32, device="cuda") if with_sel else None
    hud = torch.from_numpy(_hud(n)).cuda() if with_hud else None
    got = env.view(scale=S, sel=sel, hud=hud)
    hc = 104 if with_hud else 84
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (n, hc * S, 84 * S, 3)
    assert (got.cpu().numpy() == want[(S, with_sel, with_hud)]).all()
    assert (env.game.cpu().numpy() == rows).all()
    if with_sel and not with_hud:           # sel as a list, and the palette is uploaded once
        pal = env._palette
        assert torch.equal(env.view(scale=S, sel=SEL), got) and env._palette is pal


def test_view_refuses_bad_arguments():
    from ba3c_amd.breakout import BreakoutVec
    env = BreakoutVec(2)
    for scale in (0, 9, 1.5):
        with pytest.raises(ValueError):
            env.view(scale=scale)
    with pytest.raises(ValueError):
        env.view(hud=torch.zeros((3, 20), dtype=torch.uint8))
    with pytest.raises(ValueError):
        env.view(hud=torch.zeros((2, 20), dtype=torch.int32))
    with pytest.raises(ValueError):
        env.view(sel=[])
    assert tuple(env.view(scale=8).shape) == (2, 672, 672, 3)


@pytest.mark.parametrize("name", GAME_NAMES)
def test_view_writes_nothing_it_can_be_observed_through(name):
    from ba3c_amd import frameskip as F
    from ba3c_amd.rollout import FrameHistory
    K, Vec, P, _ = _game(name)
    lo, hi, q16 = SKIP
    env = Vec(E, seed=SEED, limit=LIMIT, frame_skip=(lo, hi), sticky=q16 / 65536.0)
    assert env.skip == SKIP
    hist = FrameHistory(E, hist_len=4, channels=1)
    env.reset_history(hist)
    rs = np.random.RandomState(SEED)
    game, aux = K.initial_game(E, SEED), F.initial_aux(E, SEED)
    state = np.zeros((E, 84, 84, 4), np.uint8)
    state[..., 3] = K.render_numpy(game)

    def decision():
        nonlocal state
        a = P.scripted_actions(game, rs)
        r, over, _ = F.step_numpy(K, game, aux, a, LIMIT, lo, hi, q16)
        state = P.history_push_numpy(state, K.render_numpy(game), over)
        got_r, got_over = env.step_into(torch.from_numpy(a).cuda(), hist)
        assert (got_r.cpu().numpy() == r).all() and (got_over.cpu().numpy() == over).all()
        assert (env.game.cpu().numpy() == game).all() and (env.aux.cpu().numpy() == aux).all()
        assert (hist.state.cpu().numpy() == state).all()
    for _ in range(STEPS):
        decision()
    before = [t.clone() for t in (env.game, env.aux, hist.state, env.reward, env.over, env.ep_score)]
    env.view()
    env.view(scale=3, sel=SEL, hud=torch.from_numpy(_hud(len(SEL))).cuda())
    env.view(scale=2, hud=torch.from_numpy(_hud(E)).cuda())
    torch.cuda.synchronize()
    after = (env.game, env.aux, hist.state, env.reward, env.over, env.ep_score)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert (env.game.cpu().numpy() == game).all() and (env.aux.cpu().numpy() == aux).all()
    decision()                              # the next step still matches the oracle


def test_hud_from_policy_gives_the_same_bytes_on_the_device():
    from ba3c_amd.view import hud_from_policy
    g = torch.Generator().manual_seed(1)
    probs = torch.softmax(3 * torch.randn(257, 18, generator=g), dim=1)
    probs[0] = 0.0
    probs[0, 5] = 1.0
    probs[1] = 1.5 / 16                    # a tie: round half to even on both
    actions = torch.randint(-2, 21, (257,), generator=g)
    value = 2 * torch.randn(257, generator=g)
    value[:3] = torch.tensor([0.0, 50.0, -50.0])
    cpu = hud_from_policy(probs, actions, value)
    dev = hud_from_policy(probs.cuda(), actions.cuda(), value.cuda())
    assert dev.is_cuda and dev.dtype == torch.uint8 and torch.equal(dev.cpu(), cpu)
    assert cpu[0, :18].tolist() == [0] * 5 + [16] + [0] * 12 and cpu[1, :18].tolist() == [2] * 18
    assert torch.equal(hud_from_policy(probs.cuda(), None, None).cpu(), hud_from_policy(probs, None, None))


def _check_episode(ep, K, S, hud):
    """The recording against its own replay: rewards, score, and every kept frame's game part
    against the oracle's view of the replayed row."""
    from ba3c_amd.view import view_numpy
    rows, rewards, score = ep.replay()
    assert ep.steps >= 1 and rows.shape == (ep.steps + 1, 16)
    assert (rewards == ep.rewards).all() and score == ep.score and ep.rewards.dtype == np.float64
    assert (rows[0] == ep.row0).all()
    hc = 104 if hud else 84
    assert ep.frames.shape == (len(ep.frame_steps), hc * S, 84 * S, 3)
    assert (ep.frames[:, :84 * S] == view_numpy(rows[ep.frame_steps], K.PALETTE, S)).all()
    return rows


@pytest.mark.parametrize("skip", [None, SKIP], ids=["plain", "skip-2-4-sticky"])
@pytest.mark.parametrize("name", GAME_NAMES)
def test_record_episodes_with_a_uniform_policy_replays(name, skip):
    from ba3c_amd.evaluate import eval_with_envs, uniform_policy
    from ba3c_amd.model import Model
    from ba3c_amd.record import record_episodes
    K, _, _, game = _game(name)
    A = K.NUM_ACTIONS
    m = Model(num_actions=A, fc_neurons=128, fc_splits=4, batch_size=32, max_batch=32, seed=0)
    kw = dict(seed=2, limit=LIMIT, policy=uniform_policy(A))
    if skip is not None:
        kw.update(frame_skip=skip[:2], sticky=skip[2] / 65536.0)
    torch.manual_seed(0)
    eps = record_episodes(m.engine, game, 4, n_envs=3, scale=2, every=1, **kw)
    assert len(eps) >= 4
    for ep in eps:
        assert (ep.game, ep.limit, ep.skip) == (game, LIMIT, skip) and (ep.aux0 is None) == (skip is None)
        rows = _check_episode(ep, K, 2, True)
        assert (ep.frame_steps == np.arange(ep.steps)).all()
        assert ep.probs.shape == (ep.steps, A) and not ep.values.any()
        assert ((ep.actions >= 0) & (ep.actions < A)).all()
        assert int(rows[-2, 8]) < LIMIT and (skip is not None or ep.steps <= LIMIT)   # column 8: t
    # the recorder plays what the evaluation plays: same scores for the same arguments
    torch.manual_seed(0)
    mean, mx = eval_with_envs(m.engine, 4, 3, game=game, **kw)
    scores = [ep.score for ep in eps]
    assert mean == float(np.mean(scores)) and mx == float(max(scores))


def test_record_keeps_every_nth_frame_up_to_max_frames():
    from ba3c_amd import boxing as K
    from ba3c_amd.evaluate import uniform_policy
    from ba3c_amd.flags import GRID_BOXING
    from ba3c_amd.model import Model
    from ba3c_amd.record import record_episodes
    m = Model(num_actions=18, fc_neurons=128, fc_splits=4, batch_size=32, max_batch=32, seed=0)
    eps = record_episodes(m.engine, GRID_BOXING, 2, n_envs=2, limit=LIMIT, policy=uniform_policy(18),
                          scale=1, hud=False, every=7, max_frames=5)
    for ep in eps:
        assert ep.steps == LIMIT and ep.frame_steps.tolist() == [0, 7, 14, 21, 28]
        _check_episode(ep, K, 1, False)


@pytest.mark.parametrize("name", GAME_NAMES)
def test_record_episodes_with_a_tiny_engine_draws_the_policy(name):
    from ba3c_amd.engine import Ba3cEngine
    from ba3c_amd.record import record_episodes
    from ba3c_amd.view import hud_from_policy, hud_strip_numpy
    K, _, _, game = _game(name)
    A = K.NUM_ACTIONS
    eng = Ba3cEngine(num_actions=A, channels=4, fc_neurons=128, fc_splits=4, max_batch=3)
    eng.init_params(seed=1)
    eps = record_episodes(eng, game, 3, n_envs=3, seed=1, limit=LIMIT, scale=3, every=2)
    assert len(eps) >= 3
    for ep in eps:
        _check_episode(ep, K, 3, True)
        assert ep.probs.shape == (ep.steps, A) and np.isfinite(ep.values).all()
        assert np.abs(ep.probs.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-5
        assert (ep.frame_steps == np.arange(0, ep.steps, 2)).all()
        t = ep.frame_steps
        hud = hud_from_policy(torch.from_numpy(ep.probs[t]), torch.from_numpy(ep.actions[t]),
                              torch.from_numpy(ep.values[t])).numpy()
        assert (hud[:, 18] == ep.actions[t]).all()
        strip = np.repeat(np.repeat(hud_strip_numpy(hud), 3, axis=1), 3, axis=2)
        assert (ep.frames[:, 84 * 3:] == strip).all()


def test_record_cli_end_to_end(tmp_path, capsys):
    import json

    from ba3c_amd import boxing as K
    from ba3c_amd import record
    from ba3c_amd.checkpoint import ModelSaver
    from ba3c_amd.flags import GRID_BOXING
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.rollout import FrameHistory
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    m = Model(num_actions=18, fc_neurons=128, fc_splits=4, batch_size=32, max_batch=32, seed=5)
    trainer = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    ckpt = ModelSaver(str(tmp_path / "models")).trigger_step(trainer)
    out = record.main(["--load", ckpt, "-e", GRID_BOXING, "--num_actions", "18", "--fc_neurons", "128",
                       "--fc_splits", "4", "-b", "32", "--simulator_procs", "32", "--episodes", "1",
                       "--scale", "1", "--limit", "40", "--out", str(tmp_path / "rec")])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    npz = tmp_path / "rec" / "episode_000.npz"
    assert out["game"] == GRID_BOXING and str(npz) in out["files"] and npz.exists()
    ep = record.Episode.load(str(npz))
    assert out["scores"] == [ep.score] and out["steps"] == [ep.steps] == [40]
    _check_episode(ep, K, 1, True)
    # the checkpoint's policy, not a fresh one: the first decision's output is this model's
    env = K.BoxingVec(1, seed=0, limit=40)
    hist = FrameHistory(1, hist_len=4, channels=1)
    env.reset_history(hist)
    probs, _, value = m.engine.forward(hist.state)
    assert np.allclose(ep.probs[0], probs.cpu().numpy()[0], rtol=0, atol=1e-6)
    assert np.allclose(ep.values[0], value.cpu().numpy()[0], rtol=0, atol=1e-5)
    gif = tmp_path / "rec" / "episode_000.gif"
    try:
        import PIL  # noqa: F401
    except ImportError:
        assert not gif.exists() and out["files"] == [str(npz)]
    else:
        assert str(gif) in out["files"] and gif.stat().st_size > 0
