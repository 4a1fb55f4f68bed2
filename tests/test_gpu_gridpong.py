"""GridPong on the MI355X: the step, the frame-skip decision, the render-only launch and the view equal
the CPU statements (ba3c_amd.gridpong, .frameskip, .view) bit for bit at E = 1, 3 and 37 simulators."""
import functools

import numpy as np
import pytest
import torch

from boxing_policy import history_push_numpy
from gridpong_policy import tracking_actions

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 37]
STEPS, LIMIT, SEED = 300, 130, 4


def _actions(game, s, rs):
    """Random actions, out-of-range ones among them; every third row plays the tracking script."""
    E = game.shape[0]
    odd = np.array([6, -1, (1 << 32) + 2, np.iinfo(np.int64).min, 1 << 40], np.int64)
    a = np.where(rs.random_sample(E) < 0.15, np.roll(np.resize(odd, E), s), rs.randint(6, size=E)).astype(np.int64)
    a[2::3] = tracking_actions(game, rs)[2::3]
    return a


@functools.lru_cache(maxsize=None)
def reference(E, skip):
    """STEPS steps (skip None) or decisions (lo, hi, q16) of the CPU statement: the start, and
    [(actions, game, aux, reward, over, ep_score, frames, state)] after each."""
    from ba3c_amd import frameskip as F
    from ba3c_amd import gridpong as K
    rs = np.random.RandomState(SEED + E)
    game, aux = K.initial_game(E, SEED), F.initial_aux(E, SEED)
    game[1::2, K.HITS] = 6            # a rally already six hits old: two more hits reach the cap (met at E = 37)
    state = np.zeros((E, 84, 84, 4), np.uint8)
    state[..., 3] = K.render_numpy(game)
    start, out = (game.copy(), state.copy()), []
    for s in range(STEPS):
        a = _actions(game, s, rs)
        if skip is None:
            r, over, ep = K.step_numpy(game, a, LIMIT)
        else:
            r, over, ep = F.step_numpy(K, game, aux, a, LIMIT, *skip)
        frames = K.render_numpy(game)
        state = history_push_numpy(state, frames, over)
        out.append((a, game.copy(), aux.copy(), r, over, ep, frames, state))
    return start, out


def _env(E, skip, game0):
    """PongVec on `game0`, its history started; skip: on the decision launch, then set to (lo, hi, q16)."""
    from ba3c_amd.gridpong import PongVec
    from ba3c_amd.rollout import FrameHistory
    env = PongVec(E, seed=SEED, limit=LIMIT, **(dict(frame_skip=(2, 4), sticky=0.25) if skip else {}))
    env.skip = skip
    env.game.copy_(torch.from_numpy(game0.copy()))
    hist = FrameHistory(E, hist_len=4, channels=1)
    env.reset_history(hist)
    return env, hist


def _replay(E, env, hist, ref, aux):
    """Every launch writes BOTH frame and state; everything it writes is compared."""
    ep = torch.full((E,), -777, dtype=torch.int32, device=env.device)
    env.ep_score = ep
    for s, (a, game, aux_ref, r, over, ep_ref, frames, state) in enumerate(ref):
        ep.fill_(-777)
        reward, got_over = env._step(torch.from_numpy(a.copy()).cuda(), env.frame, hist.state)
        assert (env.game.cpu().numpy() == game).all(), s
        assert not aux or (env.aux.cpu().numpy() == aux_ref).all(), s
        assert reward.dtype == torch.float64 and (reward.cpu().numpy() == r).all() and (got_over.cpu().numpy() == over).all(), s
        assert (ep.cpu().numpy() == np.where(over, ep_ref, -777)).all(), s
        assert (env.frame.cpu().numpy()[..., 0] == frames).all(), s
        assert (hist.state.cpu().numpy() == state).all(), s


@pytest.mark.parametrize("skip", [None, (2, 4, 16384), (1, 1, 0)], ids=["step", "2-4-sticky", "1-1"])
@pytest.mark.parametrize("E", SIZES)
def test_launch_equals_the_cpu_statement_bit_for_bit(E, skip):
    (game0, state0), ref = reference(E, skip)
    if skip is None and E == 37:                # what the run covers: resets, both signs, vx at its cap
        reward = np.stack([x[3] for x in ref])
        assert any(x[4].any() for x in ref) and (reward < 0).any() and (reward > 0).any()
        assert max(abs(x[1][:, 4]).max() for x in ref) == 14
    # a 1-1 / 0 decision must also equal the plain step's reference
    for want in [ref] + ([reference(E, None)[1]] if skip == (1, 1, 0) else []):
        env, hist = _env(E, skip, game0)
        assert (hist.state.cpu().numpy() == state0).all()
        _replay(E, env, hist, want, aux=want is ref and skip is not None)


@pytest.mark.parametrize("E", SIZES)
def test_render_only_launch_and_view(E):
    from ba3c_amd import gridpong as K
    from ba3c_amd.view import view_numpy
    rows = reference(E, None)[1][STEPS // 2][1]          # mid-run rows: scores, a ball in play
    env, hist = _env(E, None, rows)
    frames = K.render_numpy(rows)
    assert (env.frames().cpu().numpy()[..., 0] == frames).all()
    hist.state.fill_(9)
    got = env.reset_history(hist).cpu().numpy()
    assert (got[..., 3] == frames).all() and not got[..., :3].any()
    sel = [E - 1, 0, 0, E, -1]
    hud = np.random.RandomState(E).randint(0, 256, size=(len(sel), 20)).astype(np.uint8)
    for S in (1, 3):
        for use_sel, use_hud in ((sel, hud), (None, None)):
            got = env.view(scale=S, sel=use_sel, hud=None if use_hud is None else torch.from_numpy(use_hud).cuda())
            assert (got.cpu().numpy() == view_numpy(rows, K.PALETTE, S, use_hud, use_sel)).all(), (S, use_sel)
    assert (env.game.cpu().numpy() == rows).all()         # neither a render nor a view writes a row
