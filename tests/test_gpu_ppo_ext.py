"""ba3c_ppo_norm_adv, the extended PPO heads (ba3c_train_grads_ppo_ext: the clipped value loss and
the advantage from the row), their phases and the learner's loop with the three optional pieces on
the GPU, held to ba3c_amd.ppo (float64) with test_gpu_parity's bounds."""
import numpy as np
import pytest
import torch

from ba3c_amd import ppo
from ba3c_amd._lib import PPO_ADV_FROM_ROW, SCALAR_NAMES
from fc_stage import ALL_HEADS_FORMS, heads_form
from oracle import ba3c_oracle as O
from test_gpu_parity import FWD_TOL, GRAD_TOL, as64, case, dev, engine, gpu_decisions, rel
from test_gpu_ppo import HEADS, _check_scalars, _lpa
from test_ppo_ext_rules import ALL_VALUE_CLIPPED, VCASES, VCLIP, check_cases_ext, crafted_rows_ext
from test_ppo_rules import BETA, EPS

pytestmark = pytest.mark.gpu


# ---- ba3c_ppo_norm_adv --------------------------------------------------------------------------
NORM_N = [1, 2, 5, 32, 33, 63, 64, 65, 255, 256, 257, 2049]


def _norm_rows(kind, n, seed):
    rs = np.random.RandomState(seed)
    rows = rs.normal(size=(n, 4)).astype(np.float32)          # column 3: whatever was there
    if kind == "offset":
        rows[:, 0] = (2.0 ** 20 + 8.0 * rs.normal(size=n)).astype(np.float32)
    elif kind == "constant":
        rows[:, 0], rows[:, 1] = np.float32(0.7), np.float32(0.4)
    elif kind == "tiny":
        rows[:, 1] = rows[:, 0] - (1e-6 * rs.normal(size=n)).astype(np.float32)
    return rows


@pytest.mark.parametrize("kind", ["plain", "offset", "constant", "tiny"])
def test_norm_adv_matches_the_rules(kind):
    eng = engine()
    worst = 0.0
    for n in NORM_N:
        rows = _norm_rows(kind, n, seed=1000 + n)
        ref, mean, std = ppo.normalise_adv_numpy(rows)
        adv = rows[:, 0].astype(np.float64) - rows[:, 1].astype(np.float64)
        a, b = dev(rows), dev(rows)
        stats = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
        assert eng.ppo_norm_adv(a, stats) is a
        eng.ppo_norm_adv(b, None)                             # a null stats is accepted
        got, again, st = a.cpu().numpy(), b.cpu().numpy(), stats.cpu().numpy()
        assert got[:, :3].tobytes() == rows[:, :3].tobytes(), (kind, n)
        assert got.tobytes() == again.tobytes(), (kind, n)    # a second launch: the same bits
        bound = 2.0 ** -23 * np.maximum(np.abs(ref[:, 3].astype(np.float64)), 1.0)
        err = np.abs(got[:, 3].astype(np.float64) - ref[:, 3].astype(np.float64))
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (kind, n, float((err / bound).max()))
        tol = 1e-12 * np.abs(adv).max()
        assert abs(st[0] - mean) <= tol and abs(st[1] - std) <= tol, (kind, n, st, mean, std)
        if kind == "constant":
            assert np.abs(got[:, 3]).max() <= 1e-6
        if n == 1:
            assert got[0, 3] == 0.0
    print("%s: worst .w deviation %.3f of its bound" % (kind, worst))


# ---- the extended heads -------------------------------------------------------------------------
def _ext(eng, state, action, rows, clip, vclip, flags, phase=0):
    """ba3c_train_grads_ppo_ext as it is exported (the engine's method makes the same call);
    vclip = None: ba3c_train_grads_ppo, the exported plain entry, which has neither setting."""
    from ba3c_amd import _lib
    from ba3c_amd.engine import _ptr, _stream
    B = state.shape[0]
    if eng.ratio is None:
        eng.ratio = torch.ones(eng.max_batch, dtype=torch.float32, device=eng.device)
    tail = (_ptr(eng._workspace(True)), _ptr(eng.grads), _ptr(eng.scalars), _ptr(eng.ratio), phase)
    head = (eng.h, _stream(), _ptr(eng.params), _ptr(state), _ptr(action), _ptr(rows), B, BETA)
    if vclip is None:
        _lib.check(eng.lib.ba3c_train_grads_ppo(*head, clip, *tail))
    else:
        _lib.check(eng.lib.ba3c_train_grads_ppo_ext(*head, clip, vclip, flags, *tail))
    return eng.scalars


def _value(h, params):
    return (h.astype(np.float64) @ params["fc-v/W"].astype(np.float64)
            + params["fc-v/b"].astype(np.float64))[:, 0]


def _prepared(seed, B, vcases=VCASES, **cfgk):
    """An engine that has run the A3C pass on a fresh case, the case, the GPU's own h and rows
    crafted on it over the policy x value cases (h does not depend on the loss)."""
    params, state, action, R, cfg = case(seed, B, **cfgk)
    eng = engine(max_batch=max(64, B), **cfgk)
    eng.load_params(params)
    a3c = eng.train_grads(dev(state), dev(action), dev(R), entropy_beta=BETA).cpu().numpy()
    h = eng.workspace_tensor("h", B).cpu().numpy().reshape(B, cfgk["F"]).copy()
    V = _value(h, params)
    rows, kinds, vkinds = crafted_rows_ext(_lpa(h, params, action), V, seed=seed + 1, vcases=vcases)
    return eng, params, state, action, cfg, h, V, rows, (kinds, vkinds), a3c


def _reference(h, V, params, action, rows, kinds, vwant=VCASES):
    out = ppo.heads_from_h(h, params, action, rows, EPS, BETA, vclip=VCLIP, adv_from_row=True)
    check_cases_ext(out, rows, kinds[0], kinds[1], V, vwant=vwant)
    return out


def _check_value_term_is_the_clipped_one(out, h, params, action, rows):
    """The oracle's value_loss and cost with the clip differ from those without it by far more
    than the scalars' tolerance, so matching them is matching the clipped term."""
    plain = ppo.heads_from_h(h, params, action, rows, EPS, BETA, adv_from_row=True)["scalars"]
    for i in (0, 3):
        assert abs(out["scalars"][i] - plain[i]) > 1e-2 * max(1.0, abs(plain[i])), SCALAR_NAMES[i]


@pytest.mark.parametrize("name", sorted(HEADS))
def test_ext_heads_match_the_rules_on_the_policy_and_value_cases(name):
    cfgk, B = HEADS[name], 33                                 # a partial last workgroup of 4 waves
    eng, params, state, action, cfg, h, V, rows, kinds, a3c = _prepared(140, B, **cfgk)
    sc = eng.train_grads_ppo(dev(state), dev(action), dev(rows), EPS, entropy_beta=BETA, vclip=VCLIP,
                             adv_from_row=True)
    got_sc, ratio = sc.cpu().numpy(), eng.ratio[:B].cpu().numpy()
    assert np.array_equal(eng.workspace_tensor("h", B).cpu().numpy().reshape(B, -1), h)
    dh = eng.workspace_tensor("dh", B).cpu().numpy().reshape(B, -1)
    out = _reference(h, V, params, action, rows, kinds)
    ref_dh = out["dh"] * (h > 0) if cfgk.get("legacy") else out["dh"]
    print("dh rel %.3e, ratio rel %.3e" % (rel(dh, ref_dh), rel(ratio, out["rho"])))
    assert rel(dh, ref_dh) < GRAD_TOL
    assert rel(ratio, out["rho"]) < FWD_TOL
    _check_scalars(got_sc, out["scalars"], a3c)               # active_relus untouched
    _check_value_term_is_the_clipped_one(out, h, params, action, rows)


@pytest.mark.parametrize("B", [32, 260])
def test_ext_scalars_of_both_launch_forms(B):
    """B=32: the last heads workgroup reduces the terms; B=260: the scalars' own launch."""
    eng, params, state, action, cfg, h, V, rows, kinds, a3c = _prepared(150 + B, B, A=4, F=128, S=4)
    sc = eng.train_grads_ppo(dev(state), dev(action), dev(rows), EPS, entropy_beta=BETA, vclip=VCLIP,
                             adv_from_row=True).cpu().numpy()
    out = _reference(h, V, params, action, rows, kinds)
    _check_scalars(sc, out["scalars"], a3c)
    _check_value_term_is_the_clipped_one(out, h, params, action, rows)
    assert rel(eng.ratio[:B].cpu().numpy(), out["rho"]) < FWD_TOL


# one configuration per heads instantiation (fc_stage.ALL_HEADS_FORMS), in launch_heads' order
FORM_CASES = [dict(A=4, F=128, S=4), dict(A=4, F=512, S=1), dict(A=1, F=4, S=1), dict(A=18, F=128, S=4),
              dict(A=4, F=192, S=4), dict(A=17, F=500, S=5), dict(A=31, F=516, S=3)]
assert {heads_form(c["F"], c["A"]) for c in FORM_CASES} == ALL_HEADS_FORMS and len(FORM_CASES) == 7


@pytest.mark.parametrize("B,cfgk", [pytest.param(32, FORM_CASES[0], id="32"),
                                    pytest.param(260, FORM_CASES[0], id="260")]
                         + [pytest.param(33, c, id="A%d_F%d_S%d" % (c["A"], c["F"], c["S"]))
                            for c in FORM_CASES])    # 33: a partial last workgroup of 4 waves
def test_ext_with_both_settings_off_is_the_ppo_form_bit_for_bit(B, cfgk):
    """The plain entry is the extended one at (0, 0): the same bits from both exported symbols."""
    eng, params, state, action, cfg, h, V, rows, kinds, _ = _prepared(160 + B, B, **cfgk)
    st, ac, rw = dev(state), dev(action), dev(rows)
    _ext(eng, st, ac, rw, EPS, None, None)
    want = [eng.scalars.clone(), eng.ratio[:B].clone(), eng.grads.clone()]
    eng.grads.zero_()
    eng.ratio.zero_()
    _ext(eng, st, ac, rw, EPS, 0.0, 0)
    got = [eng.scalars.clone(), eng.ratio[:B].clone(), eng.grads.clone()]
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    # and each setting alone moves the gradient.  With one action p = 1 and dz = 0 whatever the
    # advantage is: there the row's advantage moves the policy loss and leaves the gradient's bits.
    for vclip, flags in ((VCLIP, 0), (0.0, PPO_ADV_FROM_ROW)):
        _ext(eng, st, ac, rw, EPS, vclip, flags)
        if flags and cfgk["A"] == 1:
            assert torch.equal(eng.grads, want[2]) and not torch.equal(eng.scalars, want[0])
        else:
            assert not torch.equal(eng.grads, want[2])


def test_ext_whole_gradient_matches_the_oracle_backward():
    B, cfgk = 32, dict(A=4, F=128, S=4)
    eng, params, state, action, cfg, h, V, rows, kinds, _ = _prepared(170, B, **cfgk)
    eng.train_grads_ppo(dev(state), dev(action), dev(rows), EPS, entropy_beta=BETA, vclip=VCLIP,
                        adv_from_row=True)
    got = eng.state_dict(eng.grads)
    forced, _ = gpu_decisions(eng, B)
    p64 = as64(params)
    t, _, _ = O.loss_and_grads(p64, state, action, rows[:, 0].astype(np.float64), cfg, forced=forced)
    out = _reference(t["h"], _value(t["h"], p64), p64, action, rows, kinds)
    assert out["use_clipped"].any() and not out["use_clipped"].all()
    g = O._backward_from_heads(p64, t, cfg, out["dz"], out["dV"])
    for k in g:
        e = rel(got[k], g[k])
        print("%s rel %.3e" % (k, e))
        assert e < GRAD_TOL, (k, e)


def test_all_value_clipped_batch_has_no_value_head_gradient():
    B = 32
    eng, params, state, action, cfg, h, V, rows, kinds, _ = _prepared(180, B, vcases=ALL_VALUE_CLIPPED,
                                                                       A=4, F=128, S=4)
    st, ac, rw = dev(state), dev(action), dev(rows)
    eng.train_grads_ppo(st, ac, rw, EPS, entropy_beta=BETA, vclip=VCLIP, adv_from_row=True)
    got = eng.state_dict(eng.grads)
    out = _reference(h, V, params, action, rows, kinds, vwant=ALL_VALUE_CLIPPED)
    assert out["use_clipped"].all()
    assert np.all(got["fc-v/W"] == 0.0) and np.all(got["fc-v/b"] == 0.0)
    assert rel(got["fc-pi/W"], h.astype(np.float64).T @ out["dz"]) < GRAD_TOL
    eng.train_grads_ppo(st, ac, rw, EPS, entropy_beta=BETA, adv_from_row=True)    # no clip: it is not
    assert np.any(eng.state_dict(eng.grads)["fc-v/W"] != 0.0)


def test_ext_phases_equal_the_whole_pass_bit_for_bit():
    from ba3c_amd.optimizer import AdamOptimizer
    B = 32
    eng, params, state, action, cfg, h, V, rows, kinds, _ = _prepared(190, B, A=4, F=128, S=4)
    st, ac, rw = dev(state), dev(action), dev(rows)

    def run(phases):
        eng.load_params(params)
        for ph in phases:
            eng.train_grads_ppo(st, ac, rw, EPS, entropy_beta=BETA, phase=ph, vclip=VCLIP,
                                adv_from_row=True)
        res = [eng.scalars.clone(), eng.ratio[:B].clone(), eng.grads.clone()]
        AdamOptimizer(1e-3, 0.8, 0.75, 1e-8).apply_gradients(eng, fuse_clip=True)
        res.append(eng.params.clone())
        torch.cuda.synchronize()
        return res

    whole, split = run((0,)), run((1, 2))
    assert len(whole) == len(split) == 4
    assert all(torch.equal(a, b) for a, b in zip(whole, split))
    assert eng.device_errors() == 0


def test_train_grads_is_unchanged_around_ext_calls():
    B = 32
    eng, params, state, action, cfg, h, V, rows, kinds, _ = _prepared(195, B, A=4, F=128, S=4)
    st, ac, R = dev(state), dev(action), dev(rows[:, 0].copy())
    before = (eng.train_grads(st, ac, R, entropy_beta=BETA).clone(), eng.grads.clone())
    eng.train_grads_ppo(st, ac, dev(rows), EPS, entropy_beta=BETA, vclip=VCLIP, adv_from_row=True)
    assert not torch.equal(eng.grads, before[1])
    eng.train_grads_ppo(st, ac, dev(rows), 0.3, entropy_beta=BETA, ratio=None, phase=1, vclip=0.5)
    eng.ppo_norm_adv(dev(rows))
    after = (eng.train_grads(st, ac, R, entropy_beta=BETA).clone(), eng.grads.clone())
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


# ---- the learner's loop -------------------------------------------------------------------------
E, LB, M, K, A = 24, 8, 2, 3, 18


def _loop(setting, iters=12):
    """An ActorLearner on BoxingVec run for `iters` iterations; returns it, the trainer's engine,
    the start parameters and the pool's stored rows tensors every gather read from."""
    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.boxing import BoxingVec
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    m = Model(num_actions=A, fc_neurons=128, fc_splits=4, batch_size=LB, max_batch=max(LB, E))
    m.engine.load_params(O.init_params(128, 4, A, seed=0, dtype=np.float32))
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    p0 = m.engine.params.clone()
    loop = ActorLearner(tr, n_envs=E, batch_size=LB, seed=1, env=BoxingVec(E, seed=1, limit=25),
                        ppo=setting)
    stored, gather = [], loop.pool.gather

    def watched(src, idx):
        if src.dtype == torch.float32 and src.dim() == 2 and src.shape[1] == 4:
            stored.append(src)
        return gather(src, idx)
    loop.pool.gather = watched
    loop.run(iters)
    torch.cuda.synchronize()
    return loop, m.engine, p0, stored


def test_loop_with_normalised_advantages_and_the_value_clip():
    loop, eng, p0, stored = _loop(ppo.Setting(0.2, K, M, norm_adv=True, vclip=0.2))
    assert loop.train_steps == len(loop.pool_trainer.pool_epochs) * K * M > 0
    assert torch.isfinite(loop.last_scalars).all() and not torch.equal(eng.params, p0)
    assert torch.isfinite(eng.params).all() and eng.device_errors() == 0
    assert stored and all(bool((s[:, 3] == 0).all()) for s in stored)     # the pool's rows keep 0
    mean, std = loop.pool_trainer.last_adv_stats.tolist()
    assert np.isfinite(mean) and np.isfinite(std) and std >= 0.0


def test_loop_stops_a_pool_after_one_epoch_at_a_tiny_target_kl():
    loop, eng, p0, _ = _loop(ppo.Setting(0.2, K, M, target_kl=1e-9))
    pools = len(loop.pool_trainer.pool_epochs)
    print("epochs per pool %r\nepoch KLs %r" % (loop.pool_trainer.pool_epochs, ["%.3e" % k for k in loop.pool_trainer.epoch_kls]))
    assert pools > 1 and loop.pool_trainer.pool_epochs == [1.0] * pools and loop.train_steps == pools * M


def test_loop_runs_every_epoch_at_a_huge_target_kl():
    loop, eng, p0, _ = _loop(ppo.Setting(0.2, K, M, target_kl=1e9))
    pools = len(loop.pool_trainer.pool_epochs)
    assert pools > 1 and loop.pool_trainer.pool_epochs == [float(K)] * pools and loop.train_steps == pools * K * M


def test_loop_with_the_new_fields_at_their_defaults_is_the_loop_it_was():
    a = _loop(ppo.Setting(0.2, K, M))
    b = _loop(ppo.Setting(0.2, K, M, False, 0.0, 0.0))
    assert a[0].train_steps == b[0].train_steps > 0 and a[0].pool_trainer.last_adv_stats is None
    assert torch.equal(a[1].params, b[1].params) and not torch.equal(a[1].params, a[2])


# ---- the launcher -------------------------------------------------------------------------------
def test_end_to_end_with_the_three_flags(tmp_path):
    from ba3c_amd.train import main
    out = main(("-e GridBoxing-v0 --num_actions 18 -b 32 --fc_neurons 128 --fc_splits 4 --simulator_procs 20 "
                "--max_steps 6 --send_debug_every 2 -l 0.001 --ppo_clip 0.2 --ppo_norm_adv --ppo_vclip 0.2 "
                "--ppo_target_kl 0.02").split() + ["--experiment_dir", str(tmp_path)])
    assert out["global_step"] == 6 and all(np.isfinite(v) for v in out["last"].values())
    for name in ("ppo_adv_mean", "ppo_adv_std", "ppo_epochs_run", "ppo_clip_fraction", "ppo_approx_kl"):
        rows = (tmp_path / (name + ".csv")).read_text().strip().splitlines()
        assert rows[0] == "x,y" and len(rows) >= 2, name
        assert all(np.isfinite(float(r.split(",")[1])) for r in rows[1:]), name
    p = out["ppo"]
    assert (p["clip"], p["norm_adv"], p["vclip"], p["target_kl"]) == (0.2, True, 0.2, 0.02)
    assert p["ppo_adv_std"] > 0.0 and 0.0 < p["ppo_epochs_run"] <= 4.0
