"""The clipped-surrogate (PPO) heads, ba3c_train_grads_ppo's phases, ba3c_sample_logp and the
replaying loop on the GPU, held to ba3c_amd.ppo (float64) with test_gpu_parity's bounds."""
import numpy as np
import pytest
import torch

from ba3c_amd import ppo
from ba3c_amd._lib import SCALAR_NAMES
from oracle import ba3c_oracle as O
from test_gpu_parity import FWD_TOL, GRAD_TOL, as64, case, dev, engine, gpu_decisions, rel
from test_ppo_rules import ALL_CLIPPED, BETA, CASES, EPS, check_cases, crafted_rows

pytestmark = pytest.mark.gpu

HEADS = {
    "A4_F128": dict(A=4, F=128, S=4),                       # every load up front (the PRE path)
    "A18_F128": dict(A=18, F=128, S=4),                     # runtime action count
    "A6_F1024": dict(A=6, F=1024, S=4),                     # the runtime loop over features
    "legacy": dict(A=18, F=256, S=1, legacy=True, ps=4),    # --use_normal_fc: bias + ReLU FC
}


def _lpa(h, params, action):
    z = h.astype(np.float64) @ params["fc-pi/W"].astype(np.float64) + params["fc-pi/b"].astype(np.float64)
    return np.log(ppo.softmax(z) + 1e-6)[np.arange(len(action)), action]


def _prepared(seed, B, cases=CASES, **cfgk):
    """An engine that has run the A3C pass on a fresh case, the case, the GPU's own h and rows
    crafted on it (h does not depend on the loss)."""
    params, state, action, R, cfg = case(seed, B, **cfgk)
    eng = engine(max_batch=max(64, B), **cfgk)
    eng.load_params(params)
    a3c = eng.train_grads(dev(state), dev(action), dev(R), entropy_beta=BETA).cpu().numpy()
    h = eng.workspace_tensor("h", B).cpu().numpy().reshape(B, cfgk["F"]).copy()
    rows, kinds = crafted_rows(_lpa(h, params, action), R, seed=seed + 1, cases=cases)
    return eng, params, state, action, cfg, h, rows, kinds, a3c


def _check_scalars(got, ref, a3c):
    for i, name in enumerate(SCALAR_NAMES[:7]):
        print("scalar %s: gpu %.9g oracle %.9g" % (name, got[i], ref[i]))
        assert abs(got[i] - ref[i]) <= 1e-4 * max(1.0, abs(ref[i])), (name, got[i], ref[i])
    assert got[7] == a3c[7]                                   # active_relus: not the loss's


@pytest.mark.parametrize("name", sorted(HEADS))
def test_heads_match_the_rules_on_the_seven_cases(name):
    cfgk, B = HEADS[name], 33                                 # a partial last workgroup of 4 waves
    eng, params, state, action, cfg, h, rows, kinds, a3c = _prepared(40, B, **cfgk)
    sc = eng.train_grads_ppo(dev(state), dev(action), dev(rows), EPS, entropy_beta=BETA)
    got_sc, ratio = sc.cpu().numpy(), eng.ratio[:B].cpu().numpy()
    assert np.array_equal(eng.workspace_tensor("h", B).cpu().numpy().reshape(B, -1), h)
    dh = eng.workspace_tensor("dh", B).cpu().numpy().reshape(B, -1)
    out = ppo.heads_from_h(h, params, action, rows, EPS, BETA)
    check_cases(out, rows, kinds)
    ref_dh = out["dh"] * (h > 0) if cfgk.get("legacy") else out["dh"]
    print("dh rel %.3e, ratio rel %.3e" % (rel(dh, ref_dh), rel(ratio, out["rho"])))
    assert rel(dh, ref_dh) < GRAD_TOL
    assert rel(ratio, out["rho"]) < FWD_TOL
    _check_scalars(got_sc, out["scalars"], a3c)


@pytest.mark.parametrize("B", [32, 260])
def test_scalars_of_both_launch_forms(B):
    """B=32: the last heads workgroup reduces the terms; B=260: the scalars' own launch."""
    eng, params, state, action, cfg, h, rows, kinds, a3c = _prepared(50 + B, B, A=4, F=128, S=4)
    sc = eng.train_grads_ppo(dev(state), dev(action), dev(rows), EPS, entropy_beta=BETA).cpu().numpy()
    out = ppo.heads_from_h(h, params, action, rows, EPS, BETA)
    check_cases(out, rows, kinds)
    _check_scalars(sc, out["scalars"], a3c)
    assert rel(eng.ratio[:B].cpu().numpy(), out["rho"]) < FWD_TOL


@pytest.mark.parametrize("B", [32, 160])
def test_whole_gradient_matches_the_oracle_backward(B):
    cfgk = dict(A=4, F=128, S=4)
    eng, params, state, action, cfg, h, rows, kinds, _ = _prepared(60 + B, B, **cfgk)
    eng.train_grads_ppo(dev(state), dev(action), dev(rows), EPS, entropy_beta=BETA)
    got = eng.state_dict(eng.grads)
    forced, _ = gpu_decisions(eng, B)
    p64 = as64(params)
    t, _, _ = O.loss_and_grads(p64, state, action, rows[:, 0].astype(np.float64), cfg, forced=forced)
    out = ppo.heads_from_h(t["h"], p64, action, rows, EPS, BETA)
    check_cases(out, rows, kinds)
    g = O._backward_from_heads(p64, t, cfg, out["dz"], out["dV"])
    for k in g:
        e = rel(got[k], g[k])
        print("%s rel %.3e" % (k, e))
        assert e < GRAD_TOL, (k, e)


def test_rho_one_is_the_a3c_gradient():
    """rows from the forward's own value and sample_logp's logp: rho == 1 up to the float32
    rounding of l_old, V_old == V up to the value's, so every gradient tensor is train_grads'."""
    B = 32
    params, state, _, R, cfg = case(70, B, A=4, F=128, S=4)
    eng = engine(A=4, F=128, S=4)
    eng.load_params(params)
    probs, probsT, value = eng.forward(dev(state))
    u = dev(np.random.RandomState(1).random_sample(B))
    action, logp, flag = eng.sample_logp(probsT, probs, u)
    rows = torch.stack([dev(R), value, logp, torch.zeros_like(value)], dim=1).contiguous()
    eng.train_grads(dev(state), action, dev(R), entropy_beta=BETA)
    ref = eng.state_dict(eng.grads)
    eng.train_grads_ppo(dev(state), action, rows, EPS, entropy_beta=BETA)
    got = eng.state_dict(eng.grads)
    ratio = eng.ratio[:B].cpu().numpy()
    worst = max(rel(got[k], ref[k]) for k in ref)
    print("rho == 1: worst gradient rel %.3e, max |rho - 1| %.3e" % (worst, np.abs(ratio - 1).max()))
    assert int(flag.item()) == 0 and np.abs(ratio - 1).max() < FWD_TOL
    for k in ref:
        assert rel(got[k], ref[k]) < GRAD_TOL, k


def test_all_clipped_batch_leaves_the_entropy_gradient():
    B = 32
    eng, params, state, action, cfg, h, rows, kinds, _ = _prepared(80, B, cases=ALL_CLIPPED, A=4, F=128, S=4)
    eng.train_grads_ppo(dev(state), dev(action), dev(rows), EPS, entropy_beta=BETA)
    got = eng.state_dict(eng.grads)
    out = ppo.heads_from_h(h, params, action, rows, EPS, BETA)
    check_cases(out, rows, kinds, want=ALL_CLIPPED)
    assert not out["active"].any()
    ent_rows = rows.copy()
    ent_rows[:, 1] = ent_rows[:, 0]                           # Adv = 0: the entropy term alone
    ent = ppo.heads_from_h(h, params, action, ent_rows, EPS, BETA)
    h64 = h.astype(np.float64)
    assert rel(got["fc-pi/W"], h64.T @ ent["dz"]) < GRAD_TOL
    assert rel(got["fc-pi/b"], ent["dz"].sum(axis=0)) < GRAD_TOL


def test_phases_equal_the_whole_pass_bit_for_bit():
    from ba3c_amd.optimizer import AdamOptimizer
    B = 32
    eng, params, state, action, cfg, h, rows, kinds, _ = _prepared(90, B, A=4, F=128, S=4)
    st, ac, rw = dev(state), dev(action), dev(rows)

    def run(phases):
        eng.load_params(params)
        for ph in phases:
            eng.train_grads_ppo(st, ac, rw, EPS, entropy_beta=BETA, phase=ph)
        res = [eng.scalars.clone(), eng.ratio[:B].clone(), eng.grads.clone()]
        AdamOptimizer(1e-3, 0.8, 0.75, 1e-8).apply_gradients(eng, fuse_clip=True)
        res.append(eng.params.clone())
        torch.cuda.synchronize()
        return res

    whole, split = run((0,)), run((1, 2))
    assert len(whole) == len(split) == 4
    assert all(torch.equal(a, b) for a, b in zip(whole, split))
    assert eng.device_errors() == 0


def test_train_grads_is_unchanged_around_ppo_calls():
    B = 32
    eng, params, state, action, cfg, h, rows, kinds, _ = _prepared(95, B, A=4, F=128, S=4)
    st, ac, R = dev(state), dev(action), dev(rows[:, 0].copy())
    before = (eng.train_grads(st, ac, R, entropy_beta=BETA).clone(), eng.grads.clone())
    eng.train_grads_ppo(st, ac, dev(rows), EPS, entropy_beta=BETA)
    assert not torch.equal(eng.grads, before[1])
    eng.train_grads_ppo(st, ac, dev(rows), 0.3, entropy_beta=BETA, ratio=None, phase=1)
    after = (eng.train_grads(st, ac, R, entropy_beta=BETA).clone(), eng.grads.clone())
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


@pytest.mark.parametrize("A", [1, 4, 18, 31])
@pytest.mark.parametrize("B", [1, 100, 1000])
def test_sample_logp_is_sample_plus_the_log(A, B):
    eng = engine()
    rs = np.random.RandomState(A * 1000 + B)
    probs = O.softmax(rs.normal(scale=2.0, size=(B, A))).astype(np.float32)
    pi = O.softmax(rs.normal(scale=2.0, size=(B, A))).astype(np.float32)
    if B > 1:
        probs[B // 2] *= np.float32(1.01)                     # a row that does not sum to 1: flag 2
    u = rs.random_sample(B)
    for recorded in (probs, pi):
        a0, f0 = eng.sample(dev(probs), dev(u))
        a1, logp, f1 = eng.sample_logp(dev(probs), dev(recorded), dev(u))
        assert torch.equal(a0, a1) and torch.equal(f0, f1) and int(f0.item()) == (2 if B > 1 else 0)
        a = np.minimum(a1.cpu().numpy(), A - 1)
        want = np.log(recorded[np.arange(B), a].astype(np.float64) + 1e-6).astype(np.float32)
        got = logp.cpu().numpy()
        assert got.dtype == np.float32 and np.all(np.abs(got - want) <= np.spacing(np.abs(want)))


def _counted(monkeypatch):
    """Count the engine's calls of the two PPO entry points and keep each step's ratio."""
    from ba3c_amd.engine import Ba3cEngine
    calls = {"train_grads_ppo": 0, "sample_logp": 0, "ratios": []}
    grads, sample = Ba3cEngine.train_grads_ppo, Ba3cEngine.sample_logp

    def train_grads_ppo(self, state, *a, **kw):
        calls["train_grads_ppo"] += 1
        out = grads(self, state, *a, **kw)
        calls["ratios"].append(self.ratio[:state.shape[0]].clone())
        return out

    def sample_logp(self, *a, **kw):
        calls["sample_logp"] += 1
        return sample(self, *a, **kw)

    monkeypatch.setattr(Ba3cEngine, "train_grads_ppo", train_grads_ppo)
    monkeypatch.setattr(Ba3cEngine, "sample_logp", sample_logp)
    return calls


E2E = ("-e GridBreakout-v0 -b 32 --fc_neurons 128 --fc_splits 4 --simulator_procs 20 --max_steps 12 "
       "--send_debug_every 4 -l 0.001").split()


def test_end_to_end_replays_each_pool(tmp_path, monkeypatch):
    from ba3c_amd.train import main
    calls = _counted(monkeypatch)
    out = main(E2E + ["--ppo_clip", "0.2", "--ppo_epochs", "2", "--ppo_minibatches", "2",
                      "--experiment_dir", str(tmp_path)])
    assert out["global_step"] == 12 and calls["train_grads_ppo"] == 12
    assert calls["sample_logp"] == out["simulator_steps"] > 0
    assert all(np.isfinite(v) for v in out["last"].values())
    ratios = [r.cpu().numpy() for r in calls["ratios"]]
    assert all(r.shape == (32,) and np.isfinite(r).all() for r in ratios)
    print("first minibatch max |rho - 1| %.3e; second epoch's %.3e"
          % (np.abs(ratios[0] - 1).max(), np.abs(ratios[2] - 1).max()))
    assert np.abs(ratios[0] - 1).max() < 1e-5                 # the behaviour policy is the learner
    assert any(np.any(r != 1) for r in ratios[2:4])           # the pool's second epoch: it has moved
    for name in ("ppo_clip_fraction", "ppo_approx_kl"):
        rows = (tmp_path / (name + ".csv")).read_text().strip().splitlines()
        assert rows[0] == "x,y" and len(rows) == 1 + 3        # one row per flush of 4 steps
        assert all(np.isfinite(float(r.split(",")[1])) for r in rows[1:])
    assert out["ppo"]["clip"] == 0.2 and 0.0 <= out["ppo"]["ppo_clip_fraction"] <= 1.0


def test_end_to_end_without_the_flags_calls_no_ppo_entry(tmp_path, monkeypatch):
    from ba3c_amd.train import main
    calls = _counted(monkeypatch)
    out = main(E2E + ["--experiment_dir", str(tmp_path)])
    assert out["global_step"] >= 12 and "ppo" not in out
    assert calls["train_grads_ppo"] == 0 and calls["sample_logp"] == 0
    assert not (tmp_path / "ppo_clip_fraction.csv").exists()


def test_end_to_end_through_the_bucketed_sync_step(tmp_path, monkeypatch):
    """--use_sync -g 1 (the README's flags): every step is the N>1 step's two phases, both
    through the PPO entry point."""
    from ba3c_amd.train import main
    calls = _counted(monkeypatch)
    out = main(E2E + ["-o", "adam", "--use_sync", "-g", "1", "--max_steps", "4", "--ppo_clip", "0.2",
                      "--ppo_epochs", "2", "--ppo_minibatches", "2", "--experiment_dir", str(tmp_path)])
    assert out["global_step"] == 4 and calls["train_grads_ppo"] == 8
    assert all(np.isfinite(v) for v in out["last"].values())
    assert np.abs(calls["ratios"][0].cpu().numpy() - 1).max() < 1e-5
    assert torch.equal(calls["ratios"][0], calls["ratios"][1])    # phase 2 runs no heads


def test_capture_refuses_a_ppo_step():
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    m = Model(num_actions=4, fc_neurons=128, fc_splits=4, batch_size=4, max_batch=16)
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    st = torch.zeros(4, 84, 84, 4, dtype=torch.uint8, device="cuda")
    ac = torch.zeros(4, dtype=torch.int64, device="cuda")
    rows = torch.zeros(4, 4, device="cuda")
    with pytest.raises(ValueError):
        tr.capture_step(st, ac, None, rows=rows, clip=0.2)
    with pytest.raises(ValueError):
        tr.train_step(st, ac, None, rows=rows)
