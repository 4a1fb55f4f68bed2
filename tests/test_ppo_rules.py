"""The clipped-surrogate loss's rules on the CPU (ba3c_amd.ppo): the closed-form gradient against
torch float64 autograd of the stated cost, its reduction to the A3C oracle at rho = 1 and
V_old = V, the all-clipped batch, the replay pool's order and the flags' refusals."""
import numpy as np
import pytest
import torch

from ba3c_amd import ppo
from oracle import ba3c_oracle as O

EPS = float(np.float32(0.2))       # the clip as the kernel receives it (a float32)
BETA = 0.01
MARGIN = 1e-3                      # every sample's rho is at least this far from 1 +- eps

# (sign of Adv, where rho lies): the seven cases of the policy term
CASES = [(+1, "below"), (+1, "inside"), (+1, "above"), (-1, "below"), (-1, "inside"),
         (-1, "above"), (0, "inside")]
ALL_CLIPPED = [(+1, "above"), (-1, "below")]


def crafted_rows(lpa, R, seed, eps=EPS, cases=CASES):
    """float32 rows {R, V_old, l_old, 0} that put sample n into cases[n % len(cases)], given the
    current log(p_a + 1e-6) of each sample: rho's target is drawn inside its region at least
    0.02 from 1 +- eps, and the draw is checked again after l_old's rounding to float32
    (reject and redraw: a plain random draw comes within 4e-3 of a boundary)."""
    rs = np.random.RandomState(seed)
    lpa, R = np.asarray(lpa, np.float64), np.asarray(R, np.float32)
    B = len(lpa)
    rows = np.zeros((B, 4), np.float32)
    kinds = []
    for n in range(B):
        sign, where = cases[n % len(cases)]
        lo, hi = {"below": (0.3, 1 - eps - 0.02), "inside": (1 - eps + 0.02, 1 + eps - 0.02),
                  "above": (1 + eps + 0.02, 2.0)}[where]
        while True:
            l_old = np.float32(lpa[n] - np.log(rs.uniform(lo, hi)))
            rho = np.exp(lpa[n] - np.float64(l_old))
            if lo <= rho <= hi and min(abs(rho - (1 - eps)), abs(rho - (1 + eps))) >= MARGIN:
                break
        adv = np.float32(sign * rs.uniform(0.2, 1.5))
        rows[n] = (R[n], R[n] - adv if sign else R[n], l_old, 0.0)
        kinds.append((int(np.sign(np.float64(R[n]) - np.float64(rows[n, 1]))), where))
    return rows, kinds


def check_cases(out, rows, kinds, eps=EPS, want=CASES):
    """Every sample is in the case it was built for, away from the clip boundaries."""
    rho = out["rho"]
    assert np.all(np.minimum(np.abs(rho - (1 - eps)), np.abs(rho - (1 + eps))) >= MARGIN)
    where = np.where(rho < 1 - eps, "below", np.where(rho > 1 + eps, "above", "inside"))
    adv = rows[:, 0].astype(np.float64) - rows[:, 1].astype(np.float64)
    seen = set(zip(np.sign(adv).astype(int).tolist(), where.tolist()))
    assert [(s, w) for s, w in kinds] == list(zip(np.sign(adv).astype(int).tolist(), where.tolist()))
    if len(kinds) >= len(want):
        assert seen == set(want)
    clipped = ((adv > 0) & (where == "above")) | ((adv < 0) & (where == "below"))
    assert np.array_equal(out["active"], ~clipped)


def _inputs(B, A, seed):
    rs = np.random.RandomState(seed)
    z = rs.normal(scale=1.5, size=(B, A))
    V = rs.normal(size=B)
    action = rs.randint(0, A, size=B)
    R = rs.normal(size=B).astype(np.float32)
    lpa = np.log(ppo.softmax(z) + 1e-6)[np.arange(B), action]
    return z, V, action, R, lpa


def _autograd(z, V, action, rows, eps, beta):
    f8 = lambda x: torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)
    zt, Vt = f8(z).requires_grad_(), f8(V).requires_grad_()
    R, v_old, l_old = f8(rows[:, 0]), f8(rows[:, 1]), f8(rows[:, 2])
    B = zt.shape[0]
    p = torch.softmax(zt, dim=1)
    lp = torch.log(p + 1e-6)
    lpa = lp.gather(1, torch.tensor(action, dtype=torch.int64)[:, None])[:, 0]
    adv = R - v_old
    rho = torch.exp(lpa - l_old)
    s = -torch.minimum(rho * adv, torch.clamp(rho, 1 - eps, 1 + eps) * adv)
    cost = (s.sum() + beta * (p * lp).sum() + 0.5 * ((Vt - R) ** 2).sum()) / B
    cost.backward()
    return cost.item(), zt.grad.numpy(), Vt.grad.numpy(), s.detach().numpy()


@pytest.mark.parametrize("B,A", [(37, 18), (5, 4)])
def test_closed_form_matches_autograd(B, A):
    """B=37 holds all seven cases; B=5 the first five of CASES."""
    z, V, action, R, lpa = _inputs(B, A, seed=B)
    rows, kinds = crafted_rows(lpa, R, seed=100 + B)
    out = ppo.heads_numpy(z, V, action, rows[:, 0], rows[:, 1], rows[:, 2], EPS, BETA)
    check_cases(out, rows, kinds)
    cost, dz, dV, s = _autograd(z, V, action, rows, EPS, BETA)
    assert abs(out["cost"] - cost) <= 1e-12
    assert np.abs(out["dz"] - dz).max() <= 1e-12
    assert np.abs(out["dV"] - dV).max() <= 1e-12
    assert np.abs(out["terms"][:, 0] - s).max() <= 1e-12
    Rd = rows[:, 0].astype(np.float64)
    assert np.abs(out["terms"][:, 2] - (V - Rd) ** 2).max() <= 1e-12
    assert np.abs(out["terms"][:, 3] - (V - Rd)).max() <= 1e-12


def test_adv_zero_sample_is_among_the_cases():
    z, V, action, R, lpa = _inputs(37, 18, seed=37)
    rows, kinds = crafted_rows(lpa, R, seed=137)
    assert sum(1 for s, _ in kinds if s == 0) >= 5 and np.all(rows[6::7, 0] == rows[6::7, 1])


def test_reduces_to_the_a3c_oracle_at_rho_one():
    B, A, F, S = 3, 4, 128, 4
    rs = np.random.RandomState(5)
    params = {k: v.astype(np.float64) for k, v in O.init_params(F, S, A, seed=5).items()}
    state = rs.randint(0, 256, size=(B, 84, 84, 4)).astype(np.uint8)
    action = rs.randint(0, A, size=B).astype(np.int64)
    R = rs.normal(size=B)
    cfg = {"fc_neurons": F, "fc_splits": S}
    t, _, _ = O.loss_and_grads(params, state, action, R, cfg, entropy_beta=BETA)
    V = t["pred_value"]
    lpa = t["logp"][np.arange(B), action]
    rows = np.stack([R, V, lpa, np.zeros(B)], axis=1)          # float64: rho == 1, V_old == V
    out = ppo.heads_from_h(t["h"], params, action, rows, EPS, BETA)
    assert np.all(out["rho"] == 1.0)
    assert np.abs(out["dz"] - t["dz"]).max() <= 1e-12
    assert np.abs(out["dV"] - t["dV"]).max() <= 1e-12
    assert np.abs(out["dh"] - t["dh"]).max() <= 1e-12


def test_all_clipped_batch_has_no_policy_gradient():
    B, A = 12, 6
    z, V, action, R, lpa = _inputs(B, A, seed=3)
    rows, kinds = crafted_rows(lpa, R, seed=4, cases=ALL_CLIPPED)
    out = ppo.heads_numpy(z, V, action, rows[:, 0], rows[:, 1], rows[:, 2], EPS, BETA)
    check_cases(out, rows, kinds, want=ALL_CLIPPED)
    assert not out["active"].any() and np.all(out["c"] == 0.0)
    # the entropy-only gradient: the same batch with Adv = 0
    ent = ppo.heads_numpy(z, V, action, rows[:, 0], rows[:, 0], rows[:, 2], EPS, BETA)
    assert np.array_equal(out["dz"], ent["dz"]) and np.array_equal(out["dV"], ent["dV"])
    assert np.abs(out["s"]).min() > 0            # though the loss itself is not zero


# ---- the pool ---------------------------------------------------------------------------------
def _dps(ids):
    from ba3c_amd.rollout import Datapoints
    ids = np.asarray(ids, np.int64)
    t = torch.from_numpy(ids)
    rows = torch.zeros(len(ids), 4)
    rows[:, 0] = t.float()
    z = torch.zeros(len(ids))
    return Datapoints(t.view(-1, 1).clone(), t.clone(), z, z, z.to(torch.uint8), t.to(torch.int32),
                      rows=rows)


def _host_gather(src, idx):
    return src[idx.long()]


def _drain(pool):
    out = []
    while True:
        it = pool.get()
        if it is None:
            return out
        out.append(list(it))


def test_pool_replays_the_first_arrivals():
    B, M, K = 4, 3, 2
    N = M * B
    pool = ppo.Pool(B, minibatches=M, epochs=K, seed=9, gather=_host_gather)
    pool.put(_dps(range(0, 7)))
    assert pool.get() is None and len(pool) == 7
    pool.put(_dps(range(7, 17)))                         # 17 >= N = 12: one pool, 5 left over
    pools = _drain(pool)
    assert len(pools) == 1 and len(pools[0]) == K * M and len(pool) == 5
    for k in range(K):
        epoch = pools[0][k * M:(k + 1) * M]
        for st, ac, rows in epoch:
            assert st.shape == (B, 1) and ac.shape == (B,) and rows.shape == (B, 4)
            assert np.array_equal(st[:, 0].numpy(), ac.numpy())
            assert np.array_equal(rows[:, 0].numpy(), ac.numpy().astype(np.float32))
        ids = np.concatenate([ac.numpy() for _, ac, _ in epoch])
        assert sorted(ids.tolist()) == list(range(N))     # a permutation of exactly the first N
        assert np.array_equal(ids, pool.last_perms[k])
    assert not np.array_equal(pool.last_perms[0], pool.last_perms[1])
    pool.put(_dps(range(17, 24)))                        # the 5 leftovers lead the next pool
    pools = _drain(pool)
    assert len(pools) == 1 and len(pool) == 0
    ids = np.concatenate([ac.numpy() for _, ac, _ in pools[0][:M]])
    assert sorted(ids.tolist()) == list(range(12, 24))


def test_pool_order_is_its_seeds_alone():
    def order(seed):
        pool = ppo.Pool(2, minibatches=4, epochs=3, seed=seed, gather=_host_gather)
        pool.put(_dps(range(20)))
        return [ac.numpy().tolist() for p in _drain(pool) for _, ac, _ in p]
    state = np.random.get_state()[1].copy()
    a, b, c = order(1), order(1), order(2)
    assert a == b and a != c and len(a) == 2 * 12         # two pools of 8, 4 left over
    rs = np.random.RandomState(1)
    assert a[:4] == rs.permutation(8).reshape(4, 2).tolist()
    assert np.array_equal(np.random.get_state()[1], state)   # the global generator did not move


def test_pool_refuses_datapoints_without_rows():
    from ba3c_amd.rollout import Datapoints
    z = torch.zeros(3)
    pool = ppo.Pool(2, gather=_host_gather)
    with pytest.raises(ValueError):
        pool.put(Datapoints(z, z, z, z, z, z))
    with pytest.raises(ValueError):
        ppo.Pool(2, minibatches=0)


def test_datapoints_and_batch_queue_are_unchanged_without_the_new_fields():
    from ba3c_amd.rollout import BatchQueue, Datapoints
    f = [torch.arange(5) + 10 * i for i in range(6)]
    d = Datapoints(*f)
    assert d.rows is None and len(d) == 5
    assert [getattr(d, k) for k in ("state", "action", "R", "init_R", "over", "src")] == f
    q = BatchQueue(3)
    q.put(d)
    q.put(Datapoints(*f))
    b = q.get()
    assert isinstance(b, list) and len(b) == 5
    assert all(torch.equal(x, y[:3]) for x, y in zip(b, f))
    b = q.get()
    assert len(b) == 5 and torch.equal(b[0], torch.cat([f[0][3:], f[0][:1]]))
    assert torch.equal(q.get()[1], f[1][1:4])
    assert q.get() is None and len(q) == 1


def test_metrics_of_a_ratio():
    rho = np.array([1.0, 1.3, 0.7, 1.1], np.float32)
    assert ppo.clip_fraction(rho, 0.2) == 0.5
    assert abs(ppo.approx_kl(rho) + np.log(rho.astype(np.float64)).mean()) < 1e-15


# ---- the flags --------------------------------------------------------------------------------
def _resolve(*argv):
    from ba3c_amd.flags import build_parser, resolve
    return resolve(build_parser().parse_args(list(argv)))


def test_ppo_is_off_without_its_flags():
    a = _resolve()
    assert a.ppo is None and a.ppo_clip == 0.0 and a.ppo_epochs is None and a.ppo_minibatches is None
    a = _resolve("-e", "GridBoxing-v0", "--num_actions", "18", "--self_play")
    assert a.ppo is None


def test_ppo_setting_and_defaults():
    a = _resolve("--ppo_clip", "0.2")
    assert a.ppo == ppo.Setting(clip=0.2, epochs=4, minibatches=4)
    a = _resolve("--ppo_clip", "0.1", "--ppo_epochs", "2", "--ppo_minibatches", "8", "-e",
                 "GridBoxing-v0", "--num_actions", "18", "--self_play")
    assert a.ppo == ppo.Setting(clip=0.1, epochs=2, minibatches=8)


@pytest.mark.parametrize("argv,word", [
    (("--ppo_clip", "-0.1"), "--ppo_clip"),
    (("--ppo_clip", "1.0"), "--ppo_clip"),
    (("--ppo_clip", "1.5"), "--ppo_clip"),
    (("--ppo_clip", "nan"), "--ppo_clip"),
    (("--ppo_epochs", "2"), "--ppo_epochs needs"),
    (("--ppo_minibatches", "2"), "--ppo_minibatches needs"),
    (("--ppo_clip", "0", "--ppo_epochs", "2"), "--ppo_epochs needs"),
    (("--ppo_clip", "0.2", "--ppo_epochs", "0"), "--ppo_epochs 0"),
    (("--ppo_clip", "0.2", "--ppo_minibatches", "-1"), "--ppo_minibatches -1"),
    (("--ppo_clip", "0.2", "--ppo_minibatches", "300", "-b", "2048"), "16 GiB"),
    (("--ppo_clip", "0.2", "--dummy", "1"), "--dummy"),
])
def test_resolve_refuses(argv, word):
    with pytest.raises(SystemExit) as e:
        _resolve(*argv)
    assert word in str(e.value)
