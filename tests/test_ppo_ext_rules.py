"""The rules of the PPO loss's three optional pieces on the CPU (ba3c_amd.ppo): per-minibatch
advantage normalisation, the clipped value loss against torch float64 autograd of the stated cost,
the bit-for-bit equalities with the plain clipped-surrogate loss, the KL stop and the flags."""
import numpy as np
import pytest
import torch

from ba3c_amd import ppo
from test_ppo_rules import BETA, CASES, EPS, MARGIN, _inputs, crafted_rows

VCLIP = float(np.float32(0.2))     # the value clip as the kernel receives it (a float32)

# where d = V - V_old lies against +-vclip, and where R lies: the five cases of the value term
VCASES = ["above_clipped",         # d > vclip, R beyond V: the clipped square is larger, dV = 0
          "above_unclipped",       # d > vclip, R below Vc: the unclipped square is larger
          "below_clipped",         # the two mirror cases, d < -vclip
          "below_unclipped",
          "inside"]                # |d| < vclip
ALL_VALUE_CLIPPED = ["above_clipped", "below_clipped"]


def value_case(V, R, v_old, vclip=VCLIP):
    """(case name, | |d| - vclip |, |(V-R)^2 - (Vc-R)^2|) of one sample, in float64."""
    V, R, v_old = float(V), float(R), float(v_old)
    d = V - v_old
    if abs(d) <= vclip:
        return "inside", abs(abs(d) - vclip), None
    Vc = v_old + np.sign(d) * vclip
    gap = (Vc - R) ** 2 - (V - R) ** 2
    side = "above" if d > 0 else "below"
    return side + ("_clipped" if gap > 0 else "_unclipped"), abs(abs(d) - vclip), abs(gap)


def crafted_rows_ext(lpa, V, seed, eps=EPS, vclip=VCLIP, cases=CASES, vcases=VCASES):
    """float32 rows {R, V_old, l_old, Adv} that put sample n into policy case cases[n % len(cases)]
    (by l_old and the row's own advantage, as test_ppo_rules.crafted_rows builds them) and into
    value case vcases[n % len(vcases)] (by V_old and R around the sample's current value V).
    Every |d| is at least MARGIN from vclip and every non-tie difference of the two squares at
    least MARGIN, checked after the rounding of R and V_old to float32 (reject and redraw)."""
    lpa, V = np.asarray(lpa, np.float64), np.asarray(V, np.float64)
    B = len(lpa)
    base, kinds = crafted_rows(lpa, np.zeros(B, np.float32), seed=seed, eps=eps, cases=cases)
    rows = np.zeros((B, 4), np.float32)
    rows[:, 2] = base[:, 2]
    rows[:, 3] = -base[:, 1]                        # base is {0, 0 - adv, l_old, 0}: exact
    rs = np.random.RandomState(seed + 7919)
    vkinds = []
    for n in range(B):
        want = vcases[n % len(vcases)]
        while True:
            if want == "inside":
                v_old = V[n] + rs.uniform(-(vclip - 0.05), vclip - 0.05)
                R = V[n] + rs.normal()
            else:
                up = want.startswith("above")
                v_old = V[n] - (1 if up else -1) * rs.uniform(vclip + 0.05, 1.0)
                Vc = v_old + (1 if up else -1) * vclip
                away = rs.uniform(0.1, 1.0)
                if want.endswith("_clipped"):       # R on V's far side
                    R = V[n] + (away if up else -away)
                else:                               # R on Vc's far side
                    R = Vc - (away if up else -away)
            R, v_old = np.float32(R), np.float32(v_old)
            got, dm, gap = value_case(V[n], R, v_old, vclip)
            if got == want and dm >= MARGIN and (gap is None or gap >= MARGIN):
                break
        rows[n, 0], rows[n, 1] = R, v_old
        vkinds.append(want)
    return rows, kinds, vkinds


def check_cases_ext(out, rows, kinds, vkinds, V, eps=EPS, vclip=VCLIP, want=CASES, vwant=VCASES):
    """Every sample is in the policy and the value case it was built for, away from the
    boundaries, and use_clipped / active say so."""
    rho = out["rho"]
    assert np.all(np.minimum(np.abs(rho - (1 - eps)), np.abs(rho - (1 + eps))) >= MARGIN)
    where = np.where(rho < 1 - eps, "below", np.where(rho > 1 + eps, "above", "inside"))
    adv = rows[:, 3].astype(np.float64)
    seen = list(zip(np.sign(adv).astype(int).tolist(), where.tolist()))
    assert [(s, w) for s, w in kinds] == seen
    if len(kinds) >= len(want):
        assert set(seen) == set(want)
    clipped = ((adv > 0) & (where == "above")) | ((adv < 0) & (where == "below"))
    assert np.array_equal(out["active"], ~clipped)
    got = [value_case(V[n], rows[n, 0], rows[n, 1], vclip) for n in range(len(V))]
    assert [g[0] for g in got] == list(vkinds)
    assert all(g[1] >= MARGIN and (g[2] is None or g[2] >= MARGIN) for g in got)
    if len(vkinds) >= len(vwant):
        assert set(vkinds) == set(vwant)
    assert np.array_equal(out["use_clipped"], np.array([k.endswith("_clipped") for k in vkinds]))


# ---- the normalisation --------------------------------------------------------------------------
def test_normalise_hand_worked():
    rows = ppo.make_rows([3.0, 1.0, 4.0, 0.0], [1.0, 1.0, 0.0, 2.0], [0.5, 0.25, -1.0, -2.0])
    out, mean, std = ppo.normalise_adv_numpy(rows)      # Adv = 2, 0, 4, -2: mean 1, var 5
    assert mean == 1.0 and abs(std - np.sqrt(5.0)) <= 1e-15
    want = (np.array([1.0, -1.0, 3.0, -3.0]) / (np.sqrt(5.0) + 1e-8)).astype(np.float32)
    assert out.dtype == np.float32 and np.array_equal(out[:, 3], want)
    assert np.array_equal(out[:, :3], rows[:, :3]) and np.all(rows[:, 3] == 0)   # a copy


def test_normalise_edge_batches():
    out, mean, std = ppo.normalise_adv_numpy(ppo.make_rows([2.5], [1.0], [0.0]))
    assert out[0, 3] == 0.0 and mean == 1.5 and std == 0.0
    R = np.full(33, 0.7, np.float32)
    out, mean, std = ppo.normalise_adv_numpy(ppo.make_rows(R, R - np.float32(0.3), np.zeros(33)))
    assert np.abs(out[:, 3]).max() <= 1e-6
    rs = np.random.RandomState(0)
    rows = rs.normal(size=(257, 4)).astype(np.float32)
    out, mean, std = ppo.normalise_adv_numpy(rows)
    a = out[:, 3].astype(np.float64)
    assert abs(a.mean()) <= 1e-7 and abs(a.std() - 1.0) <= 1e-6
    assert out[:, :3].tobytes() == rows[:, :3].tobytes()
    adv = rows[:, 0].astype(np.float64) - rows[:, 1].astype(np.float64)
    assert abs(mean - adv.mean()) <= 1e-12 and abs(std - adv.std()) <= 1e-12


# ---- the closed form ----------------------------------------------------------------------------
def _autograd_ext(z, V, action, rows, eps, beta, vclip):
    f8 = lambda x: torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)
    zt, Vt = f8(z).requires_grad_(), f8(V).requires_grad_()
    R, v_old, l_old, adv = f8(rows[:, 0]), f8(rows[:, 1]), f8(rows[:, 2]), f8(rows[:, 3])
    B = zt.shape[0]
    p = torch.softmax(zt, dim=1)
    lp = torch.log(p + 1e-6)
    lpa = lp.gather(1, torch.tensor(action, dtype=torch.int64)[:, None])[:, 0]
    rho = torch.exp(lpa - l_old)
    s = -torch.minimum(rho * adv, torch.clamp(rho, 1 - eps, 1 + eps) * adv)
    Vc = v_old + torch.clamp(Vt - v_old, -vclip, vclip)
    vsq = torch.maximum((Vt - R) ** 2, (Vc - R) ** 2)
    cost = (s.sum() + beta * (p * lp).sum() + 0.5 * vsq.sum()) / B
    cost.backward()
    return cost.item(), zt.grad.numpy(), Vt.grad.numpy(), s.detach().numpy(), vsq.detach().numpy()


@pytest.mark.parametrize("B,A", [(37, 18), (5, 4)])
def test_closed_form_with_vclip_matches_autograd(B, A):
    """B=37 holds all seven policy cases and (35 = 7 x 5) every pair with the five value cases;
    B=5 the first five of each."""
    z, V, action, _, lpa = _inputs(B, A, seed=B)
    rows, kinds, vkinds = crafted_rows_ext(lpa, V, seed=200 + B)
    out = ppo.heads_numpy(z, V, action, rows[:, 0], rows[:, 1], rows[:, 2], EPS, BETA, vclip=VCLIP,
                          adv=rows[:, 3])
    check_cases_ext(out, rows, kinds, vkinds, V)
    if B >= 35:
        assert len(set(zip(kinds, vkinds))) == 35
    cost, dz, dV, s, vsq = _autograd_ext(z, V, action, rows, EPS, BETA, VCLIP)
    assert abs(out["cost"] - cost) <= 1e-12
    assert np.abs(out["dz"] - dz).max() <= 1e-12
    assert np.abs(out["dV"] - dV).max() <= 1e-12
    assert np.abs(out["terms"][:, 0] - s).max() <= 1e-12
    assert np.abs(out["terms"][:, 2] - vsq).max() <= 1e-12
    Rd = rows[:, 0].astype(np.float64)
    assert np.abs(out["terms"][:, 3] - (V - Rd)).max() <= 1e-12           # term 3 stays V - R
    uc = out["use_clipped"]
    assert np.all(out["dV"][uc] == 0.0) and np.all(out["dV"][~uc] == ((V - Rd) / B)[~uc])
    assert abs(out["scalars"][3] - 0.5 * vsq.sum() * 128.0 / B) <= 1e-12
    # through heads_from_h's row: the same numbers
    F = 6
    rs = np.random.RandomState(B)
    params = {"fc-pi/W": rs.normal(size=(F, A)), "fc-pi/b": rs.normal(size=A),
              "fc-v/W": rs.normal(size=(F, 1)), "fc-v/b": rs.normal(size=1)}
    h = rs.normal(size=(B, F))
    a = ppo.heads_from_h(h, params, action, rows, EPS, BETA, vclip=VCLIP, adv_from_row=True)
    b = ppo.heads_numpy(h @ params["fc-pi/W"] + params["fc-pi/b"], a["V"], action, rows[:, 0],
                        rows[:, 1], rows[:, 2], EPS, BETA, VCLIP, rows[:, 3].astype(np.float64))
    assert np.array_equal(a["dz"], b["dz"]) and np.array_equal(a["dV"], b["dV"])
    assert np.array_equal(a["dh"], a["dz"] @ params["fc-pi/W"].T + a["dV"][:, None] @ params["fc-v/W"].T)


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_the_defaults_are_the_plain_loss_bit_for_bit():
    B, A = 37, 18
    z, V, action, R, lpa = _inputs(B, A, seed=11)
    rows, _ = crafted_rows(lpa, R, seed=12)
    args = (z, V, action, rows[:, 0], rows[:, 1], rows[:, 2], EPS, BETA)
    plain = ppo.heads_numpy(*args)
    assert not plain["use_clipped"].any()
    _same(plain, ppo.heads_numpy(*args, vclip=0.0, adv=None))
    _same(plain, ppo.heads_numpy(*args, adv=rows[:, 0].astype(np.float64) - rows[:, 1].astype(np.float64)))
    big = 2.0 * np.abs(V - rows[:, 1].astype(np.float64)).max()
    _same(plain, ppo.heads_numpy(*args, vclip=big))
    assert not np.array_equal(plain["dV"], ppo.heads_numpy(*args, vclip=1e-3)["dV"])   # the clip bites


def test_all_value_clipped_batch_has_no_value_gradient():
    B, A = 12, 6
    z, V, action, _, lpa = _inputs(B, A, seed=3)
    rows, kinds, vkinds = crafted_rows_ext(lpa, V, seed=4, vcases=ALL_VALUE_CLIPPED)
    args = (z, V, action, rows[:, 0], rows[:, 1], rows[:, 2], EPS, BETA)
    out = ppo.heads_numpy(*args, vclip=VCLIP, adv=rows[:, 3])
    check_cases_ext(out, rows, kinds, vkinds, V, vwant=ALL_VALUE_CLIPPED)
    assert out["use_clipped"].all() and np.all(out["dV"] == 0.0)
    plain = ppo.heads_numpy(*args, adv=rows[:, 3])
    assert np.array_equal(out["dz"], plain["dz"]) and np.all(plain["dV"] != 0.0)
    assert np.all(out["terms"][:, 2] > plain["terms"][:, 2])       # the larger square is the loss


# ---- the KL stop, the setting, the flags --------------------------------------------------------
def test_should_stop():
    assert not ppo.should_stop(5.0, 0) and not ppo.should_stop(float("nan"), 0.0)
    assert not ppo.should_stop(0.01, 0.02) and not ppo.should_stop(0.02, 0.02)
    assert ppo.should_stop(0.020001, 0.02)
    assert ppo.should_stop(float("nan"), 0.02) and ppo.should_stop(float("inf"), 0.02)
    assert not ppo.should_stop(float("-inf"), 0.02)


def test_stop_kl_is_never_negative():
    rho = np.array([1.0, 1.3, 0.7, 1.1], np.float32)
    r = rho.astype(np.float64)
    assert abs(ppo.stop_kl(rho) - ((r - 1) - np.log(r)).mean()) < 1e-15 and ppo.stop_kl(np.ones(5)) == 0.0
    # a batch whose mean(-log rho) is negative still has a positive stop estimate
    up = np.array([1.02, 1.01, 0.995], np.float32)
    assert ppo.approx_kl(up) < 0 < ppo.stop_kl(up)
    assert not ppo.should_stop(ppo.stop_kl(np.ones(5)), 1e-9) and ppo.should_stop(ppo.stop_kl(up), 1e-9)
    rs = np.random.RandomState(0)
    small = np.exp(1e-3 * rs.normal(size=1000))
    assert abs(ppo.stop_kl(small) / (0.5 * (np.log(small) ** 2).mean()) - 1) < 1e-2   # ~ (log rho)^2 / 2


def _resolve(*argv):
    from ba3c_amd.flags import build_parser, resolve
    return resolve(build_parser().parse_args(list(argv)))


def test_setting_defaults():
    s = ppo.Setting(clip=0.2, epochs=4, minibatches=4)
    assert (s.norm_adv, s.vclip, s.target_kl) == (False, 0.0, 0.0)
    assert s == ppo.Setting(0.2, 4, 4, False, 0.0, 0.0) and s == (0.2, 4, 4, False, 0.0, 0.0)
    assert _resolve("--ppo_clip", "0.2").ppo == s
    assert _resolve().ppo is None
    a = _resolve("--ppo_clip", "0.1", "--ppo_norm_adv", "--ppo_vclip", "0.3", "--ppo_target_kl", "0.02",
                 "--ppo_epochs", "2")
    assert a.ppo == ppo.Setting(clip=0.1, epochs=2, minibatches=4, norm_adv=True, vclip=0.3,
                                target_kl=0.02)
    assert _resolve("--ppo_clip", "0.2", "--ppo_vclip", "0", "--ppo_target_kl", "0").ppo == s


@pytest.mark.parametrize("argv,word", [
    (("--ppo_norm_adv",), "--ppo_norm_adv needs"),
    (("--ppo_vclip", "0.2"), "--ppo_vclip needs"),
    (("--ppo_target_kl", "0.02"), "--ppo_target_kl needs"),
    (("--ppo_clip", "0", "--ppo_norm_adv"), "--ppo_norm_adv needs"),
    (("--ppo_clip", "0.2", "--ppo_vclip", "-0.1"), "--ppo_vclip"),
    (("--ppo_clip", "0.2", "--ppo_vclip", "nan"), "--ppo_vclip"),
    (("--ppo_clip", "0.2", "--ppo_vclip", "inf"), "--ppo_vclip"),
    (("--ppo_clip", "0.2", "--ppo_target_kl", "-1"), "--ppo_target_kl"),
    (("--ppo_clip", "0.2", "--ppo_target_kl", "nan"), "--ppo_target_kl"),
    (("--ppo_clip", "0.2", "--ppo_target_kl", "inf"), "--ppo_target_kl"),
])
def test_resolve_refuses(argv, word):
    with pytest.raises(SystemExit) as e:
        _resolve(*argv)
    assert word in str(e.value)


def test_target_kl_is_single_replica():
    from ba3c_amd.train import check_distributed
    a = _resolve("--ppo_clip", "0.2", "--ppo_target_kl", "0.02", "--use_sync", "-g", "2")
    with pytest.raises(SystemExit) as e:
        check_distributed(a, 2)
    assert "--ppo_target_kl" in str(e.value)
    check_distributed(_resolve("--ppo_clip", "0.2", "--ppo_norm_adv", "--use_sync", "-g", "2"), 2)
