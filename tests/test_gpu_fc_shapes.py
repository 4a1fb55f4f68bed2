"""fc1 and the heads at every tile edge of F, A, S and B, held to float64 product by product.

ba3c_create accepts any fc_neurons that is a multiple of 4 x the fc1 tensor count and any
num_actions in 1..31; the rest of the suite runs the FC stage at F in {128, 256, 512, 1024} and
A in {4, 6, 18} only, all multiples of 64 that fill every tile.  The thirteen geometries of
fc_stage.GEOMETRIES are each the smallest case of a code path that those never reach: the
seven heads_kernel forms of launch_heads, the 64-lane feature tails of heads_sample, the four
exits of wave_reduce_d, the N / K / M tails of FcFwd, FcDgrad and BatchWgrad on both tile
sizes, split boundaries that are no multiple of 32, the legacy bias row, and the C = 12 path's
separate launches (tests/test_fc_stage.py asserts that coverage on the host).

One case is one engine, one training pass and one forward.  Each product is compared with the
float64 product of THE GPU'S OWN inputs (its a3 for h, its h for the loss and dh, its dh and a3
for dY3 and the fc1 gradients), so no convolution is evaluated on the CPU, no pooling decision
can differ, and an error is pinned to the one kernel that made it.  Two checks per product:
element-wise within the error model of fc_stage (derived there, not measured; it sees one wrong
small element in a tail column) and normwise within test_gpu_parity's tolerances (it sees a
precision regression of the whole product).  Every case prints max |err| / bound per product.
"""
import numpy as np
import pytest
import torch

import fc_stage as S
from ba3c_amd import ppo
from ba3c_amd._lib import SCALAR_NAMES
from test_gpu_parity import FWD_TOL, GRAD_TOL, as64, case, check_gradients_and_scalars, dev
from test_gpu_ppo import _check_scalars, _prepared
from test_ppo_rules import BETA, EPS, check_cases

pytestmark = pytest.mark.gpu

EVERY = (33, 129)                # every geometry: fwd 64-row tile + tail / first 128 x 128 backward
MORE = (1, 3, 65, 257)           # g3, g9, g11 too: one wave, a partial heads workgroup, off the
                                 # 64-row forward tiles, the scalars' own launch (B > 256)
CASES = [(n, B) for n in sorted(S.GEOMETRIES, key=lambda n: int(n[1:]))
         for B in sorted(EVERY + (MORE if n in ("g3", "g9", "g11") else ()))]
SWITCHES = [("BA3C_GENERIC", "1"),     # the fp32-MFMA engine (gemm_kernel) for every product
            ("BA3C_MULTI", "0"),       # the three FC products as separate launches, small tiles
            ("BA3C_MULTI_BIG", "2"),   # the large-batch fc1 pair off the multi-job launch
            ("BA3C_OVERLAP", "1")]     # weight gradients on the side stream


def _engine(g, B):
    from ba3c_amd.engine import Ba3cEngine
    return Ba3cEngine(num_actions=g["A"], channels=g["C"], fc_neurons=g["F"], fc_splits=g["S"],
                      replace_with_conv=not g.get("legacy", False), ps=g.get("ps", 1), max_batch=B)


def _report(label, product, ratio, norm=None):
    print("%s %-8s max|err|/bound %.4f%s" % (label, product, ratio,
                                             "" if norm is None else "  normwise %.3e" % norm))


def check_fc_stage(name, B, label=None):
    """The seven comparisons of one training pass and the forward call's (module docstring)."""
    g = S.GEOMETRIES[name]
    F, A = g["F"], g["A"]
    label = label or "%s B=%d" % (name, B)
    params, state, action, R, cfg = case(500 + 7 * int(name[1:]) + B, B, wscale=2.0, **g)
    p64 = as64(params)
    eng = _engine(g, B)
    eng.load_params(params)
    eng.grads.fill_(float("nan"))
    sc = eng.train_grads(dev(state), dev(action), dev(R), entropy_beta=0.01)
    ws = lambda n, w: eng.workspace_tensor(n, B).cpu().numpy().reshape(B, w).copy()
    a3, h, dh, dy3 = ws("a3", 1600), ws("h", F), ws("dh", F), ws("dy3", 1600)
    h_train = eng.workspace_tensor("h", B).clone()
    flat = eng.grads.cpu().numpy()
    got = eng.state_dict(eng.grads)
    s = sc.cpu().numpy()
    assert eng.device_errors() == 0
    fails = []

    def hold(product, ok, detail):
        if not ok:
            fails.append((product, detail))

    # 1. h from the GPU's a3
    fw = S.fc1_forward(p64, cfg, a3)
    r, nw = S.model_ratio(h, fw["h"], fw["mag"], 1600), S.normwise(h, fw["h"])
    _report(label, "h", r, nw)
    hold("h", r < 1 and nw < FWD_TOL, (r, nw))
    # 2. dh from the GPU's h (the legacy ReLU mask is the GPU's own h > 0)
    lb = S.loss_backward(p64, h, action, R, entropy_beta=0.01)
    ref_dh, _ = S.head_dh(p64, cfg, lb["dz"], lb["dV"], h)
    nw = S.normwise(dh, ref_dh)
    print("%s %-8s normwise %.3e" % (label, "dh", nw))
    hold("dh", nw < GRAD_TOL, nw)
    # 3. the seven scalars from the GPU's h
    for i, n in enumerate(SCALAR_NAMES[:7]):
        ref = lb["scalars"][i]
        hold(n, abs(s[i] - ref) <= 1e-4 * max(1.0, abs(ref)), (s[i], ref))
    # 4. dY3 from the GPU's dh and a3: exactly zero where a3 <= 0
    ref_dy3, mag = S.fc1_dgrad(p64, cfg, dh, a3)
    on = a3 > 0
    r = S.model_ratio(dy3[on], ref_dy3[on], mag[on], F)
    _report(label, "dy3", r, S.normwise(dy3, ref_dy3))
    hold("dy3", r < 1, r)
    hold("dy3 off", np.all(dy3[~on] == 0), int(np.count_nonzero(dy3[~on])))
    # 5. fc1's weight (and legacy bias) gradients from the GPU's a3 and dh
    for k, (ref, mag) in sorted(S.fc1_wgrad(cfg, a3, dh).items()):
        r = S.model_ratio(got[k], ref, mag, B)
        _report(label, k, r, S.normwise(got[k], ref))
        hold(k, r < 1, r)
    # 6. the head gradients from the GPU's h (the GPU's product reads its float32 [dz | dV] row)
    for k, (ref, mag) in sorted(S.head_wgrad(h, lb["dz"], lb["dV"]).items()):
        r, nw = S.model_ratio(got[k], ref, mag, B, extra=S.STORED_ROW), S.normwise(got[k], ref)
        _report(label, k, r, nw)
        hold(k, r < 1 and nw < GRAD_TOL, (r, nw))
    # 7. every gradient element was written (the reduction runs without a memset), and nothing
    # else: the flat layout starts each tensor on a multiple of 64 floats, and the floats
    # between a tensor's end and the next one's start, where a store past a tail would land,
    # still hold the fill
    owned = np.zeros(flat.size, bool)
    for _, off, numel, _ in eng.layout:
        owned[off:off + numel] = True
    hold("nan fill", not np.isnan(flat[owned]).any(), int(np.isnan(flat[owned]).sum()))
    hold("padding untouched", np.isnan(flat[~owned]).all(), int((~np.isnan(flat[~owned])).sum()))

    # the predictor forward on the same engine: the heads from the inference workspace's h
    probs, probsT, value = eng.forward(dev(state), explore_factor=1.7)
    h_fwd = eng.workspace_tensor("h", B, train=False)
    hold("h fwd == train", torch.equal(h_fwd, h_train), None)
    hd = S.heads_forward(p64, h_fwd.cpu().numpy().reshape(B, F), explore_factor=1.7)
    e = (S.normwise(probs.cpu().numpy(), hd["logits"]), S.normwise(probsT.cpu().numpy(), hd["logitsT"]),
         float(np.abs(value.cpu().numpy().astype(np.float64) - hd["pred_value"]).max() / hd["value_mag"].max()))
    print("%s forward  probs %.3e probsT %.3e value %.3e" % ((label,) + e))
    hold("forward", max(e) < FWD_TOL, e)
    assert eng.device_errors() == 0
    del eng
    torch.cuda.synchronize()
    assert not fails, (label, fails)


@pytest.mark.parametrize("name,B", CASES)
def test_fc_stage_matches_float64(name, B):
    check_fc_stage(name, B)


@pytest.mark.parametrize("var,val", SWITCHES)
@pytest.mark.parametrize("B", EVERY)
@pytest.mark.parametrize("name", ["g3", "g5", "g11"])
def test_fc_stage_under_each_launch_structure(monkeypatch, name, B, var, val):
    """The same comparisons, not another GPU run: the tile sizes differ between the structures,
    so bit-identity is not promised."""
    for v, _ in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(var, val)
    check_fc_stage(name, B, label="%s B=%d %s=%s" % (name, B, var, val))


@pytest.mark.parametrize("name", ["g1", "g3", "g4", "g7", "g9", "g12"])
def test_ppo_heads_match_the_rules(name):
    """test_gpu_ppo.test_heads_match_the_rules_on_the_seven_cases at the new forms."""
    cfgk, B = S.GEOMETRIES[name], 33
    eng, params, state, action, cfg, h, rows, kinds, a3c = _prepared(40, B, **cfgk)
    sc = eng.train_grads_ppo(dev(state), dev(action), dev(rows), EPS, entropy_beta=BETA)
    got_sc, ratio = sc.cpu().numpy(), eng.ratio[:B].cpu().numpy()
    assert np.array_equal(eng.workspace_tensor("h", B).cpu().numpy().reshape(B, -1), h)
    dh = eng.workspace_tensor("dh", B).cpu().numpy().reshape(B, -1)
    out = ppo.heads_from_h(h, params, action, rows, EPS, BETA)
    check_cases(out, rows, kinds)
    ref_dh = out["dh"] * (h > 0) if cfgk.get("legacy") else out["dh"]
    print("%s dh rel %.3e, ratio rel %.3e" % (name, S.normwise(dh, ref_dh), S.normwise(ratio, out["rho"])))
    assert S.normwise(dh, ref_dh) < GRAD_TOL
    assert S.normwise(ratio, out["rho"]) < FWD_TOL
    _check_scalars(got_sc, out["scalars"], a3c)
    assert eng.device_errors() == 0


@pytest.mark.parametrize("name", ["g3", "g9"])
def test_forward_is_batch_independent_at_a_tail(name):
    """test_large_batch_forward_is_batch_independent where the last N tile is 4 columns wide."""
    g, B = S.GEOMETRIES[name], 257
    params, state, _, _, _ = case(900 + int(name[1:]), B, wscale=2.0, **g)
    eng = _engine(g, B)
    eng.load_params(params)
    state = dev(state)
    whole = [x.clone() for x in eng.forward(state)]
    h_all = eng.workspace_tensor("h", B, train=False).clone().view(B, g["F"])
    for lo, hi in ((0, 1), (5, 70), (128, 257)):
        p, _, v = eng.forward(state[lo:hi].contiguous())
        h = eng.workspace_tensor("h", hi - lo, train=False).view(hi - lo, g["F"])
        assert torch.equal(p, whole[0][lo:hi]) and torch.equal(v, whole[2][lo:hi]), (lo, hi)
        assert torch.equal(h, h_all[lo:hi]), (lo, hi)
    assert eng.device_errors() == 0
    del eng
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["g1", "g4", "g9", "g11", "g13"])
def test_whole_pass_matches_oracle_once_per_new_form(name):
    """test_gpu_parity.test_gradients_and_scalars_match_oracle's body at B = 5: the oracle driven
    by the GPU's decisions, every gradient including the convolutions' (a tail dY3 flows on
    into conv3's kernels), all eight scalars and the padded conv0 channels."""
    check_gradients_and_scalars(S.GEOMETRIES[name], 5)
