"""The scaled-fp16 conv path on batches whose exponents differ (tests/mixed_frames.py).

Every conv operand is multiplied by a power of two before it is split into fp16 planes: maps
per image (amax_publish into slot [1 + img], amax_exp(amax_in[1 + img])), weights per tensor
(the eight wexp slots), the weight-gradient kernels by the maximum over the batch's slots; the
step's weight-prep launch zeroes the slots.  With random or Atari-like frames and the
initialisers' weights all of those exponents coincide, so reading a neighbour's, a stale or
another tensor's slot gives the same bits, and a batch-normwise tolerance hides a dim image
computed with too few bits next to a bright one.  Here neighbouring images differ by up to
2^8 in the input (and one is black: amax == 0), per-image gradients by ~2^17, and conv0..3 sit
in four distinct binades:

* per-image parity against the fp64 oracle at B=32, every engine configuration;
* an image's maps do not depend, bit for bit, on its slot, workgroup or ring position
  (B=32 / 160 / 1024 under a permutation that changes every slot's kind);
* the ring walk (2 images per workgroup at B=1024) against the one-band kernels, bit for bit;
* nothing survives on a handle from a large bright batch into a small dim one;
* distinct weight binades at B=160 (whole-map conv2 kernels, multi-band conv0 weight gradient).

The tolerances are test_gpu_parity's FWD_TOL and GRAD_TOL, here applied per image.
"""
import numpy as np
import pytest
import torch

from oracle import ba3c_oracle as O
from mixed_frames import (KINDS, device_mixed_returns, mixed_frames, mixed_returns,
                          return_classes, scaled_params)
from test_gpu_hard_inputs import _check_against_oracle, _engine
from test_gpu_parity import (CONFIGS, FWD_TOL, GRAD_TOL, as64, dev, engine, gpu_decisions, rel,
                             value_err)

pytestmark = pytest.mark.gpu

FWD_MAPS = ("p0", "p1", "p2", "a3", "h")
BWD_MAPS = ("dh", "dp2", "dp1", "dp0")
CODES = ("c0", "c1", "c2")


def per_image(got, ref):
    """(max|got_i - ref_i|, max|ref_i|) for every image i."""
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    return np.abs(got - ref).max(axis=1), np.abs(ref).max(axis=1)


def worst_ratio(err, den):
    """max_i err_i / den_i over the images with a non-zero reference (reported, not asserted)."""
    nz = den > 0
    return float((err[nz] / den[nz]).max()) if nz.any() else 0.0


@pytest.mark.parametrize("cfgk", CONFIGS)
def test_every_image_matches_oracle_at_b32(cfgk):
    """B=32 (small-band kernels, multi-job launches): the gradients and scalars as in
    test_gradients_and_scalars_match_oracle, and every workspace map within the tolerance of
    EACH IMAGE's own max |ref| — bright, dim and black images side by side."""
    B = 32
    A, C, F, S = cfgk["A"], cfgk["C"], cfgk["F"], cfgk["S"]
    legacy, ps = cfgk.get("legacy", False), cfgk.get("ps", 1)
    cfg = {"fc_neurons": F, "fc_splits": S, "replace_with_conv": not legacy, "ps": ps}
    params = scaled_params(5, F, S, A, replace_with_conv=not legacy, ps=ps)
    state, kinds = mixed_frames(B, 7, C=C)
    action = np.random.RandomState(7).randint(0, A, size=B).astype(np.int64)
    p64 = as64(params)
    R = mixed_returns(O.get_nn_prediction(p64, state, cfg)["pred_value"], 7)
    eng = engine(**cfgk)
    eng.load_params(params)
    sc = eng.train_grads(dev(state), dev(action), dev(R), entropy_beta=0.01)
    got = eng.state_dict(eng.grads)
    ws = {n: eng.workspace_tensor(n, B).cpu().numpy().reshape(B, -1)
          for n in FWD_MAPS + BWD_MAPS + CODES}
    forced, codes = gpu_decisions(eng, B)
    t, osc, g = O.loss_and_grads(p64, state, action, R.astype(np.float64), cfg, forced=forced)
    for layer in range(3):
        own = np.where(t["p%d" % layer] > 0, t["c%d" % layer], 255)
        assert np.mean(own != codes[layer]) < 1e-4, layer
    assert np.mean((t["a3"] > 0) != forced["a3_mask"]) < 1e-4
    for k in g:
        e = rel(got[k], g[k])
        assert e < GRAD_TOL, (k, e)
    assert np.all(got["conv0/W"][:, :, C:, :] == 0)
    s = sc.cpu().numpy()
    from ba3c_amd._lib import SCALAR_NAMES
    print("scalar error / bound:", {n: "%.2e" % (abs(s[i] - float(osc[n])) / (1e-4 * max(1.0, abs(float(osc[n])))))
                                    for i, n in enumerate(SCALAR_NAMES)})
    for i, name in enumerate(SCALAR_NAMES):
        ref = float(osc[name])
        assert abs(s[i] - ref) <= 1e-4 * max(1.0, abs(ref)), (name, s[i], ref)
    assert abs(int(s[7]) - osc["active_relus"]) <= max(2, 1e-5 * osc["active_relus"])

    # per image.  An image whose return is float32(V) has an advantage of a few ulps of V: its
    # head gradient is linear in the forward's own rounding of V, and no fp32 forward meets
    # GRAD_TOL there against an fp64 one (the oracle's own fp32 evaluation of such a batch: dh
    # and dp0..2 off by up to 5e-4 of the image's max on those images, <= 4.5e-6 on all
    # others; the GPU, measured here: dh off by 3.5e-4 .. 3.5e-3).  For those images the reference's heads, loss and backward are evaluated on
    # the GPU's own FC output (forced_h, as for the saturated policies of
    # test_gpu_hard_inputs), which is itself held to FWD_TOL per image just below; every other
    # image is compared with the oracle's own forward and backward.
    R64 = R.astype(np.float64)
    th, _ = O.build_graph_cost(p64, state, action, R64, cfg, forced_h=ws["h"].astype(np.float64))
    th.update(R=R64, forced=forced)
    O.backward(p64, th, cfg)
    floor = (return_classes(B) == 0)[:, None]
    ref = {n: t[n] for n in FWD_MAPS}
    for n in BWD_MAPS:
        ref[n] = np.where(floor, th[n].reshape(B, -1), t[n].reshape(B, -1))
    if legacy:
        # the legacy FC's ReLU sign is the one decision the oracle is not handed: dh is compared
        # where both sides made the same one (a pre-activation within rounding of 0 may flip)
        agree = (ws["h"] > 0) == (t["h_pre"] > 0)
        assert np.mean(~agree) < 1e-4
        ws["dh"], ref["dh"] = ws["dh"] * agree, ref["dh"] * agree
    probs, _, value = eng.forward(dev(state))
    probs, value = probs.cpu().numpy(), value.cpu().numpy()
    worst, fails = {}, []
    for n in FWD_MAPS + BWD_MAPS + ("probs",):
        tol = GRAD_TOL if n in BWD_MAPS else FWD_TOL
        err, den = per_image(probs, t["logits"]) if n == "probs" else per_image(ws[n], ref[n])
        worst[n] = worst_ratio(err, den)
        fails += [(n, int(i), KINDS[kinds[i]], err[i], den[i]) for i in np.flatnonzero(err > tol * den)]
    verr = [value_err(value[i:i + 1], {"h": t["h"][i:i + 1], "pred_value": t["pred_value"][i:i + 1]}, params)
            for i in range(B)]
    worst["value"] = max(verr)
    print("largest per-image error / max|ref_i|:", {k: "%.2e" % v for k, v in worst.items()})
    if not legacy:
        print("  zero-advantage images against the oracle's own forward (reported): dh %.2e"
              % worst_ratio(*per_image(ws["dh"][floor[:, 0]], t["dh"][floor[:, 0]])))
    assert not fails, fails[:8]
    assert max(verr) < FWD_TOL, (int(np.argmax(verr)), max(verr))

    # a black image: amax == 0 in every layer, forward and backward.  The convs have no bias, so
    # every map is exactly zero, no window has a positive max, and the policy is softmax(bias).
    # (dh is not a map of the image: it is the heads' gradient, non-zero for any sample.)
    black = kinds == 2
    for n in FWD_MAPS + BWD_MAPS[1:]:
        assert not np.any(ws[n][black]), n
    for n in CODES:
        assert np.all(ws[n][black] == 255), n
    want = O.softmax(p64["fc-pi/b"][None, :])[0]
    assert np.abs(probs[black] - want).max() <= FWD_TOL * want.max()


def _train_and_keep(eng, state, action, R, names):
    B = state.shape[0]
    sc = eng.train_grads(state, action, R)
    ws = {n: eng.workspace_tensor(n, B).clone() for n in names}
    torch.cuda.synchronize()
    return eng.grads.clone(), sc.clone(), ws


@pytest.mark.parametrize("B", [32, 160, 1024])
def test_maps_of_an_image_do_not_depend_on_its_slot(B):
    """The same batch in two orders.  The same B means the same kernels and the same 1/B; only
    the slot, the workgroup and the ring position of an image change — and the kind of its
    neighbours: perm[n] = B - 1 - 3 n (mod B), a reversal with stride 3, puts an image of
    another kind into every slot (kind 7 - 3 k against k: never equal mod 8) and separates the
    images that shared a ring-walk workgroup.  (A reversal rolled by an odd count maps some
    slots onto their own kind — rolled by 3, slot 1 onto itself.)  Every map of run 2 equals
    run 1's at the permuted index bit for bit.  Weight gradients are sums in another order
    and are not compared."""
    state, kinds = mixed_frames(B, 17)
    perm = (B - 1 - 3 * np.arange(B)) % B
    assert np.array_equal(np.sort(perm), np.arange(B)) and np.all(kinds[perm] != kinds)
    assert np.all(perm[0::2] // 2 != perm[1::2] // 2)           # no pair stays together
    action = np.random.RandomState(17).randint(0, 4, size=B).astype(np.int64)
    eng = _engine(B)
    eng.load_params(scaled_params(9))
    R = device_mixed_returns(eng, dev(state), 17)
    names = FWD_MAPS + CODES + BWD_MAPS
    _, _, one = _train_and_keep(eng, dev(state), dev(action), dev(R), names)
    _, _, two = _train_and_keep(eng, dev(state[perm]), dev(action[perm]), dev(R[perm]), names)
    idx = dev(perm)
    for n in names:
        assert torch.equal(two[n].view(B, -1), one[n].view(B, -1)[idx]), n


def test_ring_walk_on_mixed_images_matches_one_band_kernels(monkeypatch):
    """test_ring_walk_at_bench_batch_matches_one_band_kernels at B=1024 (2 images per ring-walk
    workgroup) on mixed images: the walk prefetches the next image's raw rows while it still
    holds the current image's scale, and here the two always differ."""
    B = 1024
    state, _ = mixed_frames(B, 79)
    action = dev(np.random.RandomState(79).randint(0, 4, size=B).astype(np.int64))
    state = dev(state)
    params = scaled_params(8)
    out, R = [], None
    for env in ("0", None):
        if env is None:
            monkeypatch.delenv("BA3C_RING", raising=False)
        else:
            monkeypatch.setenv("BA3C_RING", env)
        eng = _engine(B)
        eng.load_params(params)
        if R is None:
            R = dev(device_mixed_returns(eng, state, 79))
        out.append(_train_and_keep(eng, state, action, R, ("p1", "c1", "dp0", "p0", "c0")))
        del eng
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    for n in out[0][2]:
        assert torch.equal(out[0][2][n], out[1][2][n]), n


def test_no_scale_survives_from_a_bright_batch_into_a_dim_one():
    """One handle (max_batch=64): a B=64 step on bright images with advantages of 1e3 fills
    every max-|x| slot with large values; a B=8 step on dim, black and single-pixel images with
    advantage ~ 0 and a B=5 forward follow.  Both equal, bit for bit, those of a handle that
    never saw the bright batch (stale slots above `batch`, slots not zeroed between steps)."""
    params = scaled_params(13)
    helper = engine(A=4, C=4, F=512, S=1)                # only to place R around the values
    helper.load_params(params)
    frames, kinds = mixed_frames(256, 23)
    bright = dev(frames[(kinds == 0) | (kinds == 6)])
    dim = dev(frames[:16][np.isin(kinds[:16], (1, 2, 3, 7))])
    assert bright.shape[0] == 64 and dim.shape[0] == 8
    rs = np.random.RandomState(23)
    a_bright, a_dim = (dev(rs.randint(0, 4, size=n).astype(np.int64)) for n in (64, 8))
    v = helper.forward(bright)[2].cpu().numpy()
    R_bright = dev((v + 1e3 * rs.choice([-1.0, 1.0], size=64)).astype(np.float32))
    R_dim = helper.forward(dim)[2].clone()               # R = float32(V)
    names = FWD_MAPS + CODES + BWD_MAPS + ("dy3",)
    runs = []
    for with_bright in (True, False):
        eng = _engine(64)
        eng.load_params(params)
        if with_bright:
            eng.train_grads(bright, a_bright, R_bright)
        step2 = _train_and_keep(eng, dim, a_dim, R_dim, names)
        step3 = [x.clone() for x in eng.forward(dim[:5])]
        torch.cuda.synchronize()
        runs.append((step2, step3))
        del eng
    (g1, s1, w1), f1 = runs[0]
    (g2, s2, w2), f2 = runs[1]
    assert torch.equal(g1, g2) and torch.equal(s1, s2)
    for n in names:
        assert torch.equal(w1[n], w2[n]), n
    for a, b in zip(f1, f2):
        assert torch.equal(a, b)


def test_distinct_weight_binades_at_b160_match_oracle():
    """B=160 (whole-map conv2 kernels, multi-band conv0 weight gradient) with conv0..3 in four
    binades on mixed images: a weight exponent taken from another tensor's slot moves a layer
    by at least 2x.  The returns are the parity tests' N(0, 1): _check_against_oracle bounds
    every scalar by 1e-4 of its own value, and with returns of +-1e3 policy_loss is a sum of
    terms of ~1e3 that cancel to ~17: an fp32 forward's rounding of log p (~1e-7) times 1e3
    per image is then of the order of that bound (measured here: 6.1e-3 against 1.7e-3)."""
    B = 160
    params = scaled_params(5)
    state, _ = mixed_frames(B, 31)
    rs = np.random.RandomState(31)
    action = rs.randint(0, 4, size=B).astype(np.int64)
    R = rs.normal(size=B).astype(np.float32)
    _check_against_oracle(_engine(B), params, state, action, R, strict_codes=True, chunk=16)
