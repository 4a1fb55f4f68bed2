"""The bench workload itself (B=2048, F=512, S=1 — configs[2]/[3]) against a float64 reference,
every gradient tensor held to 1e-4 per tensor, conv0..conv2's weight gradients included (VERDICT
r04 item 1: they are the outputs of the dominant launch, the conv1 ‖ conv0 weight-gradient pair).

The checker is `oracle/ba3c_torch_f64.py` (torch float64 convolutions + autograd of the
reference graph, train.py:164-327, run on the CPU; pinned to the numpy oracle in
tests/test_oracle.py), driven by the GPU's own discrete decisions — the max-pool argmax codes
c0..c2 and conv3's ReLU mask read back from the workspace — so the comparison is of arithmetic
alone.  Those decisions are separately held to the float64 forward's own: they may differ only
on numerically ambiguous windows (fp32 near-ties; exact ties must match).  Random frames and Atari-like frames (exact ties
everywhere, tests/atari_frames.py)."""
import numpy as np
import pytest
import torch

from atari_frames import atari_frames
from oracle import ba3c_oracle as O
from oracle.ba3c_torch_f64 import loss_and_grads_forced, own_decisions
from test_gpu_parity import GRAD_TOL, gpu_decisions, rel

pytestmark = pytest.mark.gpu

B = 2048
CFG = {"fc_neurons": 512, "fc_splits": 1}


def _case(frames):
    rs = np.random.RandomState(2048)
    params = O.init_params(512, 1, 4, seed=21, dtype=np.float32)
    if frames == "atari":
        params = {k: (v * np.float32(2.0)).astype(np.float32) for k, v in params.items()}
        state = atari_frames(B, 77)
    else:
        state = rs.randint(0, 256, size=(B, 84, 84, 4)).astype(np.uint8)
    action = rs.randint(0, 4, size=B).astype(np.int64)
    R = rs.normal(size=B).astype(np.float32)
    return params, state, action, R


@pytest.mark.parametrize("frames", ["random", "atari"])
def test_bench_workload_every_gradient_matches_fp64(frames):
    from ba3c_amd.engine import Ba3cEngine
    params, state, action, R = _case(frames)
    eng = Ba3cEngine(num_actions=4, fc_neurons=512, fc_splits=1, max_batch=B)
    eng.load_params(params)
    sc = eng.train_grads(torch.from_numpy(state).cuda(), torch.from_numpy(action).cuda(),
                         torch.from_numpy(R).cuda(), entropy_beta=0.01)
    got = {k: v.astype(np.float64) for k, v in eng.state_dict(eng.grads).items()}
    forced, codes = gpu_decisions(eng, B)
    cost = float(sc.cpu().numpy()[0])
    del eng
    torch.cuda.synchronize()

    # the GPU's decisions equal the fp64 forward's own in every window that is not numerically
    # ambiguous (a near-tie or a max within rounding of zero, which any fp32 evaluation may
    # resolve either way; exact ties are NOT ambiguous: the first-max rule decides them), and
    # ambiguous windows stay rare (as tests/test_gpu_hard_inputs.py at B <= 512)
    own = own_decisions(params, state)
    for layer in range(3):
        near = own["near_c%d" % layer]
        assert np.mean(near) < 1e-2, (layer, np.mean(near))
        bad = (own["c%d" % layer] != codes[layer]) & ~near
        assert not bad.any(), (layer, int(bad.sum()), np.argwhere(bad)[:4])
    bad = (own["a3_mask"] != forced["a3_mask"]) & ~own["near_a3"]
    assert not bad.any(), int(bad.sum())

    ref, out = loss_and_grads_forced(params, state, action, R, CFG, forced, chunk=256)
    errs = {k: rel(got[k], ref[k]) for k in ref}
    print("per-tensor rel err vs fp64 (%s frames): %s" % (
        frames, ", ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
    bad = {k: e for k, e in errs.items() if e >= GRAD_TOL}
    assert not bad, bad
    assert np.all(got["conv0/W"][:, :, 4:, :] == 0)
    assert abs(cost - out["cost"]) <= 1e-4 * max(1.0, abs(out["cost"])), (cost, out["cost"])


# Decision flips against the float64 forward, split path vs the fp32-MFMA engine (VERDICT r05
# item 2).  A discrete decision (a window's argmax, conv3's ReLU sign) flips when an
# evaluation's error exceeds the gap between the competing values; near a tie the gap is
# roughly uniformly distributed, so the flip count scales with the size of the evaluation
# error.  DESIGN.md §3.1's error model: both engines accumulate in fp32; the split products add
# at most 3 x 2^-22 relative per product, about sqrt(K) x 2^-20.4 x rms(term) per output, the
# same order as fp32 accumulation over K = 100..800 terms (between K^0.5 and K x 2^-24 x rms),
# so the split path's error scale is within 2x of the fp32 engine's.  Bound, fixed before the
# first run: flips_split <= 2 x flips_fp32 + 3 sqrt(flips_fp32) (Poisson noise of the count)
# + 3, per layer.
FLIP_LAYERS = ("c0", "c1", "c2", "a3_mask")


def flip_bound(n_fp32):
    return 2.0 * n_fp32 + 3.0 * np.sqrt(n_fp32) + 3.0


@pytest.mark.parametrize("frames", ["random", "atari"])
def test_decision_flips_split_path_vs_fp32_engine(monkeypatch, frames):
    from ba3c_amd.engine import Ba3cEngine
    params, state, action, R = _case(frames)
    own = own_decisions(params, state)
    counts = {}
    for name, generic in (("split", "0"), ("fp32", "1")):
        monkeypatch.setenv("BA3C_GENERIC", generic)
        eng = Ba3cEngine(num_actions=4, fc_neurons=512, fc_splits=1, max_batch=B)
        eng.load_params(params)
        eng.train_grads(torch.from_numpy(state).cuda(), torch.from_numpy(action).cuda(),
                        torch.from_numpy(R).cuda(), entropy_beta=0.01)
        forced, _ = gpu_decisions(eng, B)
        torch.cuda.synchronize()
        del eng
        counts[name] = {}
        for k in FLIP_LAYERS:
            flip = own[k] != forced[k]
            near = own["near_a3" if k == "a3_mask" else "near_" + k]
            counts[name][k] = (int(flip.sum()), int((flip & ~near).sum()), flip.size)
    print("decision flips vs fp64 (%s frames, B=%d): %s" % (frames, B, "; ".join(
        "%s split %d (%d outside ambiguous) / fp32 %d (%d) of %d" % (
            k, counts["split"][k][0], counts["split"][k][1], counts["fp32"][k][0],
            counts["fp32"][k][1], counts["split"][k][2]) for k in FLIP_LAYERS)))
    for k in FLIP_LAYERS:
        ns, nf = counts["split"][k][0], counts["fp32"][k][0]
        assert ns <= flip_bound(nf), (k, ns, nf, flip_bound(nf))
