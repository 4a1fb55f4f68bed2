"""conv0's input-gradient kernel, the seed heads, ba3c_input_grads and the recorder's --saliency on
the MI355X, held to float64 (ba3c_amd.saliency, torch autograd) with test_gpu_parity's bound."""
import numpy as np
import pytest
import torch

from ba3c_amd import saliency as S
from conv0d_walk import BINADES, deal
from test_gpu_parity import GRAD_TOL, case, dev, engine, gpu_decisions, rel
from test_gpu_ppo import HEADS

pytestmark = pytest.mark.gpu


def run_kernel(eng, dp0, c0):
    B = dp0.shape[0]
    eng.workspace_tensor("dp0", B).copy_(dev(dp0.reshape(-1)))
    eng.workspace_tensor("c0", B).copy_(dev(c0.reshape(-1)))
    dx, m = eng.conv0_input_grad(B, map=True)
    return dx.cpu().numpy(), m.cpu().numpy()


def held_normwise(dp0, c0, w0, dx, m, tag):
    """The per-image normwise bound on dX against the float64 rule (an all-zero image: exact zeros)
    and `map` within 4 spacings of the float64 channel sum of the kernel's own dX."""
    ref = S.conv0_input_grad_numpy(dp0, c0, w0)
    f32 = S.conv0_input_grad_numpy(dp0, c0, w0, np.float32)
    for b in range(len(dp0)):
        if not dp0[b].any():
            assert not dx[b].any() and not m[b].any()           # exact zeros
            continue
        print("%s image %d: kernel %.3e, float32 numpy %.3e" % (tag, b, rel(dx[b], ref[b]), rel(f32[b], ref[b])))
        assert rel(dx[b], ref[b]) < GRAD_TOL
    want = np.abs(dx).sum(axis=3, dtype=np.float64)
    assert np.all(np.abs(m - want) <= 4 * np.spacing(want.astype(np.float32)))


def check(kind, B, pad=0.0):
    params = case(3, 1)[0]
    params["conv0/W"][:, :, 4:] = pad
    eng = engine()
    eng.load_params(params)
    dp0, c0 = deal(kind, B)
    dx, m = run_kernel(eng, dp0, c0)
    held_normwise(dp0, c0, params["conv0/W"], dx, m, "%s B=%d" % (kind, B))
    return dx, m


@pytest.mark.parametrize("kind,B", [(k, B) for k in ("single0", "single1", "single2", "single3", "dense")
                                    for B in (1, 3)] + [("binades", len(BINADES))])
def test_kernel_alone_matches_float64(kind, B):
    check(kind, B)


def test_padded_weight_channels_are_not_read():
    a, b = check("dense", 3), check("dense", 3, pad=1e6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_an_image_does_not_depend_on_its_slot():
    eng = engine()
    eng.load_params(case(3, 1)[0])
    dp0, c0 = deal("dense", 3)
    whole = run_kernel(eng, dp0, c0)
    for j in range(3):
        one = run_kernel(eng, dp0[j:j + 1], c0[j:j + 1])
        assert np.array_equal(one[0][0], whole[0][j]) and np.array_equal(one[1][0], whole[1][j])


@pytest.mark.parametrize("seed", [(1.0, 0.0), (0.0, 1.0), None], ids=["pi", "v", "mix"])
@pytest.mark.parametrize("name", ["A4_F128", "legacy"])
def test_seed_heads_match_the_rule_on_the_gpus_own_h(name, seed):
    cfgk, B = HEADS[name], 33
    params, state, action, _, _ = case(40, B, **cfgk)
    eng = engine(max_batch=64, **cfgk)
    eng.load_params(params)
    seeds = np.random.RandomState(5).normal(size=(B, 2)) if seed is None else np.tile(seed, (B, 1))
    eng.input_grads(dev(state), dev(action), dev(seeds.astype(np.float32)))
    h = eng.workspace_tensor("h", B).cpu().numpy().reshape(B, -1).astype(np.float64)
    dh = eng.workspace_tensor("dh", B).cpu().numpy().reshape(B, -1)
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    z = h @ p64["fc-pi/W"] + p64["fc-pi/b"]
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    dz = seeds[:, :1].astype(np.float32) * (np.eye(cfgk["A"])[action] - p)
    ref = dz @ p64["fc-pi/W"].T + seeds[:, 1:].astype(np.float32) @ p64["fc-v/W"].T
    ref = ref * (h > 0) if cfgk.get("legacy") else ref
    print("%s dh rel %.3e" % (name, rel(dh, ref)))
    assert rel(dh, ref) < GRAD_TOL


def autograd_reference(params, state, action, seeds, forced):
    """d(s_pi log pi(a) + s_v V) / d(state / 255) in float64, the pooling and conv3's ReLU taking
    the GPU's own decisions."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    conv = lambda x, k: torch.nn.functional.conv2d(x, t(params[k]).permute(3, 2, 0, 1))
    x = t(state / 255.0).permute(0, 3, 1, 2).requires_grad_()
    a = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, 12))
    for l in range(3):
        z = conv(a, "conv%d/W" % l)
        B, C, H, W = z.shape
        win = z.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
        code = torch.from_numpy(forced["c%d" % l].astype(np.int64)).permute(0, 3, 1, 2)
        a = torch.gather(win, 4, (code % 255)[..., None])[..., 0] * (code != 255)
    a3 = conv(a, "conv3/W").permute(0, 2, 3, 1) * t(forced["a3_mask"])
    h = a3.reshape(len(state), 1600) @ torch.cat([t(params["fc1_%d/W" % i]).reshape(1600, -1) for i in range(4)], 1)
    logp = torch.log_softmax(h @ t(params["fc-pi/W"]) + t(params["fc-pi/b"]), 1)[np.arange(len(action)), action]
    J = (t(seeds[:, 0]) * logp + t(seeds[:, 1]) * (h @ t(params["fc-v/W"]))[:, 0]).sum()
    return torch.autograd.grad(J, x)[0].permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("seed,B", [((0.0, 1.0), 2), ((1.0, 0.0), 2), (None, 129)], ids=["v", "pi", "mix129"])
def test_input_grads_end_to_end(seed, B):
    """B = 129 is one above OVERLAP_B: ba3c_input_grads then runs the seed heads under the
    large-batch launch plan (mj_fc on big tiles, whole-map conv2, no multi-job conv launches) and
    conv0d_kernel walks (2709 bands); mixed per-sample seeds.  All 129 images are compared, the
    float64 autograd evaluated in chunks of at most 32 (the objective is a per-sample sum)."""
    params, state, action, _, _ = case(60, B, wscale=2.0)
    eng = engine(max_batch=max(B, 64))
    eng.load_params(params)
    if seed is None:
        seeds = np.random.RandomState(6).normal(size=(B, 2)).astype(np.float32)
    else:
        seeds = np.tile(np.float32(seed), (B, 1))
    before = eng.grads.clone()
    for n in ("c0", "c1", "c2"):                               # no code, no finite a3: the decisions
        eng.workspace_tensor(n, B).fill_(7)                    # read back below are this call's
    eng.workspace_tensor("a3", B).fill_(float("nan"))
    dx, m = eng.input_grads(dev(state), dev(action), dev(seeds), map=True)
    assert torch.equal(eng.grads, before)                      # the weight gradients go to scratch
    forced, codes = gpu_decisions(eng, B)
    assert all(np.isin(c, (0, 1, 2, 3, 255)).all() for c in codes)
    assert np.isfinite(eng.workspace_tensor("a3", B).cpu().numpy()).all()
    dx = dx.cpu().numpy()
    for i in range(0, B, 32):
        ref = autograd_reference(params, state[i:i + 32], action[i:i + 32], seeds[i:i + 32],
                                 {k: v[i:i + 32] for k, v in forced.items()})
        for b in range(len(ref)):
            print("seed %s image %d: rel %.3e" % (seed, i + b, rel(dx[i + b], ref[b])))
            assert rel(dx[i + b], ref[b]) < GRAD_TOL
    if seed is not None:
        assert torch.equal(S.value_map(eng, dev(state)) if seed[1] else S.policy_map(eng, dev(state), dev(action)), m)


def test_recorder_stores_the_value_map_of_each_decision(tmp_path):
    from ba3c_amd import boxing as K
    from ba3c_amd.engine import Ba3cEngine
    from ba3c_amd.flags import GRID_BOXING
    from ba3c_amd.record import ARRAYS, Episode, record_episodes
    eng = Ba3cEngine(num_actions=18, channels=4, fc_neurons=128, fc_splits=4, max_batch=4)
    eng.init_params(seed=1)
    kw = dict(n_envs=1, seed=2, limit=3, scale=1)
    torch.manual_seed(0)
    plain, = record_episodes(eng, GRID_BOXING, 1, **kw)
    torch.manual_seed(0)
    ep, = record_episodes(eng, GRID_BOXING, 1, saliency="v", **kw)
    assert plain.saliency is None and ep.steps == 3 and ep.saliency.shape == (3, 84, 84)
    for k in ARRAYS:
        assert np.array_equal(getattr(plain, k), getattr(ep, k)), k
    frames = K.render_numpy(ep.replay()[0][:3])                # the frame each decision saw
    for t in range(3):
        state = np.zeros((1, 84, 84, 4), np.uint8)
        state[0, :, :, 3 - t:] = frames[:t + 1].transpose(1, 2, 0)
        assert np.array_equal(S.value_map(eng, dev(state), newest=True).cpu().numpy()[0], ep.saliency[t])
    assert ep.saliency.any() and ep.tinted_frames().shape == ep.frames.shape
    back = Episode.load(ep.save(str(tmp_path / "e"))[0])
    assert np.array_equal(back.saliency, ep.saliency) and "saliency" not in np.load(plain.save(str(tmp_path / "p"))[0]).files
