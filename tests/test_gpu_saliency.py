"""conv0's input-gradient kernel, the seed heads, ba3c_input_grads and the recorder's --saliency on
the MI355X, held to float64 (ba3c_amd.saliency, torch autograd) with test_gpu_parity's bound."""
import numpy as np
import pytest
import torch

from ba3c_amd import saliency as S
from test_gpu_parity import GRAD_TOL, case, dev, engine, gpu_decisions, rel
from test_gpu_ppo import HEADS

pytestmark = pytest.mark.gpu

SPOTS = [(y, x) for y in (0, 19, 39) for x in (0, 19, 39)]    # corners, edges, centre (pooled)
BINADES = (1e-6, 1.0, 1e4, 0.0)


def deal(kind, B, seed=0):
    """(dP0 float32 [B,40,40,32], codes): single-K: one element per spot (disjoint footprints) under
    code K; dense: N(0,1), ~30 % dead windows; binades: dense, image i scaled by BINADES[i]."""
    rs = np.random.RandomState(seed + B)
    c0 = rs.randint(0, 4, size=(B, 40, 40, 32)).astype(np.uint8)
    if kind.startswith("single"):
        dp0 = np.zeros((B, 40, 40, 32), np.float32)
        c0[:] = int(kind[-1])
        for b in range(B):
            for y, x in SPOTS:
                dp0[b, y, x, rs.randint(32)] = rs.normal()
        return dp0, c0
    c0[rs.random_sample(c0.shape) < 0.3] = 255
    dp0 = rs.normal(size=c0.shape)
    if kind == "binades":
        dp0 *= np.asarray(BINADES)[:B, None, None, None]
    return dp0.astype(np.float32), c0


def run_kernel(eng, dp0, c0):
    B = dp0.shape[0]
    eng.workspace_tensor("dp0", B).copy_(dev(dp0.reshape(-1)))
    eng.workspace_tensor("c0", B).copy_(dev(c0.reshape(-1)))
    dx, m = eng.conv0_input_grad(B, map=True)
    return dx.cpu().numpy(), m.cpu().numpy()


def check(kind, B, pad=0.0):
    params = case(3, 1)[0]
    params["conv0/W"][:, :, 4:] = pad
    eng = engine()
    eng.load_params(params)
    dp0, c0 = deal(kind, B)
    dx, m = run_kernel(eng, dp0, c0)
    ref = S.conv0_input_grad_numpy(dp0, c0, params["conv0/W"])
    f32 = S.conv0_input_grad_numpy(dp0, c0, params["conv0/W"], np.float32)
    for b in range(B):
        if not dp0[b].any():
            assert not dx[b].any() and not m[b].any()           # exact zeros
            continue
        print("%s B=%d image %d: kernel %.3e, float32 numpy %.3e" % (kind, B, b, rel(dx[b], ref[b]), rel(f32[b], ref[b])))
        assert rel(dx[b], ref[b]) < GRAD_TOL
    want = np.abs(dx).sum(axis=3, dtype=np.float64)
    assert np.all(np.abs(m - want) <= 4 * np.spacing(want.astype(np.float32)))
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


@pytest.mark.parametrize("seed", [(0.0, 1.0), (1.0, 0.0)], ids=["v", "pi"])
def test_input_grads_end_to_end(seed):
    B = 2
    params, state, action, _, _ = case(60, B, wscale=2.0)
    eng = engine()
    eng.load_params(params)
    seeds = np.tile(np.float32(seed), (B, 1))
    before = eng.grads.clone()
    dx, m = eng.input_grads(dev(state), dev(action), dev(seeds), map=True)
    assert torch.equal(eng.grads, before)                      # the weight gradients go to scratch
    ref = autograd_reference(params, state, action, seeds, gpu_decisions(eng, B)[0])
    for b in range(B):
        print("seed %s image %d: rel %.3e" % (seed, b, rel(dx[b].cpu().numpy(), ref[b])))
        assert rel(dx[b].cpu().numpy(), ref[b]) < GRAD_TOL
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
