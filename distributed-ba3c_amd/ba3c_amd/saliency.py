"""Input-gradient saliency: which pixels the value and the chosen action's log-probability
depend on.

`Ba3cEngine.input_grads` differentiates, per sample, J = s_pi log pi(a | x) + s_v V(x) with
respect to the float frames the network sees (x = state / 255): the training-mode forward, the
seed form of the heads (dlogits = s_pi (onehot(a) - p), dV = s_v), the ordinary backward pass
down to dP0, and conv0's input gradient (csrc/ba3c_conv0d.h), the one layer whose input gradient
training never needs.  This module states that last rule in float64 numpy and is the kernel's
oracle; `value_map` / `policy_map` are the two maps a viewer asks for.

The rule.  dP0 [B,40,40,32] is the gradient of the pooled conv0 output, c0 its argmax codes
(0..3: the first maximum of the 2x2 window, row-major; 255: the window's maximum was <= 0).
    dY[b, y, x, o] = dP0[b, y>>1, x>>1, o]  where c0[b, y>>1, x>>1, o] == 2 (y&1) + (x&1), else 0
    dX[b, y, x, c] = sum_{ky, kx in 0..4, o} dY[b, y-ky, x-kx, o] W0[ky, kx, c, o]
for 0 <= y, x < 84 and the C = 4 real input channels (dY is 0 outside [0, 80)^2).

`perturb_value_map` / `perturb_policy_map` are the perturbation maps of ba3c_amd.perturb, which
need no gradient: the smoother picture the Atari literature shows.  `ig_value_map` /
`ig_policy_map` are the integrated-gradients maps of ba3c_amd.intgrad: this module's gradient
averaged over a path from a baseline and scaled by the distance from it, in the same units.
"""
import numpy as np

H = W = 84          # frame
HO = WO = 80        # conv0's output
KT = 5              # its taps per axis
C = 4               # real input channels


def unpool_numpy(dp0, c0):
    """dP0 [B,40,40,O], codes [B,40,40,O] -> dY [B,80,80,O] (float64)."""
    dp0 = np.asarray(dp0, np.float64)
    B, ph, pw, O = dp0.shape
    dy = np.zeros((B, 2 * ph, 2 * pw, O), np.float64)
    for k in range(4):
        dy[:, k >> 1::2, k & 1::2, :] = np.where(np.asarray(c0) == k, dp0, 0.0)
    return dy


def conv0_input_grad_numpy(dp0, c0, w0, dtype=np.float64):
    """The rule above: -> dX [B, 2*ph+4, 2*pw+4, C] in `dtype` (float32: the yardstick of what
    plain single precision gives).  w0: conv0/W [5,5,>=C,O]; only channels < C are read."""
    dy = unpool_numpy(dp0, c0).astype(dtype)
    w = np.asarray(w0)[:, :, :C, :].astype(dtype)
    B, ho, wo, O = dy.shape
    dx = np.zeros((B, ho + KT - 1, wo + KT - 1, C), dtype)
    for ky in range(KT):
        for kx in range(KT):
            dx[:, ky:ky + ho, kx:kx + wo, :] += dy @ w[ky, kx].T      # [.., O] @ [O, C]
    return dx


def toeplitz_numpy(w0):
    """The kernel's weight matrix T [(ky, j, o), (dx, c)] = W0[ky, dx + 4 - j, c, o] where
    0 <= dx + 4 - j <= 4, else 0: a GEMM row is a group of four adjacent output pixels
    x = 4g + dx and reads the 8 dY columns 4g - 4 + j.  -> float64 [5, 8, O, 4, C]."""
    w = np.asarray(w0, np.float64)[:, :, :C, :]
    O = w.shape[3]
    t = np.zeros((KT, 8, O, 4, C), np.float64)
    for j in range(8):
        for dx in range(4):
            kx = dx + 4 - j
            if 0 <= kx < KT:
                t[:, j, :, dx, :] = w[:, kx].transpose(0, 2, 1)
    return t


def conv0_input_grad_toeplitz(dp0, c0, w0):
    """The same dX as the GEMM through T (float64): rows (y, g), K = (ky, j, o), N = (dx, c)."""
    dy = unpool_numpy(dp0, c0)
    B, ho, wo, O = dy.shape
    hh, ww = ho + KT - 1, wo + KT - 1
    assert ww % 4 == 0
    pad = np.zeros((B, ho + 2 * (KT - 1), ww + 4, O), np.float64)     # rows -4.., columns -4..
    pad[:, KT - 1:KT - 1 + ho, 4:4 + wo] = dy
    t = toeplitz_numpy(w0).reshape(KT * 8 * O, 4 * C)
    dx = np.zeros((B, hh, ww, C), np.float64)
    for g in range(ww // 4):
        # A[b, y, (ky, j, o)] = dY[b, y - ky, 4g - 4 + j, o]
        a = np.stack([pad[:, KT - 1 - ky:KT - 1 - ky + hh, 4 * g:4 * g + 8, :] for ky in range(KT)], axis=2)
        dx[:, :, 4 * g:4 * g + 4, :] = (a.reshape(B, hh, -1) @ t).reshape(B, hh, 4, C)
    return dx


def saliency_map(dx):
    """sum_c |dX| [B,84,84] (the kernel's optional second output)."""
    return np.abs(dx).sum(axis=-1)


def _seeded(engine, state, action, s_pi, s_v, newest):
    import torch
    B = state.shape[0]
    if action is None:
        action = torch.zeros(B, dtype=torch.int64, device=state.device)
    seeds = torch.tensor([s_pi, s_v], dtype=torch.float32, device=state.device).repeat(B, 1)
    dx, m = engine.input_grads(state, action, seeds, map=True)
    return dx[..., -1].abs() if newest else m


def value_map(engine, state, newest=False):
    """|dV / dx| of each state [B,84,84,4] (uint8, device): seeds (0, 1).  -> float32 [B,84,84],
    summed over the four frames, or the newest frame's channel alone."""
    return _seeded(engine, state, None, 0.0, 1.0, newest)


def policy_map(engine, state, action, newest=False):
    """|d log pi(action) / dx|: seeds (1, 0)."""
    return _seeded(engine, state, action, 1.0, 0.0, newest)


def perturb_value_map(engine, state, newest=False):
    """The perturbation saliency of the value (ba3c_amd.perturb: S_v = 1/2 (V - V')^2 under a
    blurred patch at each of 17 x 17 centres, interpolated to the frame): Ba3cEngine.perturb_maps.
    -> float32 [B,84,84]; newest: only the newest frame is blurred."""
    return engine.perturb_maps(state, "v", newest=newest)


def perturb_policy_map(engine, state, newest=False):
    """The same of the policy: S_pi = 1/2 sum_a (p_a - p'_a)^2."""
    return engine.perturb_maps(state, "pi", newest=newest)


def _integrated(engine, state, action, s_pi, s_v, newest, steps, baseline):
    import torch
    B = state.shape[0]
    if action is None:
        action = torch.zeros(B, dtype=torch.int64, device=state.device)
    seeds = torch.tensor([s_pi, s_v], dtype=torch.float32, device=state.device).repeat(B, 1)
    attr = engine.integrated_grads(state, action, seeds, steps=steps, baseline=baseline).abs()
    return attr[..., -1] if newest else attr.sum(dim=-1)


def ig_value_map(engine, state, newest=False, steps=32, baseline="blur"):
    """|integrated gradients of V| (ba3c_amd.intgrad, Ba3cEngine.integrated_grads with seeds
    (0, 1)) of each state.  -> float32 [B,84,84], summed over the four frames, or the newest
    frame's channel alone, as value_map."""
    return _integrated(engine, state, None, 0.0, 1.0, newest, steps, baseline)


def ig_policy_map(engine, state, action, newest=False, steps=32, baseline="blur"):
    """The same of log pi(action): seeds (1, 0)."""
    return _integrated(engine, state, action, 1.0, 0.0, newest, steps, baseline)
