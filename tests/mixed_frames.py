"""Batches whose images, returns and weight tensors differ by whole binades (test infrastructure).

The scaled-fp16 split (csrc/ba3c_split.h) multiplies every operand by a power of two taken
from a max |x|: activation and gradient maps per image, weights per tensor, the weight-gradient
kernels from the maximum over the batch.  Random or Atari-like frames give every image of a
batch the same max |x| to within a binade, and the initialisers give conv1..3 the same scale,
so an exponent read from a neighbouring image, a stale slot or another tensor yields the same
bits.  These helpers make the exponents differ:

* mixed_frames: image n has kind n % 8 (KINDS below), so neighbours in a batch, and the 2 or 4
  images of one ring-walk workgroup, always differ — bright, dim (pixels 0/1), all zero (the
  amax == 0 branch), a single bright pixel, Atari-like, constant (every window an exact tie).
* mixed_returns: advantages of ~0, 1 and 1e3, so per-image gradient magnitudes span ~2^17.
* layer_scaled: conv0..3 scaled by 6, 1/6, 12, 1/12 — four distinct binades, product 1.
"""
import numpy as np

from atari_frames import atari_frames

KINDS = ("random", "dim", "zero", "one_pixel", "atari", "low", "constant", "atari_dim")
LAYER_SCALES = {"conv0/W": 6.0, "conv1/W": 1.0 / 6.0, "conv2/W": 12.0, "conv3/W": 1.0 / 12.0}


def mixed_frames(B, seed, C=4):
    """(uint8 [B, 84, 84, C], kinds int64 [B]) with kinds[n] = n % 8 indexing KINDS."""
    rs = np.random.RandomState(seed)
    atari = atari_frames(B, seed, C=C)
    kinds = np.arange(B, dtype=np.int64) % 8
    out = np.zeros((B, 84, 84, C), np.uint8)
    for n in range(B):
        k = kinds[n]
        if k == 0:
            out[n] = rs.randint(0, 256, size=(84, 84, C))
        elif k == 1:
            out[n] = rs.randint(0, 2, size=(84, 84, C))       # the smallest non-zero magnitude
        elif k == 3:
            out[n, rs.randint(0, 84), rs.randint(0, 84), rs.randint(0, C)] = 255
        elif k == 4:
            out[n] = atari[n]
        elif k == 5:
            out[n] = rs.randint(0, 16, size=(84, 84, C))
        elif k == 6:
            out[n] = 255
        elif k == 7:
            out[n] = atari[n] // 64
    return out, kinds


def return_classes(B):
    """Class (0, 1, 2) of each image's return: period 3 against the kinds' period 8, shifted by
    one, so every (kind, class) pair occurs within 24 images and image 0 is not class 0."""
    return (np.arange(B) + 1) % 3


def mixed_returns(V, seed):
    """float32 R [B] from the oracle's own pred_value V: class 0 R = float32(V) (advantage ~ 0:
    only the entropy gradient remains), class 1 V +- 1, class 2 V +- 1e3."""
    V = np.asarray(V, np.float64)
    rs = np.random.RandomState(seed)
    sign = rs.choice([-1.0, 1.0], size=V.shape[0])
    offset = np.array([0.0, 1.0, 1e3])[return_classes(V.shape[0])]
    return (V + sign * offset).astype(np.float32)


def device_mixed_returns(eng, state, seed):
    """mixed_returns around the engine's own predictor values of `state` (a device tensor; the
    parameters must be loaded): for batches too large to run the oracle's forward first.  The
    forward uses the inference workspace and leaves the training one alone."""
    return mixed_returns(eng.forward(state)[2].cpu().numpy(), seed)


def scaled_params(seed, F=512, S=1, A=4, **kw):
    """The oracle's initialisers x 2 (the parity tests' wscale), then layer_scaled."""
    from oracle import ba3c_oracle as O
    params = O.init_params(F, S, A, seed=seed, dtype=np.float32, **kw)
    return layer_scaled({k: (v * np.float32(2.0)).astype(np.float32) for k, v in params.items()},
                        seed)


def layer_scaled(params, seed=0):
    """A copy of params with conv0..3 in four distinct binades (factors that are no powers of
    two, product 1 so the activations stay in range) and non-zero head biases."""
    rs = np.random.RandomState(seed)
    out = {k: v.copy() for k, v in params.items()}
    for k, s in LAYER_SCALES.items():
        out[k] = (out[k] * out[k].dtype.type(s)).astype(out[k].dtype)
    for k in ("fc-pi/b", "fc-v/b"):
        out[k] = (0.1 * rs.normal(size=out[k].shape)).astype(out[k].dtype)
    return out
