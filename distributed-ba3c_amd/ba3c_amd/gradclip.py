"""The clip of the whole gradient's norm (`max_grad_norm`), stated once; the oracle of
gnorm_partials_kernel / gnorm_scale_kernel (csrc/ba3c_small.h, ba3c_clip_grads_global).

    norm = sqrt( sum over every element of every tensor of float64(g)^2 )
    f    = max_norm / norm   if norm > max_norm   else 1.0
    g'   = float32( float64(g) * f )

The alignment gaps of the flat buffer are not elements.  f is float64; a NaN norm compares
false, so f = 1.0 and the NaNs stay where they are.  Where f == 1.0, g' has g's bits.

This is tf.clip_by_global_norm and torch.nn.utils.clip_grad_norm_ up to rounding.  Neither of
those returns the input's bits when nothing is clipped (max_norm * (1 / max_norm) need not be 1,
and torch adds 1e-6 to the norm); this rule does, because the unclipped step must be the step it
was.  The clip replaces the per-tensor clip_by_average_norm(g, 0.1), it does not follow it
(DESIGN.md §19), and at N > 1 every replica clips its own gradient before the sum, as the
reference's per-worker gradient processors do.
"""
import numpy as np


def _sumsq(tensors):
    import math
    parts = []
    for t in tensors:
        x = np.asarray(t, np.float32).astype(np.float64).reshape(-1)
        parts.append(x * x)                                 # exact: float32 x float32 in float64
    if not parts:
        return 0.0
    x = np.concatenate(parts)
    if not np.isfinite(x).all():
        return float(np.sum(x))                             # inf or NaN, as the plain sum gives it
    return math.fsum(x.tolist())                            # the correctly rounded sum


def global_norm_numpy(tensors):
    """The norm of the rule, float64: the square root of the correctly rounded sum of squares."""
    return float(np.sqrt(np.float64(_sumsq(tensors))))


def clip_factor(norm, max_norm):
    """f of the rule (float64); written so that a NaN norm gives 1.0."""
    max_norm = float(max_norm)
    if not (max_norm > 0.0 and np.isfinite(max_norm)):
        raise ValueError("max_norm %r: must be finite and > 0" % max_norm)
    return float(np.float64(max_norm) / np.float64(norm)) if norm > max_norm else 1.0


def clip_numpy(tensors, max_norm):
    """-> ([float64 g * f per tensor], norm, f).  float32 of an entry is the rule's g'; with
    f == 1.0 the entries are the float64 copies of the inputs, so g' has g's bits."""
    norm = global_norm_numpy(tensors)
    f = clip_factor(norm, max_norm)
    out = [np.asarray(t, np.float32).astype(np.float64) * np.float64(f) for t in tensors]
    return out, norm, f
