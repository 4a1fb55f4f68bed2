"""Crafted gradients for the flat clip / optimizer kernels and their fp64 reference.

Pure numpy.  The kernels under test (sumsq / clip / clip_range / update / clip_update in
csrc/ba3c_small.h) take flat buffers, so a test writes `eng.grads`, `eng.params` and the slot
buffers directly; no network pass is involved.  The reference is the oracle's own functors
(oracle/ba3c_oracle.py) on float64 copies of the float32 inputs, with the scalar
hyper-parameter arithmetic (1 - beta, Adam's alpha) kept in float32 as TF-1.2 and the kernels
do it.  The YARDSTICK of a case is the same oracle evaluated in float32 on the same inputs,
measured against the float64 one: the reference's own rounding floor, never the code under
test.

Deals.  A deal gives every tensor of a geometry one gradient kind.  Six kinds and three steps
cannot give every tensor kinds 0, 1 and one of 2 / 3 (that fills a tensor's three steps), so:
  steps 0-2: tensor i takes (0, 1, Z_i)[(i + step) % 3] with Z_i alternating 2, 3 in groups of
             three tensors.  Every tensor, the largest and the 1-element fc-v/b included, sees
             both ends of min(rsqrt(sum g^2) n, 10) where its size allows and a zero or
             tail-only gradient; every deal holds kinds 0, 1, 2 and 3.
  step 3:    kinds 4 and 5 alternate, the largest tensor on kind 4.  N(0,1)*50 has an average
             norm of 50/sqrt(n), under the 0.1 threshold for n > 250 000: the largest tensors
             of `bench` and `over` reach the clipped branch, the one that depends on the sum
             over all their chunks, only through kind 4 (average norm ~ 212/sqrt(n)).
"""
import numpy as np

from oracle import ba3c_oracle as O

f32 = np.float32
f64 = np.float64

UPD_CHUNK = 4096                 # floats per workgroup of the clip / update kernels
FLOOR = 2.0 ** -24               # the yardstick is never taken below half a float32 ulp
YARDSTICK_CAP = 1e-6             # a condition on the inputs (test_flat_updates.py)
GPU_FACTOR = 4.0                 # GPU bound = GPU_FACTOR x the case's yardstick
NSTEPS = 4
CLIP_NORM = f32(0.1)

OPTS = ("adam", "rms", "gd", "momentum", "adagrad", "adadelta")
N_SLOTS = {"adam": 2, "rms": 2, "gd": 0, "momentum": 1, "adagrad": 1, "adadelta": 2}

# named by what they exercise (chunk counts: chunk_count())
GEOMETRIES = {
    "odd": dict(A=31, C=4, F=36, S=1, legacy=False, ps=1),      # tails, 31- and 1-element biases
    "bench": dict(A=4, C=4, F=512, S=1, legacy=False, ps=1),    # fc1: 200 chunks, 4 lane passes
    "legacy": dict(A=18, C=4, F=256, S=1, legacy=True, ps=4),   # 16 tensors, 64-element biases
    "over": dict(A=6, C=12, F=1024, S=4, legacy=False, ps=1),   # more chunks than CUs
}


def tensors(geom):
    """[(name, numel)] of a geometry, in the flat layout's order."""
    g = GEOMETRIES[geom]
    specs = O.param_specs(g["F"], g["S"], g["A"], replace_with_conv=not g["legacy"], ps=g["ps"])
    return [(n, int(np.prod(s))) for n, s in specs]


def chunk_count(numels):
    return int(sum((n + UPD_CHUNK - 1) // UPD_CHUNK for n in numels))


def check_cu_sides(cus, counts):
    """`counts`: {geometry: chunks}.  Both sides of every `nchunks <= CUs` dispatch must be
    taken by some geometry, or the launch forms would silently all be the same one."""
    assert any(c <= cus for c in counts.values()), (cus, counts)
    assert any(c > cus for c in counts.values()), (cus, counts)


# --- hyper-parameters: the fields of ba3c_opt_params (the powers are passed separately) ------
def _hp(lr, **kw):
    h = dict(lr=lr, beta1=0.0, beta2=0.0, epsilon=0.0, decay=0.0, momentum=0.0, rho=0.0)
    h.update(kw)
    return h


HP = {   # [make_optimizer's defaults as test_gpu_parity.py calls it, a second set]
    "adam": [_hp(1e-3, beta1=0.8, beta2=0.75, epsilon=1e-8),
             _hp(1e-3, beta1=0.8, beta2=0.75, epsilon=1e-3)],
    "rms": [_hp(1e-3, decay=0.9, momentum=0.0, epsilon=1e-10),
            _hp(7e-4, decay=0.99, momentum=0.5, epsilon=1e-6)],
    "gd": [_hp(1e-3), _hp(1e-2)],
    "momentum": [_hp(1e-3, momentum=0.9), _hp(1e-3, momentum=0.5)],
    "adagrad": [_hp(1e-3), _hp(1e-2)],
    "adadelta": [_hp(1e-3, rho=0.95, epsilon=1e-3), _hp(0.5, rho=0.9, epsilon=1e-6)],
}
PAIRS = [(o, k) for o in OPTS for k in (0, 1)]


def initial_slots(opt, n):
    """TF-1.2 slot initial values, float32 [n] each (None where the optimizer has no slot)."""
    z = lambda v=0.0: np.full(n, v, f32)
    return {"adam": (z(), z()), "rms": (z(1.0), z()), "gd": (None, None), "momentum": (z(), None),
            "adagrad": (z(0.1), None), "adadelta": (z(), z())}[opt]


def adam_powers(hp, step):
    """beta1^t, beta2^t BEFORE apply number `step` (0-based): TF's float32 variables, which start
    at beta and are multiplied by beta after every apply."""
    b1, b2 = f32(hp["beta1"]), f32(hp["beta2"])
    p1, p2 = b1, b2
    for _ in range(step):
        p1, p2 = f32(p1 * b1), f32(p2 * b2)
    return p1, p2


# --- gradients ---------------------------------------------------------------------------------
KINDS = 6


def gradient(kind, n, rs):
    """float32 [n].  Every magnitude keeps g^2 and sum g^2 inside normal float32 range."""
    if kind == 0:      # average norm far below 0.1: the cap, factor exactly 10
        return (rs.normal(size=n) * 1e-3).astype(f32)
    if kind == 1:      # clipped where 50/sqrt(n) > 0.1
        return (rs.normal(size=n) * 50.0).astype(f32)
    if kind == 2:      # rsqrt(0) = inf: the result is exactly 0
        return np.zeros(n, f32)
    if kind == 3:      # the only mass sits in the tensor's tail chunk
        g = np.zeros(n, f32)
        g[-1] = 7.0
        return g
    if kind == 4:      # sum g^2 dominated by a few terms scattered over the chunks
        return np.ldexp(rs.normal(size=n), rs.randint(-20, 11, size=n)).astype(f32)
    if kind == 5:      # at the threshold: both branches agree to rounding
        return np.full(n, f32(0.1) * np.sqrt(f32(n)), f32)
    raise ValueError(kind)


def deal(geom, step):
    """Kind of every tensor of `geom` at `step` (module docstring)."""
    numels = [n for _, n in tensors(geom)]
    if step < 3:
        return [(0, 1, 2 + (i // 3) % 2)[(i + step) % 3] for i in range(len(numels))]
    big = int(np.argmax(numels))
    return [4 + (i + big) % 2 for i in range(len(numels))]


def deal_scale(geom, step):
    """The unfused-scale test's deal: kinds 0 / 1 / 4."""
    return [(0, 1, 4)[(i + step) % 3] for i in range(len(tensors(geom)))]


def dealt_gradients(geom, step, kinds=None, salt=0):
    """[float32 [numel]] per tensor; the same (geom, step, salt) gives the same bits."""
    kinds = deal(geom, step) if kinds is None else kinds
    gi = sorted(GEOMETRIES).index(geom)
    return [gradient(k, n, np.random.RandomState([977, gi, step, i, salt]))
            for i, (k, (_, n)) in enumerate(zip(kinds, tensors(geom)))]


def initial_params(geom, salt=0):
    gi = sorted(GEOMETRIES).index(geom)
    return [np.random.RandomState([313, gi, i, salt]).normal(0.0, 0.05, size=n).astype(f32)
            for i, (_, n) in enumerate(tensors(geom))]


# --- the reference -----------------------------------------------------------------------------
def clip_as(g, dtype):
    return O.clip_by_average_norm(np.asarray(g, f32).astype(dtype), clip_norm=CLIP_NORM)


def clip64(g):
    """clip_by_average_norm in float64 from the float32 gradient; the constant is float32(0.1)."""
    return clip_as(g, f64)


def clip32(g):
    return clip_as(g, f32)


def took_cap(g, dtype):
    """Whether the oracle in `dtype` multiplied by the cap 1/c, not by rsqrt(sum g^2) n."""
    x = np.asarray(g, f32).astype(dtype)
    c = x.dtype.type(CLIP_NORM)
    return bool(np.array_equal(clip_as(g, dtype), (x * c) * (x.dtype.type(1.0) / c)))


def apply_as(dtype, opt, p, g, s0, s1, hp, powers=None):
    """The oracle's functor of `opt` on `dtype` copies -> (p, s0, s1).  Hyper-parameters enter
    as float32 values, so 1 - beta, 1 - rho and Adam's alpha are float32 arithmetic."""
    c = lambda x: None if x is None else np.asarray(x).astype(dtype)
    p, g, s0, s1 = c(p), c(g), c(s0), c(s1)
    h = {k: f32(v) for k, v in hp.items()}
    if opt == "adam":
        return O.apply_adam(p, g, s0, s1, h["lr"], h["beta1"], h["beta2"], h["epsilon"],
                            f32(powers[0]), f32(powers[1]))
    if opt == "rms":
        q, ms, mom = O.apply_rmsprop(p, g, s0, s1, h["lr"], decay=h["decay"],
                                     momentum=h["momentum"], eps=h["epsilon"])
        return q, ms, mom
    if opt == "gd":
        return O.apply_gd(p, g, h["lr"]), None, None
    if opt == "momentum":
        q, acc = O.apply_momentum(p, g, s0, h["lr"], momentum=h["momentum"])
        return q, acc, None
    if opt == "adagrad":
        q, acc = O.apply_adagrad(p, g, s0, h["lr"])
        return q, acc, None
    if opt == "adadelta":
        return O.apply_adadelta(p, g, s0, s1, h["lr"], rho=h["rho"], eps=h["epsilon"])
    raise ValueError(opt)


def apply64(opt, p, g, s0, s1, hp, powers=None):
    return apply_as(f64, opt, p, g, s0, s1, hp, powers)


def apply32(opt, p, g, s0, s1, hp, powers=None):
    return apply_as(f32, opt, p, g, s0, s1, hp, powers)


# --- error measures (max-normalised, per tensor) -------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def norm_err(got, ref64):
    """max|got - ref| / max|ref|; a zero reference must come back exactly zero."""
    ref64 = np.asarray(ref64, f64)
    den = np.abs(ref64).max()
    if den == 0:
        return 0.0 if not np.any(got) else float("inf")
    return float(np.abs(np.asarray(got, f64) - ref64).max() / den)


def param_err(got, p64, p_before):
    """max(|got - p64| - ulp32(p64)/2) / max|p64 - p_before|: the final rounding of p to
    float32 is nobody's error, what is left is the error of the update.  Where the float64
    update of the whole tensor is 0, `got` must equal p_before bit for bit."""
    p64 = np.asarray(p64, f64)
    den = np.abs(p64 - np.asarray(p_before, f64)).max()
    if den == 0:
        return 0.0 if same_bits(got, p_before) else float("inf")
    half = 0.5 * np.spacing(np.abs(p64).astype(f32)).astype(f64)
    return float(max((np.abs(np.asarray(got, f64) - p64) - half).max(), 0.0) / den)


MEASURES = ("p", "s0", "s1")


def update_errs(got, ref64, p_before):
    """{measure: error} of one tensor's (p, s0, s1) against the float64 result."""
    e = {"p": param_err(got[0], ref64[0], p_before)}
    for k, i in (("s0", 1), ("s1", 2)):
        if ref64[i] is not None:
            e[k] = norm_err(got[i], ref64[i])
    return e


def floor(y):
    return max(float(y), FLOOR)


def reference_update(opt, hp, g_raw, p, s0, s1, powers=None, scale=None, clipped=None):
    """One tensor, one step.  scale None: the fused clip (`clipped`: its (clip64, clip32) where
    the caller has them already); else the unfused apply's float32(g * float32(scale)).
    Returns (float64 result, its yardstick errors)."""
    if scale is None:
        g64, g32 = clipped if clipped is not None else (clip64(g_raw), clip32(g_raw))
    else:
        g32 = (np.asarray(g_raw, f32) * f32(scale)).astype(f32)
        g64 = g32.astype(f64)
    r64 = apply64(opt, p, g64, s0, s1, hp, powers)
    r32 = apply32(opt, p, g32, s0, s1, hp, powers)
    assert all(x is None or x.dtype == f32 for x in r32), "the float32 oracle left float32"
    return r64, update_errs(r32, r64, p)


# --- flat buffers --------------------------------------------------------------------------------
def pack(layout, flat_size, per_tensor, gap):
    """float32 [flat_size]: the tensors at their offsets, `gap` in the alignment gaps."""
    flat = np.full(flat_size, gap, f32)
    for (_, off, numel, _), v in zip(layout, per_tensor):
        flat[off:off + numel] = np.asarray(v, f32).reshape(-1)
    return flat


def unpack(layout, flat):
    return [flat[off:off + numel] for _, off, numel, _ in layout]


def gap_mask(layout, flat_size):
    m = np.ones(flat_size, bool)
    for _, off, numel, _ in layout:
        m[off:off + numel] = False
    return m
