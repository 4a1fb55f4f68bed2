"""conv0's input-gradient kernel (csrc/ba3c_conv0d.h) restated on the host, for the tests of its
persistent walk: the launch arithmetic of run_conv0d / conv0d_kernel, a deal of images whose scale
changes at every step of every workgroup, the element-wise error model the kernel is held to, and a
numpy mirror of its arithmetic that can walk WRONGLY (tests/test_conv0d_walk.py shows that the
checks reject it).  Nothing here is imported from anything compiled.

The walk.  run_conv0d launches grid = min(21 B, 2 CUs) workgroups; workgroup w takes the bands
w, w + grid, ... of the B * 21 (image, band of 4 output rows) pairs, band // 21 the image.  It
loads the next band's dP0 and codes while the current band is in LDS and reads the image's
exponent kd (amax_exp of the image's largest live |dP0|) again in every iteration.
"""
import numpy as np

NBANDS, RB = 21, 4                  # Conv0D::NBANDS, ::RB
CLASSES = (1.0, 1e-6, 1e4, 0.0)     # per-image scales: three distant binades and a black image
PERIODS = (7, 5, 9, 11, 13)
SPOTS = [(y, x) for y in (0, 19, 39) for x in (0, 19, 39)]    # corners, edges, centre (pooled)
BINADES = (1e-6, 1.0, 1e4, 0.0)


def grid_size(B, cus):
    return min(NBANDS * B, 2 * cus)


def walk(B, cus):
    """-> for each workgroup, the list of (image, band row) pairs it visits, in order."""
    grid = grid_size(B, cus)
    return [[divmod(band, NBANDS) for band in range(w, NBANDS * B, grid)] for w in range(grid)]


def smallest_batch(cus, iterations):
    """The smallest B at which some workgroup runs `iterations` iterations."""
    B = 1
    while max(len(v) for v in walk(B, cus)) < iterations:
        B += 1
    return B


def steps(B, cus):
    """The (image before, image after) pairs of different index that some workgroup visits in
    consecutive iterations."""
    return sorted({(a[0], b[0]) for v in walk(B, cus) for a, b in zip(v, v[1:]) if a[0] != b[0]})


def classes_ok(cls, B, cus, both_orders=True):
    """The property deal_classes promises of the class indices `cls` (see there)."""
    st = steps(B, cus)
    zero = CLASSES.index(0.0)
    orders = {(cls[a] == zero, cls[b] == zero) for a, b in st}
    return all(cls[a] != cls[b] for a, b in st) and \
        (not both_orders or {(True, False), (False, True)} <= orders)


def deal_classes(B, cus, both_orders=True):
    """-> int array [B]: image i's index into CLASSES, (i % period) % 4 for the first period of
    PERIODS such that in every workgroup any two consecutively visited images of different index
    are of different classes, and (both_orders) some workgroup steps from a black image to a
    non-black one and some from a non-black one to a black one.  Raises if no period does."""
    for period in PERIODS:
        cls = (np.arange(B) % period) % len(CLASSES)
        if classes_ok(cls, B, cus, both_orders):
            return cls
    raise ValueError("no period of %r separates the images a workgroup visits at B=%d, %d CUs" % (PERIODS, B, cus))


def deal(kind, B, seed=0, scales=None):
    """(dP0 float32 [B,40,40,32], codes): single-K: one element per spot (disjoint footprints) under
    code K; dense: N(0,1), ~30 % dead windows; binades: dense, image i scaled by BINADES[i];
    scales: dense, image i scaled by scales[i]."""
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
        scales = BINADES[:B]
    if scales is not None:
        dp0 *= np.asarray(scales, np.float64)[:, None, None, None]
    return dp0.astype(np.float32), c0


# ---- the error model ---------------------------------------------------------------------------
def live_max(dp0, c0):
    """M_img: each image's largest |dP0| over live windows (code < 4), what conv0d_prep_kernel
    reduces.  -> float64 [B]."""
    return np.where(np.asarray(c0) < 4, np.abs(np.asarray(dp0, np.float64)), 0.0).reshape(len(dp0), -1).max(axis=1)


def exact_and_bound(dp0, c0, w0):
    """-> (exact dX, bound) in float64 from the same dP0, codes and W0.  Derived, not observed
    (it follows test_conv1_input_gradient_within_error_model_of_float64): a dX element is at most
    800 real taps, each evaluated as three plane products (hi hi + hi lo + lo hi, <= 3 x 2^-22
    relative together), accumulated in fp32 by the four waves (n = 3 x 800 roundings) and summed by
    three more fp32 additions; both scale removals are exact powers of two.  With u = 2^-24,
        |got - exact| <= (n u / (1 - n u) + 3 x 2^-22) sum |dY W0| + 2^-28 M_img max |W0|,
    the last term for the elements so far below their image's (tensor's) maximum that fp16 hi + lo
    keeps only an absolute 2^-39 of that maximum: 800 terms, both operands."""
    from ba3c_amd import saliency as S
    exact = S.conv0_input_grad_numpy(dp0, c0, w0)
    mag = S.conv0_input_grad_numpy(np.abs(dp0), c0, np.abs(w0))
    n, u = 3 * 800 + 3, 2.0 ** -24
    wmax = float(np.abs(np.asarray(w0)[:, :, :S.C, :]).max())
    bound = (n * u / (1 - n * u) + 3 * 2.0 ** -22) * mag + 2.0 ** -28 * live_max(dp0, c0)[:, None, None, None] * wmax
    return exact, bound


def ratios(got, exact, bound):
    """Per image, the largest |got - exact| / bound (0 / 0 = 0; inf where a zero bound is exceeded;
    nan where `got` is not finite).  -> float64 [B]."""
    err = np.abs(np.asarray(got, np.float64) - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((err == 0) & (bound == 0), 0.0, err / bound)
    r = r.reshape(len(r), -1)
    return np.where(np.isnan(r).any(axis=1), np.nan, np.where(np.isnan(r), 0.0, r).max(axis=1))


def within_model(got, exact, bound):
    return bool(np.all(ratios(got, exact, bound) <= 1.0))         # a nan fails


def class_report(r, cls):
    """{class scale: the largest ratio among its images}."""
    return {CLASSES[k]: float(r[cls == k].max()) for k in sorted(set(cls.tolist()))}


# ---- a numpy mirror of the kernel's arithmetic, and of a wrong walk -------------------------------
def amax_exp(amax):
    """ba3c_split.h: k with amax 2^k in [2^14, 2^15) (0 for 0), clamped to +-100."""
    if amax == 0:
        return 0
    return int(max(-100, min(100, 14 - int(np.floor(np.log2(float(np.float32(amax))))))))


def split2(x, k):
    """fp16 hi + lo planes of float32(x) 2^k as float64 (split2x2: lo = RN_f16(x 2^k - hi))."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = (np.asarray(x, np.float32) * np.float32(2.0 ** k)).astype(np.float32)
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def mirror(dp0, c0, w0, cus, stale=False):
    """The kernel's dX in numpy: per image kd = amax_exp(live max), per tensor kw, fp16 hi / lo
    planes of both operands, hi hi + hi lo + lo hi (products and sums in float64: the fp32
    accumulation is not mirrored), both scales removed.  stale=True is the WRONG walk the tests
    exist for: from a workgroup's second iteration on, a band whose image differs from the
    previous iteration's has its planes quantised at the PREVIOUS image's exponent (and that
    exponent removed), as if kd were read once per workgroup step too late."""
    from ba3c_amd import saliency as S
    B = len(dp0)
    kd = np.array([amax_exp(m) for m in live_max(dp0, c0)])
    used = np.repeat(kd[:, None], NBANDS, axis=1)                 # exponent applied to (image, band)
    if stale:
        for v in walk(B, cus):
            for (ia, _), (ib, br) in zip(v, v[1:]):
                used[ib, br] = kd[ia]
    w = np.asarray(w0, np.float32)[:, :, :S.C, :]
    kw = amax_exp(np.abs(w).max())
    wh, wl = split2(w, kw)
    dx = np.zeros((B, S.H, S.W, S.C), np.float64)
    for k in np.unique(used):
        imgs = np.flatnonzero((used == k).any(axis=1))
        dh, dl = split2(dp0[imgs], k)
        with np.errstate(invalid="ignore", over="ignore"):
            part = (S.conv0_input_grad_numpy(dh, c0[imgs], wh) + S.conv0_input_grad_numpy(dh, c0[imgs], wl) +
                    S.conv0_input_grad_numpy(dl, c0[imgs], wh)) * 2.0 ** -(int(k) + kw)
        for n, i in enumerate(imgs):
            for br in np.flatnonzero(used[i] == k):
                dx[i, RB * br:RB * br + RB] = part[n, RB * br:RB * br + RB]
    return dx.astype(np.float32)
