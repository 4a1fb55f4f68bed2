"""The FC stage (fc1, the two heads, the loss and their backward) in float64, stated once.

Pure numpy.  The stage starts at conv3's output a3 [B,1600] and ends at dY3 [B,1600]; every
function takes the arrays it starts from as arguments, so a GPU test can feed each product the
GPU's own inputs (its a3, its h, its dh) and hold that one product to float64 on its arithmetic
alone — no convolution is evaluated and no pooling decision can differ.  The formulas are the
oracle's (oracle/ba3c_oracle.py: get_nn_prediction, build_graph_cost, backward,
_backward_from_heads); tests/test_fc_stage.py pins every one of them to it.

Every matrix product comes with its magnitude sum, sum_k |a_k| |b_k| per output: the scale an
element-wise error bound has to be stated in.


The element-wise bound (within_model)
-------------------------------------
csrc/ba3c_gemm6.h evaluates an fp32 product a * b as six bf16 MFMAs: each operand is split
exactly into three bf16 planes (a = a0 + a1 + a2, 8 + 8 + 8 significand bits), the six plane
products of weight >= 2^-16 are kept, and the three dropped ones (a1 b2, a2 b1, a2 b2) are
together below 2^-23 |a| |b|.  Every kept plane product is exact in fp32 (8 x 8 bits) and is
ADDED to an fp32 accumulator, so an output that sums K products is a chain of 6 K fp32
additions, and the launch adds P further ones when it combines partial sums (the parity sets
or the two k-groups of a workgroup, the split-K slabs, the reduction's lane groups, the legacy
bias).  With u = 2^-24 and the standard summation bound (Higham, Accuracy and Stability of
Numerical Algorithms, §4.2: any order of n additions of terms t_i errs by at most
gamma_{n-1} sum |t_i|, gamma_n = n u / (1 - n u)) the bound is

    |got - exact| <= (gamma_n + 2^-23 + extra) * sum_k |a_k| |b_k| + K * 2^-126,
    n = 6 K + P,  gamma_n = n u / (1 - n u),  u = 2^-24.

  * gamma_n is stated over sum_k |a_k| |b_k|, the magnitude of the products themselves, not
    over the plane products' (whose magnitudes can exceed |a b| by 2^-7 relative when planes
    differ in sign).  That second-order term, 2^-7 gamma_n, is NOT added: the bound is kept as
    the model states it, and a case that needed it would be reported, not absorbed.

  * 2^-23: the dropped plane products.
  * extra: a rounding of an INPUT that the reference does not see (the head weight gradient
    reads the float32-rounded [dz | dV] row while the reference uses its float64 one: 2^-23).
  * K * 2^-126: a product or partial sum in the subnormal range is not relatively accurate;
    each of the K terms may lose up to the smallest normal float32.
  * P is not computed per launch but bounded by 64 for every product here: at B <= 257 the
    weight-gradient plans (plan_wgrad in csrc/ba3c_capi.hip) take at most 3 split-K slabs of
    fc1 and 3 of the heads, the reduction adds them in 4 lane groups (+ 3), a workgroup sums two
    k-groups or parity sets (+ 1), fc1's forward adds FC_SPLIT = 5 chunks of two k-groups
    (+ 9) and the legacy bias (+ 1): under 20 in all.  64 leaves room for a plan change without
    loosening the bound measurably (gamma grows by 64 u = 3.8e-6 relative to 6 K u).
  * The fp32-MFMA engine (BA3C_GENERIC=1) has exact products and fp32 accumulation: K + P
    additions, inside the same bound.
  * The final store is the accumulator itself (no further rounding); the ReLU of the legacy FC
    and the ReluGrad mask of dY3 are contractions / exact selections.

K per product: 1600 for h, F for dY3, B for the weight gradients.
"""
import numpy as np

from oracle import ba3c_oracle as O

f64 = np.float64
U = 2.0 ** -24
DROPPED = 2.0 ** -23             # the three dropped bf16 plane products of ba3c_gemm6.h
TINY = 2.0 ** -126               # smallest normal float32
P_MAX = 64                       # partial-sum additions on top of the 6 K (docstring)
STORED_ROW = 2.0 ** -23          # `extra` of the head gradients: the float32 [dz | dV] row


def gamma(n):
    return n * U / (1.0 - n * U)


def bound(mag, K, extra=0.0, P=P_MAX):
    """The element-wise bound of the docstring for outputs with magnitude sums `mag`."""
    return (gamma(6 * K + P) + DROPPED + extra) * np.asarray(mag, f64) + K * TINY


def model_ratio(got, exact, mag, K, extra=0.0):
    """max |got - exact| / bound (below 1: inside the model).  A NaN anywhere gives inf."""
    got, exact = np.asarray(got, f64), np.asarray(exact, f64)
    assert got.shape == exact.shape == np.shape(mag), (got.shape, exact.shape, np.shape(mag))
    r = np.abs(got - exact) / bound(mag, K, extra)
    return float("inf") if not np.all(np.isfinite(r)) else float(r.max()) if r.size else 0.0


def within_model(got, exact, mag, n, extra=0.0):
    """Every element of `got` within the error model of `exact` (n = K, the products summed)."""
    return model_ratio(got, exact, mag, n, extra) < 1.0


def normwise(got, ref):
    """test_gpu_parity.rel: max |got - ref| / max |ref| (the absolute error where ref is 0)."""
    a, b = np.asarray(got, f64), np.asarray(ref, f64)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / den) if den > 0 else float(np.abs(a - b).max())


# --- the config ---------------------------------------------------------------------------
def is_legacy(cfg):
    return not cfg.get("replace_with_conv", True)


def splits(cfg):
    """(number of fc1 tensors, columns of each)."""
    s = cfg.get("ps", 1) if is_legacy(cfg) else cfg["fc_splits"]
    return s, cfg["fc_neurons"] // s


def create_rule_ok(F, s, A):
    """ba3c_create's geometry rule (csrc/ba3c_capi.hip): 1 <= A < MAXA = 32, F >= 4 and F a
    multiple of 4 x the number of fc1 tensors."""
    return 1 <= A <= 31 and s >= 1 and F >= 4 and F % s == 0 and (F // s) % 4 == 0


def fc1_matrix(params, cfg):
    """(W1 [1600,F], bias [F] or None) in float64."""
    F = cfg["fc_neurons"]
    s, per = splits(cfg)
    if not is_legacy(cfg):
        return O.fc1_weight_matrix(params, F, s).astype(f64), None
    W1 = np.concatenate([params["fc1_%d/W" % i] for i in range(s)], axis=1).astype(f64)
    b = np.concatenate([params["fc1_%d/b" % i] for i in range(s)]).astype(f64)
    return W1, b


# --- forward --------------------------------------------------------------------------------
def fc1_forward(params, cfg, a3):
    """h_pre = a3 @ W1 (+ b), h (ReLU for the legacy FC) and the magnitude sums of h_pre."""
    a3 = np.asarray(a3, f64)
    W1, b = fc1_matrix(params, cfg)
    h_pre = a3 @ W1
    mag = np.abs(a3) @ np.abs(W1)
    if b is not None:
        h_pre = h_pre + b
        mag = mag + np.abs(b)
    return {"h_pre": h_pre, "h": O.relu(h_pre) if b is not None else h_pre, "mag": mag}


def heads_forward(params, h, explore_factor=1.0):
    """policy, logits (the softmax), logitsT, pred_value from a given h; `value_mag` is the
    magnitude sum of V = h.Wv + b (test_gpu_parity.value_err's scale)."""
    h = np.asarray(h, f64)
    Wp, bp = params["fc-pi/W"].astype(f64), params["fc-pi/b"].astype(f64)
    Wv, bv = params["fc-v/W"].astype(f64), params["fc-v/b"].astype(f64)
    policy = h @ Wp + bp
    return {"policy": policy, "logits": O.softmax(policy),
            "logitsT": O.softmax(policy * f64(explore_factor)),
            "pred_value": (h @ Wv + bv)[:, 0],
            "value_mag": (np.abs(h) @ np.abs(Wv))[:, 0] + abs(float(bv[0]))}


def loss_backward(params, h, action, R, entropy_beta=0.01):
    """dz [B,A], dV [B] and the seven scalars of SCALAR_NAMES[:7] from a given h:
    O.build_graph_cost's loss and O.backward's dz / dV."""
    fw = heads_forward(params, h)
    p, V = fw["logits"], fw["pred_value"]
    R = np.asarray(R, f64)
    B, A = f64(p.shape[0]), p.shape[1]
    beta = f64(entropy_beta)
    logp = np.log(p + O.LOG_EPS)
    onehot = np.eye(A, dtype=f64)[np.asarray(action)]
    adv = V - R
    policy_loss = ((logp * onehot).sum(axis=1) * adv).sum()
    xent = (p * logp).sum()
    value_loss = ((V - R) ** 2).sum() / 2.0
    scalars = [(policy_loss + xent * beta + value_loss) / B,
               policy_loss * O.MONITOR_SCALE / B,
               xent * O.MONITOR_SCALE / B * beta,
               value_loss * O.MONITOR_SCALE / B,
               adv.mean(), V.mean(), p.max()]
    gp = (adv[:, None] * onehot / (p + O.LOG_EPS) + beta * (logp + p / (p + O.LOG_EPS))) / B
    dz = p * (gp - (gp * p).sum(axis=1, keepdims=True))
    dV = (V - R) / B
    return {"dz": dz, "dV": dV, "scalars": [float(s) for s in scalars]}


# --- backward -------------------------------------------------------------------------------
def head_dh(params, cfg, dz, dV, h):
    """dh = dz Wpi^T + dV Wv^T, masked by h > 0 for the legacy FC (h > 0 <=> h_pre > 0)."""
    dz, dV = np.asarray(dz, f64), np.asarray(dV, f64)
    Wp, Wv = params["fc-pi/W"].astype(f64), params["fc-v/W"].astype(f64)
    dh = dz @ Wp.T + dV[:, None] @ Wv.T
    mag = np.abs(dz) @ np.abs(Wp).T + np.abs(dV)[:, None] @ np.abs(Wv).T
    if is_legacy(cfg):
        keep = np.asarray(h) > 0
        dh, mag = dh * keep, mag * keep
    return dh, mag


def fc1_dgrad(params, cfg, dh, a3):
    """dY3 = (dh @ W1^T) . (a3 > 0) and its magnitude sums (both zero where a3 <= 0)."""
    dh, keep = np.asarray(dh, f64), np.asarray(a3) > 0
    W1, _ = fc1_matrix(params, cfg)
    return (dh @ W1.T) * keep, (np.abs(dh) @ np.abs(W1).T) * keep


def fc1_wgrad(cfg, a3, dh):
    """{tensor name: (gradient, magnitude sums)} of fc1 in the tensors' own shapes:
    a3^T @ dh per split, and the column sums of dh for the legacy biases."""
    a3, dh = np.asarray(a3, f64), np.asarray(dh, f64)
    s, per = splits(cfg)
    dW, mW = a3.T @ dh, np.abs(a3).T @ np.abs(dh)
    out = {}
    for i in range(s):
        sl = slice(i * per, (i + 1) * per)
        shape = (1600, per) if is_legacy(cfg) else (5, 5, 64, per)
        out["fc1_%d/W" % i] = (dW[:, sl].reshape(shape), mW[:, sl].reshape(shape))
        if is_legacy(cfg):
            out["fc1_%d/b" % i] = (dh[:, sl].sum(axis=0), np.abs(dh[:, sl]).sum(axis=0))
    return out


def head_wgrad(h, dz, dV):
    """{tensor name: (gradient, magnitude sums)} of the two heads: h^T dz, sum dz, h^T dV,
    sum dV."""
    h, dz, dV = np.asarray(h, f64), np.asarray(dz, f64), np.asarray(dV, f64)[:, None]
    ah = np.abs(h)
    return {"fc-pi/W": (h.T @ dz, ah.T @ np.abs(dz)),
            "fc-pi/b": (dz.sum(axis=0), np.abs(dz).sum(axis=0)),
            "fc-v/W": (h.T @ dV, ah.T @ np.abs(dV)),
            "fc-v/b": (dV.sum(axis=0), np.abs(dV).sum(axis=0))}


# --- the geometries of tests/test_gpu_fc_shapes.py ------------------------------------------
# each is the smallest case of something (the table in DESIGN.md §4)
GEOMETRIES = {
    "g1": dict(A=1, C=4, F=4, S=1),                          # minimum F, one action
    "g2": dict(A=5, C=4, F=36, S=3),                         # split boundaries inside one chunk
    "g3": dict(A=4, C=4, F=68, S=1),                         # 4 valid lanes of chunk 2; dgrad K tail
    "g4": dict(A=9, C=4, F=100, S=5),                        # first A of the <= 16 exit
    "g5": dict(A=16, C=4, F=132, S=3),                       # last A of it; 128-wide tile + 4
    "g6": dict(A=4, C=4, F=192, S=4),                        # runtime-A form with four actions
    "g7": dict(A=4, C=4, F=260, S=1),                        # 4 valid lanes of chunk 5 of 8
    "g8": dict(A=17, C=4, F=500, S=5),                       # first A past the <= 16 exit
    "g9": dict(A=31, C=4, F=516, S=3),                       # runtime feature loop; A + 1 = MAXA
    "g10": dict(A=8, C=4, F=1028, S=1),                      # last A of the <= 8 exit; 8 x 128 + 4
    "g11": dict(A=5, C=4, F=132, S=1, legacy=True, ps=3),    # bias + ReLU across a split boundary
    "g12": dict(A=4, C=4, F=68, S=1, legacy=True, ps=1),     # preloaded legacy bias with a tail
    "g13": dict(A=3, C=12, F=72, S=2),                       # separate launches (C = 12), N tail
}


def n_splits(g):
    return g["ps"] if g.get("legacy") else g["S"]


def heads_form(F, A):
    """(FCH, AT) of the heads_kernel<FCH, NZ, AT, LOSS> that ba3c_capi.hip:launch_heads
    launches for (F, A) with either loss (A3C, PPO): FCH 64-lane feature chunks unrolled (0: the runtime loop), AT the
    compile-time action count (0: runtime)."""
    if A == 4 and 64 < F <= 128:
        return (2, 4)
    if A == 4 and 256 < F <= 512:
        return (8, 4)
    for fch in (1, 2, 4, 8):
        if F <= 64 * fch:
            return (fch, 0)
    return (0, 0)


ALL_HEADS_FORMS = {(2, 4), (8, 4), (1, 0), (2, 0), (4, 0), (8, 0), (0, 0)}


def reduce_exit(A):
    """The exit ba3c_gemm.h:wave_reduce_d takes for w = A lanes: after the two quad steps
    (w <= 4), the half-row mirror (w <= 8), the row mirror (w <= 16), or the full wave (64)."""
    return 4 if A <= 4 else 8 if A <= 8 else 16 if A <= 16 else 64
