"""The clipped-surrogate (PPO, Schulman et al. 2017) loss on the host and the pool that replays a
rollout: the one statement that the heads kernel's PPO form (`ba3c_train_grads_ppo`) computes,
and its oracle.  numpy, float64; torch is imported only where the pool moves device tensors.

Per sample the inputs are the action a, the return R (the value target: the A3C
`futurereward`), V_old (the predictor's value when the action was taken), l_old =
log(pi_old(a) + 1e-6), the clip eps and beta.  With p = softmax(z), lp = log(p + 1e-6),
lpa = lp[a] and the current value V:

    Adv  = R - V_old                         (a constant of the sample; no gradient)
    rho  = exp(lpa - l_old)
    s    = -min(rho * Adv, clip(rho, 1 - eps, 1 + eps) * Adv)
    cost = ( sum_n s  +  beta * sum_n sum_k p_k lp_k  +  1/2 sum_n (V - R)^2 ) / B

The entropy and value terms, the 1e-6, the division by B and the *128/B scaling of the monitored
scalars are the A3C loss's (model.py, train.py:305-327); only the policy term differs.  Its
gradient in closed form:

    active = (rho * Adv <= clip(rho, 1 - eps, 1 + eps) * Adv)     # a tie takes the unclipped branch
    c      = active ? -Adv * rho : 0
    dL/dp_k = ( c * [k == a] / (p_k + 1e-6) + beta * (lp_k + p_k / (p_k + 1e-6)) ) / B
    dz_k    = p_k * (dL/dp_k - sum_j p_j dL/dp_j)
    dV      = (V - R) / B

which is the A3C gradient with its advantage factor V - R replaced by c: at rho = 1 and
V_old = V they are equal.

Three further pieces, each off by default (ba3c_train_grads_ppo_ext, ba3c_ppo_norm_adv and the
learner's loop; baselines ppo2, CleanRL, SB3 and Spinning Up carry the same three):

Advantage normalisation, per minibatch (normalise_adv_numpy).  Over the B rows of one step

    mean = sum_n Adv / B,   std = sqrt(sum_n (Adv - mean)^2 / B)      (population form, two passes)
    A_n  = float32((Adv_n - mean) / (std + 1e-8))                     (B = 1 gives 0)

is written into the rows' fourth float, and a step told to take its advantage from the row
(`adv`, `adv_from_row`) uses A_n wherever the policy term has Adv; R and V_old keep their other
uses.

The clipped value loss (`vclip` > 0).  With d = V - V_old:

    outside     = |d| > vclip
    Vc          = outside ? V_old + sign(d) * vclip : V               (V exactly when inside)
    use_clipped = outside and (Vc - R)^2 > (V - R)^2                  # a tie takes the unclipped branch
    value term  = 1/2 sum_n (use_clipped ? (Vc - R)^2 : (V - R)^2)    = 1/2 sum_n max of the two
    dV          = use_clipped ? 0 : (V - R) / B

Term 2 of the kernel's per-sample terms and the value_loss scalar take the selected square; term 3
(and the advantage scalar) stays V - R.

The KL stop (should_stop, stop_kl).  The learner accumulates, over an epoch's minibatches, the
mean of

    stop_kl = mean_n((rho - 1) - log rho)

and with a target_kl > 0 a pool's remaining epochs are abandoned once that epoch mean is not
<= target_kl (a non-finite mean stops too).  (rho - 1) - log rho is the sample estimate of
KL(pi_old || pi) that is >= 0 for every sample and 0 only at rho = 1 (Schulman, "Approximating KL
divergence", k3; CleanRL's and SB3's stop use it).  mean(-log rho) — approx_kl, the
ppo_approx_kl channel, which stays as it is — has the same expectation but either sign on a
minibatch: on GridBoxing at B = 8 it was negative in 23 of 33 epochs, some at -1.7e-2, and a stop
on it never fired in those.
"""
import collections

import numpy as np

LOG_EPS = 1e-6            # train.py:305
MONITOR_SCALE = 128.0     # train.py:311

# An ActorLearner's PPO setting (--ppo_clip / --ppo_epochs / --ppo_minibatches)
# and its optional pieces (--ppo_norm_adv / --ppo_vclip / --ppo_target_kl), off by default
Setting = collections.namedtuple("Setting", ["clip", "epochs", "minibatches", "norm_adv", "vclip",
                                             "target_kl"], defaults=(False, 0.0, 0.0))
DEFAULT_EPOCHS = 4
DEFAULT_MINIBATCHES = 4


def softmax(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def make_rows(R, v_old, l_old):
    """The kernel's per-sample input: float32 [n, 4] = {R, V_old, l_old, 0}."""
    R = np.asarray(R)
    rows = np.zeros((R.shape[0], 4), dtype=np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2] = R, v_old, l_old
    return rows


def normalise_adv_numpy(rows):
    """(rows_out, mean, std): a copy of the float32 rows [B, 4] whose column 3 holds the
    normalised advantage float32((Adv - mean) / (std + 1e-8)), Adv = float64(R) - float64(V_old),
    with the batch's mean and population std (two passes, float64).  Columns 0-2 are untouched."""
    rows = np.asarray(rows, dtype=np.float32)
    B = rows.shape[0]
    adv = rows[:, 0].astype(np.float64) - rows[:, 1].astype(np.float64)
    mean = adv.sum() / B
    std = np.sqrt(((adv - mean) ** 2).sum() / B)
    out = rows.copy()
    out[:, 3] = ((adv - mean) / (std + 1e-8)).astype(np.float32)
    return out, float(mean), float(std)


def should_stop(epoch_kl, target_kl):
    """Whether a pool's remaining epochs are abandoned: never with target_kl == 0, else unless
    epoch_kl <= target_kl (so a NaN or an infinite KL stops)."""
    if target_kl == 0:
        return False
    return not (epoch_kl <= target_kl)


def heads_numpy(z, V, action, R, v_old, l_old, eps, beta=0.01, vclip=0.0, adv=None):
    """The loss and its closed-form gradient from the policy pre-activations z [B, A] and the
    current values V [B].  Returns a dict: cost, dz [B, A], dV [B], rho, active, c, s, the
    kernel's per-sample terms [B, 6] = {s, sum_k p lp, (V-R)^2, V - R, V, max p} and the eight
    step scalars in _lib.SCALAR_NAMES order without active_relus (scalars [7]).
    adv [B]: replaces R - V_old in the policy term; vclip > 0: the clipped value loss (term 2,
    value_loss and dV, as the module states); use_clipped [B] says where."""
    z = np.asarray(z, dtype=np.float64)
    V, R = np.asarray(V, dtype=np.float64), np.asarray(R, dtype=np.float64)
    v_old, l_old = np.asarray(v_old, dtype=np.float64), np.asarray(l_old, dtype=np.float64)
    action = np.asarray(action, dtype=np.int64)
    B, A = z.shape
    eps, beta = float(eps), float(beta)
    p = softmax(z)
    pe = p + LOG_EPS
    lp = np.log(pe)
    ar = np.arange(B)
    lpa = lp[ar, action]
    Adv = R - v_old if adv is None else np.asarray(adv, dtype=np.float64)
    rho = np.exp(lpa - l_old)
    su = rho * Adv
    sc = np.clip(rho, 1.0 - eps, 1.0 + eps) * Adv
    active = su <= sc
    s = -np.minimum(su, sc)
    c = np.where(active, -Adv * rho, 0.0)
    onehot = np.zeros((B, A), dtype=np.float64)
    onehot[ar, action] = 1.0
    gp = (c[:, None] * onehot / pe + beta * (lp + p / pe)) / B
    dz = p * (gp - (gp * p).sum(axis=1, keepdims=True))
    dV = (V - R) / B
    vsq = (V - R) ** 2
    use_clipped = np.zeros(B, dtype=bool)
    vclip = float(vclip)
    if vclip > 0.0:
        d = V - v_old
        outside = np.abs(d) > vclip
        Vc = np.where(outside, v_old + np.sign(d) * vclip, V)
        use_clipped = outside & ((Vc - R) ** 2 > vsq)
        vsq = np.where(use_clipped, (Vc - R) ** 2, vsq)
        dV = np.where(use_clipped, 0.0, dV)
    xent = (p * lp).sum(axis=1)
    terms = np.stack([s, xent, vsq, V - R, V, p.max(axis=1)], axis=1)
    pl, xe, vl = s.sum(), xent.sum(), 0.5 * vsq.sum()
    cost = (pl + beta * xe + vl) / B
    scalars = np.array([cost, pl * MONITOR_SCALE / B, xe * MONITOR_SCALE / B * beta,
                        vl * MONITOR_SCALE / B, (V - R).mean(), V.mean(), p.max()])
    return dict(cost=cost, dz=dz, dV=dV, rho=rho, active=active, c=c, s=s, terms=terms,
                scalars=scalars, p=p, lp=lp, use_clipped=use_clipped)


def heads_from_h(h, params, action, rows, eps, beta=0.01, vclip=0.0, adv_from_row=False):
    """heads_numpy on an FC output h [B, F] and the head weights of a {name: array} dict, with the
    kernel's rows [B, 4]; adds dh = dz W_pi^T + dV W_v^T (before any legacy ReLU mask).
    adv_from_row: the policy term's advantage is rows[:, 3]."""
    f8 = lambda x: np.asarray(x, dtype=np.float64)
    h, rows = f8(h), f8(rows)
    z = h @ f8(params["fc-pi/W"]) + f8(params["fc-pi/b"])
    V = (h @ f8(params["fc-v/W"]) + f8(params["fc-v/b"]))[:, 0]
    out = heads_numpy(z, V, action, rows[:, 0], rows[:, 1], rows[:, 2], eps, beta, vclip,
                      rows[:, 3] if adv_from_row else None)
    out["dh"] = out["dz"] @ f8(params["fc-pi/W"]).T + out["dV"][:, None] @ f8(params["fc-v/W"]).T
    out["V"] = V
    return out


def clip_fraction(rho, eps):
    """mean(|rho - 1| > eps)."""
    return float(np.mean(np.abs(np.asarray(rho, dtype=np.float64) - 1.0) > eps))


def approx_kl(rho):
    """mean(-log rho): the sample estimate of KL(pi_old || pi)."""
    return float(np.mean(-np.log(np.asarray(rho, dtype=np.float64))))


def stop_kl(rho):
    """mean((rho - 1) - log rho): the KL stop's estimate of KL(pi_old || pi), >= 0 per sample."""
    rho = np.asarray(rho, dtype=np.float64)
    return float(np.mean((rho - 1.0) - np.log(rho)))


def stop_kl_device(rho):
    """stop_kl of a torch tensor as a float64 scalar on the tensor's device; no host read."""
    import torch
    rho = rho.double()
    return ((rho - 1.0) - torch.log(rho)).mean()


def device_gather(src, idx):
    """src[idx] along the first axis with `ba3c_gather_rows` (rows of any byte size the kernel
    moves: states, 8-byte actions, 16-byte rows); idx: an int32 device tensor."""
    import ctypes

    import torch

    from . import _lib
    lib = _lib.load()
    n = int(idx.shape[0])
    src = src.contiguous()
    out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    row = src.element_size() * int(np.prod(src.shape[1:], dtype=np.int64))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ba3c_gather_rows(stream, ptr(src), ptr(idx), n, row, ptr(out)))
    return out


class Pool(object):
    """Replays a rollout: collects datapoints (rollout.Datapoints with `rows`) in arrival order;
    once it holds N = minibatches * batch_size of them it takes the first N (the rest wait for
    the next pool) and yields epochs * minibatches minibatches (state, action, rows).  Epoch k's
    order is the k-th `permutation(N)` of the pool's own RandomState(seed) — no other
    generator's sequence moves — and its minibatch j is perm_k[jB:(j+1)B], gathered on the
    device (`gather`, default device_gather); only the permutation indices pass through the host."""

    FIELDS = ("state", "action", "rows")

    def __init__(self, batch_size, minibatches=DEFAULT_MINIBATCHES, epochs=DEFAULT_EPOCHS, seed=0,
                 gather=None):
        self.B, self.M, self.K = int(batch_size), int(minibatches), int(epochs)
        if self.B < 1 or self.M < 1 or self.K < 1:
            raise ValueError("batch_size, minibatches and epochs must be >= 1")
        self.N = self.M * self.B
        self.rs = np.random.RandomState(seed)
        self.gather = gather or device_gather
        self._parts = []
        self._n = 0
        self.last_perms = None            # the index arrays of the pool taken last (tests, tools)

    def put(self, dps):
        if len(dps):
            if getattr(dps, "rows", None) is None:
                raise ValueError("the pool needs datapoints with rows (RolloutBuffer(logp=True))")
            self._parts.append(tuple(getattr(dps, k) for k in self.FIELDS))
            self._n += len(dps)

    def __len__(self):
        return self._n

    def get(self):
        """None while fewer than N datapoints wait; else an iterator over the next pool's
        epochs * minibatches minibatches (state, action, rows).  The pool is taken, and its
        permutations drawn, when get() returns."""
        if self._n < self.N:
            return None
        import torch
        fields = [torch.cat([p[i] for p in self._parts]) for i in range(len(self.FIELDS))]
        N = self.N
        taken = [f[:N] for f in fields]
        self._n -= N
        self._parts = [tuple(f[N:] for f in fields)] if self._n else []
        perms = [self.rs.permutation(N) for _ in range(self.K)]
        self.last_perms = perms
        return self._minibatches(taken, perms)

    def _minibatches(self, taken, perms):
        import torch
        dev = taken[0].device
        for perm in perms:
            idx = torch.from_numpy(perm.astype(np.int32)).to(dev)
            for j in range(self.M):
                sel = idx[j * self.B:(j + 1) * self.B]
                yield tuple(self.gather(f, sel) for f in taken)
