"""`ba3c_lambda_returns` (csrc/ba3c_rollout.h) against the host statement of ba3c_amd.returns:
the kernel alone through the C ABI, lambda = 1 against `ba3c_nstep_returns`, RolloutBuffer end
to end, the gather beyond 65535 rows, the argument checks and the launcher's three flags.
Index work is exact; R is the float32 cast of the float64 recursion, compared bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REWARDS = [0.0, 1.0, -1.0, 2.0, -3.0, 0.5, 30.0]
SENTINEL = 77


# ---- the kernel alone -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rings(E, T):
    """Random ring contents: every length 0..T, random starts, over and not over."""
    rs = np.random.RandomState(1000 * T + E)
    n = max(E, 1)
    reward = rs.choice(REWARDS, size=(n, T)).astype(np.float64)
    value = (rs.normal(size=(n, T)) * 3).astype(np.float32)
    start = rs.randint(0, T, size=n).astype(np.int32)
    length = rs.randint(0, T + 1, size=n).astype(np.int32)
    over = (rs.rand(n) < 0.4).astype(np.uint8)
    if E >= 37:      # the cases that emit nothing, and a full memory, next to a workgroup edge
        length[[0, 5, 31, 32]] = [0, 1, T, 0]
        over[[5, 31]] = [0, 1]
        length[E - 1], over[E - 1] = 1, 0
        length[E - 2], over[E - 2] = T, 0
    return reward, value, start, length, over


@functools.lru_cache(maxsize=None)
def _host(E, T, gamma, lam):
    """The host statement for every simulator at once: `lambda_step` over arrays is the same
    float64 operations element by element.  Returns (R float32, src, init_R, over, count)."""
    from ba3c_amd.returns import lambda_returns_numpy, lambda_step
    reward, value, start, length, over = _rings(E, T)
    ov = over[:E].astype(bool)
    ln = length[:E].astype(np.int64)
    n = np.where(ov, ln, np.maximum(ln - 1, 0))
    rows = np.arange(E)
    boot = np.where(ov | (ln == 0), np.float32(0), value[rows, (start[:E] + ln - 1) % T]).astype(np.float32)
    R = boot.astype(np.float64)
    v_next = R.copy()
    Rk = np.zeros((E, T), np.float32)
    slotk = np.zeros((E, T), np.int64)
    for k in range(int(n.max()) if E else 0):          # k-th emitted = transition n-1-k
        live = n > k
        slot = (start[:E] + n - 1 - k) % T
        r = reward[rows, slot]
        R = np.where(live, lambda_step(r, v_next, R, gamma, lam), R)
        v_next = np.where(live, value[rows, slot].astype(np.float64), v_next)
        Rk[:, k] = R.astype(np.float32)
        slotk[:, k] = slot
    for e in list(range(min(E, 3))) + [E - 1] * (E > 3):   # the vectorised form is the scalar one
        seg = [(int(start[e]) + i) % T for i in range(int(n[e]))]
        want = lambda_returns_numpy(reward[e, seg], value[e, seg], boot[e], gamma, lam)
        np.testing.assert_array_equal(want[::-1].astype(np.float32), Rk[e, :n[e]])
    mask = np.arange(T)[None, :] < n[:, None]
    e_of = np.broadcast_to(rows[:, None], (E, T))[mask]
    return (Rk[mask], (e_of * T + slotk[mask]).astype(np.int32), boot[e_of], over[:E][e_of],
            int(n.sum()))


def _device(fn_name, E, T, gamma, lam=None):
    from ba3c_amd import _lib as L
    lib = L.load()
    dev = [torch.from_numpy(x).cuda() for x in _rings(E, T)]
    m = max(E * T, 1) + 64                                # slack: nothing may be written there
    R = torch.full((m,), SENTINEL, dtype=torch.float32, device="cuda")
    src = torch.full((m,), SENTINEL, dtype=torch.int32, device="cuda")
    init = torch.full((m,), SENTINEL, dtype=torch.float32, device="cuda")
    ov = torch.full((m,), SENTINEL, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    args = [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)] + [P(t) for t in dev]
    args += [E, T, ctypes.c_double(gamma)] + ([] if lam is None else [ctypes.c_double(lam)])
    args += [P(R), P(src), P(init), P(ov), P(count)]
    L.check(getattr(lib, fn_name)(*args))
    torch.cuda.synchronize()
    c = int(count.item())
    for t in (R, src, init, ov):
        assert bool((t[c:] == SENTINEL).all()), "wrote past count"
    return R[:c].cpu().numpy(), src[:c].cpu().numpy(), init[:c].cpu().numpy(), ov[:c].cpu().numpy(), c


def _same(got, want):
    assert got[4] == want[4], (got[4], want[4])
    np.testing.assert_array_equal(got[1], want[1])                                  # src
    np.testing.assert_array_equal(got[0].view(np.int32), want[0].view(np.int32))    # R, as bits
    np.testing.assert_array_equal(got[2].view(np.int32), want[2].view(np.int32))    # init_R
    np.testing.assert_array_equal(got[3], want[3])                                  # over


@pytest.mark.parametrize("E,T,lam,gamma", [
    (0, 6, 0.95, 0.99), (1, 2, 0.5, 0.99), (1, 129, 0.0, 1.0), (37, 6, 0.95, 0.99),
    (37, 33, 1.0, 0.99), (255, 33, 0.0, 1.0), (255, 129, 0.5, 0.99), (256, 6, 0.5, 0.99),
    (256, 129, 0.95, 1.0), (257, 2, 1.0, 1.0), (257, 33, 0.95, 0.99), (257, 129, 0.95, 1.0),
    (2500, 6, 1.0, 0.99), (2500, 33, 0.5, 1.0), (2500, 129, 0.95, 0.99), (2500, 129, 0.0, 0.99)])
def test_kernel_matches_the_host_statement(E, T, lam, gamma):
    want = _host(E, T, gamma, lam)
    if E >= 37:
        assert 0 < want[4] < E * T
    _same(_device("ba3c_lambda_returns", E, T, gamma, lam), want)


@pytest.mark.parametrize("E,T,gamma", [(37, 6, 0.99), (257, 129, 1.0), (2500, 6, 0.99), (2500, 129, 0.99)])
def test_lambda_one_equals_the_nstep_entry_point(E, T, gamma):
    """If a single R ever differs here, the side that differs from the host statement (checked
    first) is the finding."""
    new = _device("ba3c_lambda_returns", E, T, gamma, 1.0)
    _same(new, _host(E, T, gamma, 1.0))
    _same(new, _device("ba3c_nstep_returns", E, T, gamma))


@pytest.mark.parametrize("lam,gamma", [(-0.1, 0.99), (1.5, 0.99), (float("nan"), 0.99), (0.95, 0.0),
                                       (0.95, float("nan"))])
def test_argument_checks(lam, gamma):
    from ba3c_amd import _lib as L
    with pytest.raises(L.Ba3cLibraryError, match="lambda" if gamma == 0.99 else "gamma"):
        _device("ba3c_lambda_returns", 37, 6, gamma, lam)


# ---- RolloutBuffer end to end -----------------------------------------------------------------
def _encode(E, t, C=4):
    """States whose first two pixels carry (env, step) as little-endian int32."""
    st = np.zeros((E, 84, 84, C), np.uint8)
    for e in range(E):
        st[e, 0, 0, :4] = np.frombuffer(np.int32(e).tobytes(), np.uint8)
        st[e, 0, 1, :4] = np.frombuffer(np.int32(t).tobytes(), np.uint8)
    return st


def _decode(st):
    b = np.ascontiguousarray(st[:, 0, :2, :4]).reshape(-1, 8)
    return [(int(np.frombuffer(x[:4].tobytes(), np.int32)[0]), int(np.frombuffer(x[4:].tobytes(), np.int32)[0]))
            for x in b]


@pytest.mark.parametrize("E,ltm,lam,steps,p_over", [(37, 5, 0.95, 40, 0.08), (9, 20, 0.9, 70, 0.02),
                                                    (300, 2, 0.0, 9, 0.3)])
def test_rollout_buffer_matches_the_host_master(E, ltm, lam, steps, p_over):
    from ba3c_amd.returns import LambdaMasterMirror
    from ba3c_amd.rollout import BatchQueue, RolloutBuffer
    rs = np.random.RandomState(E)
    gamma = 0.995 if ltm == 20 else 0.99
    buf = RolloutBuffer(E, channels=4, local_time_max=ltm, gamma=gamma, gae_lambda=lam)
    assert (buf.T, buf.gae_lambda, buf.gamma) == (ltm + 1, lam, gamma)
    mirror = LambdaMasterMirror(ltm, gamma, lam)
    got, want = [], []
    q = BatchQueue(16)
    batches = []
    for t in range(steps):
        if t > 0:
            rew = rs.choice(REWARDS, size=E).astype(np.float64)
            over = rs.rand(E) < p_over
            for e in range(E):
                mirror.on_message(e, float(rew[e]), bool(over[e]))
            dps = buf.on_reward(torch.from_numpy(rew), torch.from_numpy(over))
            q.put(dps)
            while True:
                b = q.get()
                if b is None:
                    break
                batches.append([x.cpu().numpy() for x in b])
            got.extend(zip(_decode(dps.state.cpu().numpy()), dps.action.cpu().numpy().tolist(),
                           dps.R.cpu().numpy().tolist(), dps.init_R.cpu().numpy().tolist(),
                           dps.over.cpu().numpy().tolist()))
        act = rs.randint(0, 4, size=E).astype(np.int64)
        val = (rs.normal(size=E) * 3).astype(np.float32)
        st = _encode(E, t)
        for e in range(E):
            mirror.on_state(e, (e, t), int(act[e]), val[e])
        buf.on_state(torch.from_numpy(st).cuda(), torch.from_numpy(act).cuda(),
                     torch.from_numpy(val).cuda())
    for k, R, init_r, over in mirror.queue:
        want.append((k["state"], k["action"], float(np.float32(R)), float(np.float32(init_r)), int(over)))
    assert len(got) == len(want) and len(want) > 2 * E
    for g, w in zip(got, want):
        assert g == w, (g, w)
    # BatchData(16): consecutive, in order
    flat = [dp for b in batches for dp in _decode(b[0])]
    assert flat == [w[0] for w in want[:len(flat)]] and len(flat) == 16 * len(batches) > 0


# ---- the gather beyond gridDim.y ----------------------------------------------------------------
@pytest.mark.parametrize("row_bytes", [16, 8])
def test_gather_rows_beyond_65535(row_bytes):
    from ba3c_amd import _lib as L
    lib = L.load()
    n = 70000
    rs = np.random.RandomState(row_bytes)
    rows = rs.randint(0, 2 ** 62, size=(n, row_bytes // 8)).astype(np.int64)
    idx = rs.permutation(n).astype(np.int32)
    d_rows, d_idx = torch.from_numpy(rows).cuda(), torch.from_numpy(idx).cuda()
    out = torch.zeros_like(d_rows)
    L.check(lib.ba3c_gather_rows(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                 ctypes.c_void_p(d_rows.data_ptr()), ctypes.c_void_p(d_idx.data_ptr()),
                                 n, row_bytes, ctypes.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), rows[idx])


# ---- ActorLearner and the launcher --------------------------------------------------------------
def test_actor_learner_feeds_the_lambda_datapoints():
    """As test_actor_learner_runs_and_feeds_the_reference_datapoints, at lambda = 0.95 and
    8-step rollouts: what the learner consumes is what the host master would have queued."""
    from loop_mirror import LoopMirror
    from oracle import ba3c_oracle as O

    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.returns import LambdaMasterMirror
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    E, B = 24, 32
    m = Model(num_actions=4, fc_neurons=128, fc_splits=4, batch_size=B, max_batch=max(B, E))
    m.engine.load_params(O.init_params(128, 4, 4, seed=0, dtype=np.float32))
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    loop = ActorLearner(tr, n_envs=E, batch_size=B, seed=1, local_time_max=8, gae_lambda=0.95)
    assert (loop.buf.T, loop.buf.gae_lambda, loop.buf.gamma) == (9, 0.95, 0.99)
    taps = LoopMirror(loop, LambdaMasterMirror(8, 0.99, 0.95))

    loop.run(40)
    torch.cuda.synchronize()
    assert loop.train_steps >= 4
    assert np.all(np.isfinite(loop.last_scalars.cpu().numpy()))
    want = taps.queued()
    assert taps.consumed == want and len(want) >= B * loop.train_steps


def test_launcher_takes_the_three_flags(tmp_path, monkeypatch):
    """`python -m ba3c_amd.train` on the README's best flags on GridBoxing with 20-step rollouts,
    gamma 0.995 and lambda 0.95: trains to step 6 with a finite cost through a RolloutBuffer of
    21 slots."""
    from ba3c_amd import actor_learner
    from ba3c_amd.train import main
    made = []

    class Spy(actor_learner.ActorLearner):
        def __init__(self, *a, **kw):
            super(Spy, self).__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(actor_learner, "ActorLearner", Spy)
    argv = ("-o adam --use_sync -g 1 -l 0.001 -b 32 --fc_neurons 128 --fc_splits 4 "
            "--epsilon 1e-8 --beta1 0.8 --beta2 0.75 -e GridBoxing-v0 --num_actions 18 "
            "--gae_lambda 0.95 --local_time_max 20 --gamma 0.995 --simulator_procs 32 "
            "--max_steps 6").split()
    argv += ["--models_dir", str(tmp_path / "models"), "--experiment_dir", str(tmp_path / "exp")]
    out = main(argv)
    assert out["global_step"] >= 6 and np.isfinite(out["last"]["cost"])
    assert len(made) == 1
    buf = made[0].buf
    assert (buf.E, buf.T, buf.gae_lambda, buf.gamma) == (32, 21, 0.95, 0.995)
