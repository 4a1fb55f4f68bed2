"""lambda-returns on the host (ba3c_amd.returns): the statement the GPU kernel, RolloutBuffer
and SimulatorMaster._parse_memory share, pinned against the reference's `_parse_memory` as the
oracle restates it at lambda = 1, against clip(r) + gamma * V_next at lambda = 0, against a
hand-worked segment and against the GAE identity; and the three training flags."""
import os
import shutil
import tempfile

import numpy as np
import pytest

from oracle import ba3c_oracle as O

REWARDS = [0.0, 1.0, -1.0, 2.0, -3.0, 0.5, 30.0]


def _segment(rs, n, vscale=3.0):
    """n transitions: rewards from REWARDS, float32 values, and a float32 bootstrap value."""
    rew = rs.choice(REWARDS, size=n).astype(np.float64)
    val = (rs.normal(size=n) * vscale).astype(np.float32)
    return rew, val


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def test_lambda_one_is_the_reference_parse_memory_bit_for_bit():
    from ba3c_amd.returns import lambda_returns_numpy, parse_memory_lambda
    rs = np.random.RandomState(0)
    for trial in range(300):
        n = int(rs.randint(1, 130))
        over = bool(rs.rand() < 0.5)
        gamma = [0.99, 1.0, 0.995][trial % 3]
        rew, val = _segment(rs, n)
        mem = [{"reward": float(rew[i]), "value": val[i], "id": i} for i in range(n)]
        init_r = 0 if over else val[-1]
        want, want_left = O.parse_memory(mem, init_r, over, gamma)
        got, got_left = parse_memory_lambda(mem, init_r, over, gamma, 1.0)
        assert [k["id"] for k, _, _, _ in got] == [k["id"] for k, _, _, _ in want]
        assert [k["id"] for k in got_left] == [k["id"] for k in want_left]
        assert len(got) == (n if over else n - 1)
        np.testing.assert_array_equal(_bits([R for _, R, _, _ in got]), _bits([R for _, R, _, _ in want]))
        assert all(i == init_r and o == over for _, _, i, o in got)
        # the time-ordered function itself: the emitted transitions, oldest first
        m = n if over else n - 1
        R = lambda_returns_numpy(rew[:m], val[:m], init_r, gamma, 1.0)
        np.testing.assert_array_equal(_bits(R[::-1]), _bits([r for _, r, _, _ in want]))


def test_lambda_zero_is_the_one_step_target_bit_for_bit():
    from ba3c_amd.returns import lambda_returns_numpy
    rs = np.random.RandomState(1)
    for trial in range(200):
        n = int(rs.randint(1, 130))
        gamma = [0.99, 1.0][trial % 2]
        rew, val = _segment(rs, n)
        boot = float(np.float32(rs.normal() * 3)) if trial % 3 else 0.0
        v_next = np.append(val[1:].astype(np.float64), boot)
        want = np.clip(rew, -1, 1) + gamma * v_next
        np.testing.assert_array_equal(_bits(lambda_returns_numpy(rew, val, boot, gamma, 0.0)), _bits(want))


def test_hand_worked_segment_at_lambda_half():
    """3 transitions, boot 4, gamma = lambda = 0.5 (every number below is exact in binary):
      R2 = -0.5     + 0.5 * (0.5 * 4    + 0.5 * 4)     = 1.5
      R1 = clip(2)  + 0.5 * (0.5 * 2    + 0.5 * 1.5)   = 1 + 0.5 * 1.75   = 1.875
      R0 = 1        + 0.5 * (0.5 * (-1) + 0.5 * 1.875) = 1 + 0.5 * 0.4375 = 1.21875
    V_next of transition t is the value of transition t + 1; the newest one's is the boot."""
    from ba3c_amd.returns import lambda_returns_numpy, parse_memory_lambda
    R = lambda_returns_numpy([1.0, 2.0, -0.5], [0.5, -1.0, 2.0], 4.0, 0.5, 0.5)
    assert R.dtype == np.float64 and R.tolist() == [1.21875, 1.875, 1.5]
    # the same segment as a memory of 4, not over: the newest (value 4) only bootstraps
    mem = [{"reward": r, "value": np.float32(v), "id": i}
           for i, (r, v) in enumerate([(1.0, 0.5), (2.0, -1.0), (-0.5, 2.0), (None, 4.0)])]
    dps, left = parse_memory_lambda(mem, mem[-1]["value"], False, 0.5, 0.5)
    assert [(k["id"], r) for k, r, _, _ in dps] == [(2, 1.5), (1, 1.875), (0, 1.21875)]
    assert [k["id"] for k in left] == [3] and all(i == 4.0 and o is False for _, _, i, o in dps)
    # over: boot 0, every transition emitted:  R2 = -0.5, R1 = 1 + 0.5 * (1 - 0.25) = 1.375,
    # R0 = 1 + 0.5 * (-0.5 + 0.6875) = 1.09375
    dps, left = parse_memory_lambda(mem[:3], 0, True, 0.5, 0.5)
    assert [(k["id"], r) for k, r, _, _ in dps] == [(2, -0.5), (1, 1.375), (0, 1.09375)] and left == []
    # the reference's gamma, in plain Python floats
    R = lambda_returns_numpy([1.0, 2.0, -0.5], [0.5, -1.0, 2.0], 4.0, 0.99, 0.5)
    r2 = -0.5 + 0.99 * (0.5 * 4.0 + 0.5 * 4.0)
    r1 = 1.0 + 0.99 * (0.5 * 2.0 + 0.5 * r2)
    r0 = 1.0 + 0.99 * (0.5 * -1.0 + 0.5 * r1)
    assert R.tolist() == [r0, r1, r2]


def test_gae_identity():
    """R^lambda_t - V_t == sum_k (gamma * lambda)^k delta_{t+k}, delta_t = clip(r_t) + gamma *
    V_{t+1} - V_t, V_n = boot; |V| <= 12, segments up to 129.  The bound 1e-9 is a condition:
    the float64 sums agree to ~1e-14 on such data and a formula slip is 1e-2 or more."""
    from ba3c_amd.returns import lambda_returns_numpy
    rs = np.random.RandomState(2)
    worst = 0.0
    for trial in range(120):
        n = [1, 2, 129][trial] if trial < 3 else int(rs.randint(1, 130))
        gamma = [0.99, 1.0, 0.9][trial % 3]
        lam = [0.0, 0.5, 0.95, 1.0, float(rs.rand())][trial % 5]
        rew = rs.choice(REWARDS, size=n).astype(np.float64)
        val = rs.uniform(-12, 12, size=n).astype(np.float32)
        boot = 0.0 if trial % 2 else float(np.float32(rs.uniform(-12, 12)))
        v = np.append(val.astype(np.float64), boot)
        delta = np.clip(rew, -1, 1) + gamma * v[1:] - v[:-1]
        adv = np.array([sum((gamma * lam) ** k * delta[t + k] for k in range(n - t)) for t in range(n)])
        got = lambda_returns_numpy(rew, val, boot, gamma, lam) - v[:-1]
        worst = max(worst, float(np.abs(got - adv).max()))
    print("GAE identity: max |R - V - sum| = %.3g" % worst)
    assert worst <= 1e-9


def _master(**kw):
    from ba3c_amd import simulator as S
    d = tempfile.mkdtemp(prefix="ba3c_ipcl_")
    m = S.SimulatorMaster("ipc://" + os.path.join(d, "c2s"), "ipc://" + os.path.join(d, "s2c"), 1, **kw)
    return m, d


@pytest.mark.parametrize("lam", [1.0, 0.95])
def test_simulator_master_parse_memory(lam):
    """gae_lambda = 1.0: the datapoints of the reference's statement (today's); 0.95: those of
    parse_memory_lambda.  BatchedSimulatorMaster hands gae_lambda through to it."""
    from ba3c_amd import simulator as S
    from ba3c_amd.returns import parse_memory_lambda
    from ba3c_amd.simulator_gpu import BatchedSimulatorMaster
    rs = np.random.RandomState(3)
    m, d = _master(local_time_max=20, gamma=0.995, gae_lambda=lam)
    try:
        assert S.SimulatorMaster.__init__.__defaults__[-1] == 1.0
        for over in (False, True):
            n = 21 if not over else 13
            rew, val = _segment(rs, n)
            mem = [{"reward": float(rew[i]), "value": val[i], "id": i} for i in range(n)]
            m.clients[b"c"].memory = [
                S.TransitionExperience(("s", i), i % 4, float(rew[i]), value=val[i], ts=i) for i in range(n)]
            m.queue = []
            init_r = 0 if over else val[-1]
            m._parse_memory(init_r, b"c", over, 99)
            if lam == 1.0:
                want, left = O.parse_memory(mem, init_r, over, 0.995)
            else:
                want, left = parse_memory_lambda(mem, init_r, over, 0.995, lam)
            assert [(dp[0], dp[1], dp[3], dp[4], dp[5]) for dp in m.queue] == \
                [(("s", k["id"]), k["id"] % 4, k["id"], init_r, over) for k, _, _, _ in want]
            np.testing.assert_array_equal(_bits([dp[2] for dp in m.queue]), _bits([R for _, R, _, _ in want]))
            assert [k.ts for k in m.clients[b"c"].memory] == [k["id"] for k in left]
    finally:
        m.close()
        shutil.rmtree(d, ignore_errors=True)
    d = tempfile.mkdtemp(prefix="ba3c_ipcl_")
    b = BatchedSimulatorMaster("ipc://" + os.path.join(d, "c2s"), "ipc://" + os.path.join(d, "s2c"), 1,
                               batch_policy=lambda s: None, gae_lambda=lam, local_time_max=20)
    try:
        assert b.gae_lambda == lam and b.local_time_max == 20
    finally:
        b.close()
        shutil.rmtree(d, ignore_errors=True)


def test_flags():
    from ba3c_amd import flags as F
    parse = lambda argv: F.resolve(F.build_parser().parse_args(argv))
    d = parse([])
    assert (d.gae_lambda, d.local_time_max, d.gamma) == (1.0, 5, 0.99)
    a = parse(["--gae_lambda", "0.95", "--local_time_max", "20", "--gamma", "0.995"])
    assert (a.gae_lambda, a.local_time_max, a.gamma) == (0.95, 20, 0.995)
    a = parse("-e GridBoxing-v0 --num_actions 18 --self_play --gae_lambda 0 --local_time_max 128 "
              "--gamma 1".split())
    assert (a.gae_lambda, a.local_time_max, a.gamma) == (0.0, 128, 1.0) and a.self_play
    a = parse("-e GridBreakout-v0 --frame_skip 2-4 --gae_lambda 0.9 --local_time_max 1".split())
    assert (a.gae_lambda, a.local_time_max) == (0.9, 1)
    for argv, word in [("--gae_lambda -0.1", "lambda"), ("--gae_lambda 1.5", "lambda"),
                       ("--gae_lambda nan", "lambda"), ("--local_time_max 0", "local_time_max"),
                       ("--local_time_max 129", "local_time_max"), ("--gamma 0", "gamma"),
                       ("--gamma 1.01", "gamma"), ("--gamma nan", "gamma"),
                       # 5000 x 129 states of 28224 bytes = 17.0 GiB
                       ("--simulator_procs 5000 --local_time_max 128", "GiB")]:
        with pytest.raises(SystemExit) as e:
            parse(argv.split())
        msg = str(e.value)
        assert word in msg and "\n" not in msg, (argv, msg)
    # 4000 x 129 states = 13.6 GiB passes
    assert parse("--simulator_procs 4000 --local_time_max 128".split()).simulator_procs == 4000


def test_lambda_entry_point_rejects_bad_arguments_without_gpu():
    """Null pointers, a bad shape, lambda outside [0, 1], gamma outside (0, 1] and NaN are
    BA3C_ERR_INVALID before any GPU call."""
    import ctypes
    from ba3c_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    D = ctypes.c_double

    def call(n_envs=1, slots=6, gamma=0.99, lam=0.95, first=p):
        return lib.ba3c_lambda_returns(None, first, p, p, p, p, n_envs, slots, D(gamma), D(lam), p, p, p, p, p)
    assert call(first=None) == 1 and b"pointer" in lib.ba3c_last_error()
    for kw in (dict(n_envs=-1), dict(slots=0), dict(slots=130)):
        assert call(**kw) == 1 and b"shape" in lib.ba3c_last_error(), kw
    for lam in (-0.1, 1.5, float("nan")):
        assert call(lam=lam) == 1 and b"lambda" in lib.ba3c_last_error(), lam
    for gamma in (0.0, -1.0, 1.5, float("nan")):
        assert call(gamma=gamma) == 1 and b"gamma" in lib.ba3c_last_error(), gamma
    assert lib.ba3c_gather_rows(None, p, p, -1, 16, p) == 1
