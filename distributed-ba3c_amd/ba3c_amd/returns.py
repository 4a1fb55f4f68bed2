"""lambda-returns on the host: the one statement that `ba3c_lambda_returns` (the GPU kernel),
`RolloutBuffer` and `SimulatorMaster._parse_memory` compute, and their oracle.

    R_t = clip(r_t, -1, 1) + gamma * ((1 - lambda) * V_{t+1} + lambda * R_{t+1})
    R_n = V_n = the bootstrap: the newest transition's value, or 0 when the episode ended

The learner's loss forms `advantage = futurereward - stop_gradient(value)` and fits `value` to
`futurereward` (model.py); fed R_t, the policy advantage is the GAE(lambda) advantage
R_t - V_t = sum_k (gamma * lambda)^k delta_{t+k}, delta_t = clip(r_t) + gamma * V_{t+1} - V_t,
and the value target is the TD(lambda) target.  lambda = 1 is the reference's `_parse_memory`
(OpenAIGym/train.py:418-437) exactly: `0 * V + 1 * R == R` in floating point; lambda = 0 is
`clip(r_t) + gamma * V_{t+1}`.  All arithmetic is float64, one rounding per operation.
"""
import numpy as np

GAMMA = 0.99              # train.py:94


def lambda_step(reward, v_next, R, gamma, lam):
    """One step backwards in time; `v_next` and `R` are float64 (Python float / np.float64)."""
    return np.clip(reward, -1, 1) + gamma * ((1 - lam) * v_next + lam * R)


def lambda_returns_numpy(rewards, values, boot, gamma, lam):
    """R_t for a segment in time order: rewards[t] and values[t] = V_t of transition t, boot =
    V_n.  Returns float64 [n]."""
    r = np.asarray(rewards, dtype=np.float64)
    v = np.asarray(values, dtype=np.float64)
    assert r.shape == v.shape and r.ndim == 1
    out = np.empty(len(r), dtype=np.float64)
    R = v_next = float(boot)
    for t in range(len(r) - 1, -1, -1):
        R = lambda_step(r[t], v_next, R, gamma, lam)
        out[t] = R
        v_next = float(v[t])
    return out


def parse_memory_lambda(memory, init_r, is_over, gamma=GAMMA, lam=1.0):
    """`_parse_memory` (train.py:418-437) with lambda-returns.  memory: transitions in time
    order, dicts with 'reward' and 'value'.  Not over: the newest transition only bootstraps
    (init_r = its value) and stays in memory; over: init_r = 0 and every transition is emitted.
    Returns the datapoints in queue order (newest first) as (transition, R, init_r, is_over)
    and the memory left behind."""
    mem = list(memory)
    last = None
    if not is_over:
        last = mem[-1]
        mem = mem[:-1]
    R = lambda_returns_numpy([k["reward"] for k in mem], [k["value"] for k in mem], init_r,
                             gamma, lam)
    out = [(mem[t], R[t], init_r, is_over) for t in range(len(mem) - 1, -1, -1)]
    return out, ([last] if not is_over else [])


class LambdaMasterMirror(object):
    """The per-client memory logic of SimulatorMaster.run with MySimulatorMaster's callbacks
    (RL/simulator.py:160-185, train.py:364-437) over parse_memory_lambda: parse with
    init_r = 0 at an episode end, or from the newest value once local_time_max + 1 transitions
    are in memory."""

    def __init__(self, local_time_max=5, gamma=GAMMA, lam=1.0):
        self.T = local_time_max + 1
        self.gamma, self.lam = gamma, lam
        self.memory = {}
        self.queue = []          # datapoints in put order

    def on_message(self, ident, reward, is_over):
        mem = self.memory.setdefault(ident, [])
        if len(mem) > 0:
            mem[-1]["reward"] = reward
            if is_over:
                dps, self.memory[ident] = parse_memory_lambda(mem, 0, True, self.gamma, self.lam)
                self.queue.extend(dps)
            elif len(mem) == self.T:
                dps, self.memory[ident] = parse_memory_lambda(mem, mem[-1]["value"], False,
                                                              self.gamma, self.lam)
                self.queue.extend(dps)

    def on_state(self, ident, state_id, action, value):
        self.memory.setdefault(ident, []).append(
            {"state": state_id, "action": action, "value": value, "reward": None})
