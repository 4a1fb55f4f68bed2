"""The actor-learner loop with the PPO consumer: the pool is fed the datapoints the reference's
master would have queued, with the value and log-probability recorded at the draw, and the loop
makes its calls and its host reads in the stated order and number."""
import numpy as np
import pytest
import torch

from ba3c_amd import ppo
from loop_mirror import LoopMirror
from oracle import ba3c_oracle as O

pytestmark = pytest.mark.gpu

E, LB, M, K, A, ITERS = 24, 8, 2, 3, 18, 12          # test_gpu_ppo_ext._loop's
ITERATION = ["forward", "sample_logp", "step_into"]
LEARNER_STEP = ["ppo_norm_adv", "train_grads_ppo", "on_train_step"]


def _loop(setting, on_train_step=None):
    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.boxing import BoxingVec
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    m = Model(num_actions=A, fc_neurons=128, fc_splits=4, batch_size=LB, max_batch=max(LB, E))
    m.engine.load_params(O.init_params(128, 4, A, seed=0, dtype=np.float32))
    tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
    return ActorLearner(tr, n_envs=E, batch_size=LB, seed=1, env=BoxingVec(E, seed=1, limit=25),
                        ppo=setting, on_train_step=on_train_step)


def record_calls(log, setattr, engine_methods=("forward", "sample_logp", "ppo_norm_adv", "train_grads_ppo")):
    """Wraps the named Ba3cEngine methods and GameVec.step_into (through `setattr`, a
    monkeypatch's) so that each call appends its name to `log`."""
    from ba3c_amd.engine import Ba3cEngine
    from ba3c_amd.gamevec import GameVec

    def wrap(cls, name):
        orig = getattr(cls, name)

        def recorded(self, *a, **kw):
            log.append(name)
            return orig(self, *a, **kw)
        setattr(cls, name, recorded)
    for name in engine_methods:
        wrap(Ba3cEngine, name)
    wrap(GameVec, "step_into")


def test_pool_receives_the_reference_datapoints_with_the_draws_value_and_logp():
    loop = _loop(ppo.Setting(0.2, K, M))
    taps = LoopMirror(loop, O.SimulatorMasterMirror())
    loop.run(ITERS)
    torch.cuda.synchronize()
    assert loop.train_steps >= K * M
    assert taps.consumed == taps.queued()
    rows = np.concatenate(taps.rows)
    assert rows.shape == (len(taps.consumed), 4) and rows.dtype == np.float32
    for row, (action, R), (k, _, _, _) in zip(rows, taps.consumed, taps.mirror.queue):
        t, e = k["state"]                                   # the draw this datapoint came from
        actions, values, logp = taps.drawn[t]
        assert action == actions[e] and row[0] == np.float32(R)
        assert row[1] == values[e] and row[2] == logp[e] and row[3] == 0


def test_loop_makes_its_calls_and_host_reads_in_order(monkeypatch):
    log = []
    record_calls(log, monkeypatch.setattr)
    loop = _loop(ppo.Setting(0.2, K, M, norm_adv=True, vclip=0.2, target_kl=1e9),
                 on_train_step=lambda tr: log.append("on_train_step"))
    reads, item = [], torch.Tensor.item

    def counted(self):
        reads.append(1)
        return item(self)
    monkeypatch.setattr(torch.Tensor, "item", counted)
    loop.run(ITERS)
    monkeypatch.undo()
    torch.cuda.synchronize()

    starts = [i for i, name in enumerate(log) if name == "forward"]
    assert len(starts) == ITERS and starts[0] == 0
    steps = 0
    for a, b in zip(starts, starts[1:] + [len(log)]):
        assert log[a:a + 3] == ITERATION
        learner = log[a + 3:b]
        assert learner == LEARNER_STEP * (len(learner) // 3)
        steps += len(learner) // 3
    pt = loop.pool_trainer
    pools = len(pt.pool_epochs)
    assert pools * K * M == steps == loop.train_steps > 0
    epochs = len(pt.epoch_kls)                              # one read per completed epoch
    assert epochs == pools * K
    assert len(reads) == ITERS * 2 + epochs                 # on_reward's count and the sampling flag
