"""Host-side pieces of the learner loop that need no GPU: the KL stop's two estimators agree, and
the step metrics write their channels from a stub trainer and a stub PPO consumer."""
import types

import numpy as np
import pytest
import torch

from ba3c_amd import ppo
from ba3c_amd._lib import SCALAR_NAMES
from ba3c_amd.metrics import CsvChannels, PpoMetrics, StepMetrics


@pytest.mark.parametrize("s", [1e-4, 1e-2, 0.3, 1.0])
@pytest.mark.parametrize("B", [1, 8, 1024])
def test_the_device_form_of_the_stop_estimator_agrees_with_the_host_form(B, s):
    """Both are float64 means of the same <= 1024 non-negative terms, summed in different orders:
    at most 1024 * 2^-53 ~ 1.1e-13 apart relatively; the bound is ten times that."""
    rho = np.exp(np.random.RandomState(B).normal(0.0, s, size=B)).astype(np.float32)
    host, dev = ppo.stop_kl(rho), ppo.stop_kl_device(torch.from_numpy(rho))
    assert dev.dtype == torch.float64 and dev.dim() == 0
    err = abs(float(dev) - host) / host
    print("B %d s %g: host %.17g relative difference %.2e" % (B, s, host, err))
    assert err <= 1e-12


PER_STEP = ["ppo_clip_fraction", "ppo_approx_kl", "ppo_adv_mean", "ppo_adv_std"]


def _rows(tmp_path, name):
    path = tmp_path / (name + ".csv")
    if not path.exists():
        return None
    lines = path.read_text().strip().splitlines()
    assert lines[0] == "x,y"
    return [float(line.split(",")[1]) for line in lines[1:]]


def _metrics(tmp_path, target_kl, every=2):
    model = types.SimpleNamespace(scalars=torch.arange(8, dtype=torch.float32),
                                  ratio=torch.tensor([1.0, 1.5, 0.5, 1.1]))
    trainer = types.SimpleNamespace(model=model, check_device_errors=lambda: None)
    consumer = types.SimpleNamespace(last_adv_stats=torch.tensor([0.5, 2.0], dtype=torch.float64),
                                     pool_epochs=[], setting=ppo.Setting(0.2, 3, 2, True, 0.0, target_kl))
    client = CsvChannels(str(tmp_path))
    return StepMetrics(trainer, 8, every, client, ppo=PpoMetrics(0.2, consumer, client)), trainer, consumer


def test_step_metrics_write_the_ppo_channels_per_flush_and_epochs_run_per_pool_left(tmp_path):
    metrics, trainer, consumer = _metrics(tmp_path, target_kl=0.02)
    for step in range(5):                       # flushes after steps 2 and 4
        metrics(trainer)
        if step == 2:
            consumer.pool_epochs.append(3.0)    # a pool left between the two flushes
    assert metrics.last_ppo["ppo_epochs_run"] == 3.0
    metrics.flush()                             # one step pending, no pool left since
    assert [len(_rows(tmp_path, n)) for n in PER_STEP] == [3] * 4 and _rows(tmp_path, "ppo_epochs_run") == [3.0]
    consumer.pool_epochs += [1.0, 2.0]
    metrics.flush()                             # nothing pending, two pools left
    assert [len(_rows(tmp_path, n)) for n in PER_STEP] == [3] * 4
    assert _rows(tmp_path, "ppo_epochs_run") == [3.0, 1.5]
    assert _rows(tmp_path, "ppo_clip_fraction") == [0.5] * 3
    assert _rows(tmp_path, "ppo_adv_mean") == [0.5] * 3 and _rows(tmp_path, "ppo_adv_std") == [2.0] * 3
    assert list(metrics.last_ppo) == PER_STEP + ["ppo_epochs_run"] and metrics.last_ppo["ppo_epochs_run"] == 1.5
    assert metrics.last_ppo["ppo_approx_kl"] == ppo.approx_kl(trainer.model.ratio.numpy())
    assert metrics.last == dict(zip(SCALAR_NAMES, range(8)))


def test_step_metrics_write_no_epochs_run_without_a_target_kl(tmp_path):
    metrics, trainer, consumer = _metrics(tmp_path, target_kl=0.0)
    for step in range(4):
        metrics(trainer)
        consumer.pool_epochs.append(3.0)
    metrics.flush()
    assert [len(_rows(tmp_path, n)) for n in PER_STEP] == [2] * 4
    assert _rows(tmp_path, "ppo_epochs_run") is None and list(metrics.last_ppo) == PER_STEP
