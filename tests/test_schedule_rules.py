"""The learning-rate / entropy-coefficient schedules (ba3c_amd/schedule.py), their flags
(flags.resolve), the `schedule` message of the metrics sink and the trainer's hook.  No GPU."""
import os

import pytest

from ba3c_amd import schedule as S
from ba3c_amd.flags import build_parser, resolve


# --- the forms at their boundaries ---------------------------------------------------------------
def test_const_is_the_default_and_never_moves():
    for spec in (None, "const", " const "):
        fn = S.parse(spec, 1.5e-4)
        assert fn.constant and fn.kind == "const" and fn.values == ()
        assert [fn(s) for s in (0, 1, 10 ** 9)] == [1.5e-4] * 3


def test_linear_at_its_boundaries():
    start, end, n = 2.5e-4, 0.0, 1000
    fn = S.parse("linear:0", start, max_steps=n)
    assert not fn.constant and fn.values == (0.0,)
    assert fn(0) == start
    assert fn(1) == start + (end - start) * (1 / n)
    assert fn(n - 1) == start + (end - start) * ((n - 1) / n) and fn(n - 1) > 0.0
    assert fn(n) == 0.0 and fn(n + 1) == 0.0 and fn(10 * n) == 0.0
    up = S.parse("linear:1e-3", 1e-4, max_steps=4)                 # a schedule may rise
    assert [up(s) for s in range(6)] == [1e-4 + (1e-3 - 1e-4) * min(s / 4, 1.0) for s in range(6)]
    assert up(4) == 1e-3 and up(5) == 1e-3


def test_steps_at_its_boundaries():
    spe = 250
    fn = S.parse("steps:20=0.0005,60=0.0001", 1e-3, steps_per_epoch=spe)      # the reference's
    assert not fn.constant and fn.values == (0.0005, 0.0001)
    assert fn(0) == 1e-3 and fn(20 * spe - 1) == 1e-3
    assert fn(20 * spe) == 0.0005 and fn(60 * spe - 1) == 0.0005
    assert fn(60 * spe) == 0.0001 and fn(10 ** 9) == 0.0001
    one = S.parse("steps:1=5e-4", 1e-3, steps_per_epoch=1)
    assert [one(s) for s in range(3)] == [1e-3, 5e-4, 5e-4]


def test_a_schedule_is_a_function_of_the_step_alone():
    fn = S.parse("linear:0", 1e-3, max_steps=7)
    assert [fn(s) for s in (5, 2, 5)] == [fn(5), fn(2), fn(5)]     # a resumed run continues it
    with pytest.raises(ValueError):
        fn(-1)


@pytest.mark.parametrize("spec,kw", [
    ("", {}), ("linear", {"max_steps": 5}), ("linear:", {"max_steps": 5}), ("linear:x", {"max_steps": 5}),
    ("linear:nan", {"max_steps": 5}), ("linear:inf", {"max_steps": 5}), ("linear:0", {}),
    ("linear:0", {"max_steps": 0}), ("steps", {"steps_per_epoch": 5}), ("steps:", {"steps_per_epoch": 5}),
    ("steps:1", {"steps_per_epoch": 5}), ("steps:1=", {"steps_per_epoch": 5}),
    ("steps:0=1e-3", {"steps_per_epoch": 5}), ("steps:-1=1e-3", {"steps_per_epoch": 5}),
    ("steps:1.5=1e-3", {"steps_per_epoch": 5}), ("steps:2=1e-3,2=1e-4", {"steps_per_epoch": 5}),
    ("steps:3=1e-3,2=1e-4", {"steps_per_epoch": 5}), ("steps:1=nan", {"steps_per_epoch": 5}),
    ("steps:1=1e-3,", {"steps_per_epoch": 5}), ("steps:1=1e-3", {}), ("steps:1=1e-3", {"steps_per_epoch": 0}),
    ("cosine:0", {"max_steps": 5}), ("linear:0:1", {"max_steps": 5}),
])
def test_malformed_specs(spec, kw):
    with pytest.raises(ValueError):
        S.parse(spec, 1e-3, **kw)


def test_a_start_that_is_not_finite():
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            S.parse("const", bad)


# --- the flags -------------------------------------------------------------------------------------
def _resolve(*argv):
    return resolve(build_parser().parse_args(list(argv)))


def test_the_flags_default_to_off():
    a = _resolve()
    assert a.max_grad_norm is None and a.entropy_beta == 0.01
    assert a.schedules is None and a.log_schedule is False
    assert _resolve("--max_grad_norm", "0").max_grad_norm is None
    assert _resolve("--schedule_hyper").schedules is None          # accepted and ignored


def test_the_flags_reach_the_schedules():
    a = _resolve("--max_grad_norm", "0.5", "--lr", "1e-3", "--lr_schedule", "linear:0", "--entropy_beta",
                 "0.02", "--entropy_schedule", "steps:1=0.005", "--max_steps", "6", "--steps_per_epoch", "3")
    assert a.max_grad_norm == 0.5 and a.entropy_beta == 0.02 and a.log_schedule
    lr, beta = a.schedules["learning_rate"], a.schedules["entropy_beta"]
    assert [lr(s) for s in (0, 3, 6, 7)] == [1e-3, 1e-3 + (0.0 - 1e-3) * 0.5, 0.0, 0.0]
    assert [beta(s) for s in (0, 2, 3, 6)] == [0.02, 0.02, 0.005, 0.005]
    # linear's length without --max_steps: --steps_per_epoch x --max_epoch, as the launcher runs
    b = _resolve("--lr_schedule", "linear:0", "--steps_per_epoch", "10", "--max_epoch", "4")
    assert b.schedules["learning_rate"](40) == 0.0 and b.schedules["learning_rate"](39) > 0.0
    assert b.schedules["entropy_beta"].constant and b.schedules["entropy_beta"](5) == 0.01
    # --entropy_beta alone: no schedule to run, but the channels are written
    c = _resolve("--entropy_beta", "0")
    assert c.schedules is None and c.log_schedule and c.entropy_beta == 0.0
    d = _resolve("--lr_schedule", "steps:20=0.0005,60=0.0001", "--entropy_schedule", "steps:40=0.005,80=0.001")
    assert d.schedules["learning_rate"](20 * 250) == 0.0005 and d.schedules["entropy_beta"](80 * 250) == 0.001


@pytest.mark.parametrize("argv", [
    ["--max_grad_norm", "-0.5"], ["--max_grad_norm", "nan"], ["--max_grad_norm", "inf"],
    ["--entropy_beta", "-0.01"], ["--entropy_beta", "nan"], ["--entropy_beta", "inf"],
    ["--lr_schedule", "linear:-1e-4"], ["--lr_schedule", "linear:nan"], ["--lr_schedule", "steps:1=0"],
    ["--lr_schedule", "steps:1=-1e-4"], ["--lr_schedule", "steps:2=1e-4,1=1e-5"],
    ["--lr_schedule", "steps:0=1e-4"], ["--lr_schedule", "bogus"], ["--lr_schedule", "linear:0", "--lr", "0"],
    ["--lr_schedule", "linear:0", "--max_epoch", "0"],
    ["--entropy_schedule", "linear:-0.001"], ["--entropy_schedule", "steps:1=-0.001"],
    ["--entropy_schedule", "steps:1=inf"], ["--entropy_schedule", "linear:0", "--steps_per_epoch", "0"],
])
def test_resolve_refuses(argv):
    with pytest.raises(SystemExit):
        _resolve(*argv)


def test_zero_is_a_fine_entropy_coefficient_and_a_fine_end_of_a_linear_lr():
    a = _resolve("--entropy_schedule", "steps:1=0", "--lr_schedule", "linear:0", "--max_steps", "4")
    assert a.schedules["entropy_beta"](250) == 0.0 and a.schedules["learning_rate"](4) == 0.0


# --- the metrics sink ------------------------------------------------------------------------------
def test_csv_channels_writes_the_two_files_for_a_schedule_message(tmp_path):
    from ba3c_amd.metrics import CsvChannels, ScheduleMetrics
    c = CsvChannels(str(tmp_path))
    c.send((0, ("schedule", 1e-4, 0.01)))
    c.send((0, ("schedule", 5e-5, 0.005)))
    c.close()
    assert sorted(os.listdir(str(tmp_path))) == ["entropy_beta.csv", "learning_rate.csv"]
    for name, want in (("learning_rate", [1e-4, 5e-5]), ("entropy_beta", [0.01, 0.005])):
        rows = open(os.path.join(str(tmp_path), name + ".csv")).read().split()
        assert rows[0] == "x,y" and [float(r.split(",")[1]) for r in rows[1:]] == want

    class T(object):
        pass
    sent = []
    m = ScheduleMetrics(type("C", (), {"send": lambda self, msg: sent.append(msg)})())
    t = T()
    t.optimizer, t.model = T(), T()
    for lr, beta in ((1e-3, 0.02), (5e-4, 0.01)):
        t.optimizer.learning_rate, t.model.entropy_beta = lr, beta
        m.on_step(t)
    m.flush()
    m.flush()                                                      # nothing pending: nothing sent
    assert sent == [(0, ("schedule", (1e-3 + 5e-4) / 2, (0.02 + 0.01) / 2))]
    assert m.last == {"learning_rate": 5e-4, "entropy_beta": 0.01}


# --- the trainer's hook ------------------------------------------------------------------------------
class Recording(object):
    """An object that notes every attribute written after its construction."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.__dict__["written"] = []

    def __setattr__(self, k, v):
        self.written.append((k, v))
        self.__dict__[k] = v


def _trainer():
    from ba3c_amd.model_desc import ClipByGlobalNorm
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    calls = []
    engine = Recording(clip_grads_global=lambda m: calls.append(("clip", m)))
    model = Recording(engine=engine, entropy_beta=0.01, ppo=None,
                      get_gradient_processor=lambda: [ClipByGlobalNorm(0.5)],
                      build_graph=lambda inputs: calls.append(("grads", model.entropy_beta)))
    opt = Recording(learning_rate=1e-3,
                    apply_gradients=lambda eng, **kw: calls.append(("apply", opt.learning_rate, kw)))
    return Ba3cTrainer(TrainConfig(model=model, optimizer=opt)), model, opt, calls


def test_a_trainer_without_schedules_never_touches_the_two_values():
    tr, model, opt, calls = _trainer()
    assert tr.schedules is None and not tr._fused_clip
    for _ in range(3):
        tr.train_step(None, None, None)
    assert tr.global_step == 3 and model.written == [] and opt.written == []
    # the global clip goes the generic way: process_grads, then the unfused apply
    assert calls[:3] == [("grads", 0.01), ("clip", 0.5), ("apply", 1e-3, {})]


def test_a_trainer_writes_both_values_before_the_steps_first_launch():
    tr, model, opt, calls = _trainer()
    tr.schedules = {"learning_rate": S.parse("steps:1=5e-4", 1e-3, steps_per_epoch=2),
                    "entropy_beta": S.parse("linear:0", 0.02, max_steps=4)}
    for _ in range(3):
        tr.train_step(None, None, None)
    assert [c for c in calls if c[0] == "grads"] == [("grads", 0.02), ("grads", 0.015), ("grads", 0.01)]
    assert [c[1] for c in calls if c[0] == "apply"] == [1e-3, 1e-3, 5e-4]
    assert opt.written == [("learning_rate", v) for v in (1e-3, 1e-3, 5e-4)]
    tr.global_step = 100                                           # as a checkpoint restores it
    tr.train_step(None, None, None)
    assert opt.learning_rate == 5e-4 and model.entropy_beta == 0.0
    # one schedule alone leaves the other value alone
    tr2, model2, opt2, _ = _trainer()
    tr2.schedules = {"entropy_beta": S.parse("steps:1=0.005", 0.02, steps_per_epoch=1)}
    tr2.train_step(None, None, None)
    tr2.train_step(None, None, None)
    assert opt2.written == [] and model2.written == [("entropy_beta", 0.02), ("entropy_beta", 0.005)]


def test_capture_refuses_a_schedule_that_moves():
    tr, _, _, _ = _trainer()
    tr.schedules = {"learning_rate": S.parse("linear:0", 1e-3, max_steps=4)}
    with pytest.raises(ValueError, match="schedule"):
        tr.capture_step(None, None, None)
