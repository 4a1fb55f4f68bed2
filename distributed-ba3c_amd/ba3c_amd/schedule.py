"""Schedules of the learner's run-time hyper-parameters (the learning rate and the entropy
coefficient), as pure functions of the 0-based `global_step` before the step, in Python float64.

    const                   the start value at every step (the default)
    linear:END              start + (END - start) * min(step / max_steps, 1)
    steps:E1=V1,E2=V2,...   the reference's HyperParameterScheduler(name, [(E1, V1), (E2, V2), ...])
                            (OpenAIGym/train.py:633-634): the start value, then Vk from
                            global_step >= Ek * steps_per_epoch on; Ek integers, strictly
                            increasing and >= 1

A schedule is a function of global_step alone, which the checkpoint restores, so a resumed run
continues it and every rank computes the same value.  Ba3cTrainer.schedules applies them; the
values' ranges (a learning rate > 0, a coefficient >= 0) are the flags' to check (flags.resolve).
"""
import math


class Schedule(object):
    """fn(global_step) -> float.  kind: 'const' / 'linear' / 'steps'; constant: the value never
    changes (a captured graph may freeze it); values: every value the spec names."""

    def __init__(self, kind, start, fn, values=()):
        self.kind, self.start, self._fn, self.values = kind, float(start), fn, tuple(values)

    @property
    def constant(self):
        return self.kind == "const"

    def __call__(self, global_step):
        if global_step < 0:
            raise ValueError("global_step %r: must be >= 0" % (global_step,))
        return self._fn(int(global_step))


def _number(text, spec):
    try:
        v = float(text)
    except ValueError:
        raise ValueError("schedule %r: %r is not a number" % (spec, text))
    if not math.isfinite(v):
        raise ValueError("schedule %r: %r is not finite" % (spec, text))
    return v


def parse(spec, start, max_steps=None, steps_per_epoch=None):
    """spec (None: 'const') -> Schedule from `start`.  linear needs max_steps >= 1, steps needs
    steps_per_epoch >= 1.  ValueError on anything malformed."""
    start = float(start)
    if not math.isfinite(start):
        raise ValueError("schedule start %r is not finite" % start)
    spec = "const" if spec is None else str(spec).strip()
    if spec == "const":
        return Schedule("const", start, lambda step: start)
    form, sep, rest = spec.partition(":")
    if form == "linear" and sep:
        end = _number(rest, spec)
        if max_steps is None or int(max_steps) < 1:
            raise ValueError("schedule %r: linear needs the run's max_steps >= 1" % spec)
        n = int(max_steps)
        return Schedule("linear", start, lambda step: start + (end - start) * min(step / n, 1.0),
                        values=(end,))
    if form == "steps" and sep:
        if steps_per_epoch is None or int(steps_per_epoch) < 1:
            raise ValueError("schedule %r: steps needs steps_per_epoch >= 1" % spec)
        spe = int(steps_per_epoch)
        table = []
        for item in rest.split(","):
            e, eq, v = item.partition("=")
            if not eq:
                raise ValueError("schedule %r: expected EPOCH=VALUE, got %r" % (spec, item))
            try:
                epoch = int(e)
            except ValueError:
                raise ValueError("schedule %r: epoch %r is not an integer" % (spec, e))
            if epoch < 1:
                raise ValueError("schedule %r: epoch %d must be >= 1" % (spec, epoch))
            if table and epoch <= table[-1][0]:
                raise ValueError("schedule %r: epochs must be strictly increasing (%d after %d)"
                                 % (spec, epoch, table[-1][0]))
            table.append((epoch, _number(v, spec)))

        def fn(step):
            value = start
            for epoch, v in table:
                if step >= epoch * spe:
                    value = v
            return value
        return Schedule("steps", start, fn, values=[v for _, v in table])
    raise ValueError("schedule %r: expected const, linear:END or steps:E1=V1,E2=V2,..." % spec)
