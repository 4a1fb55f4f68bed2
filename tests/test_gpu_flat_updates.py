"""The clip and optimizer kernels (sumsq / clip / clip_range / update<0..5> / clip_update<0..5>,
csrc/ba3c_small.h) and their dispatch, on crafted gradients written straight into the flat
buffers (tests/flat_updates.py): every launch form bit-identical to the others, each within
4 x the case's yardstick of the float64 oracle, and the 64-float alignment gaps untouched.

The yardstick of a case is the float32 oracle's own distance to the float64 one on the same
inputs, per measure, the worst over the case's tensors and steps, floored at 2^-24.  The factor
4: beyond the float32 oracle's roundings the kernels have v_rsq_f32 for 1/sqrt, a chunked
float32 sum of squares for a float64 one, g*lr*rsqrt(acc) associations and sqrt*rsqrt*g in
Adadelta: two or three more roundings.  Measured figures: DESIGN.md, "Flat clip and update
kernels against float64".
"""
import functools

import numpy as np
import pytest
import torch

import flat_updates as U

pytestmark = pytest.mark.gpu

GEOMS = sorted(U.GEOMETRIES)
GRAD_GAP, PARAM_GAP, SLOT_GAP = 1e30, 12345.0, -54321.0

_ENGINES = {}


def engines(geom, monkeypatch):
    """(default handle, BA3C_FUSED_UPDATE=0 handle) of a geometry; the switch is read at create."""
    if geom not in _ENGINES:
        from ba3c_amd.engine import Ba3cEngine
        g = U.GEOMETRIES[geom]
        made = []
        for env in (None, "0"):
            if env is None:
                monkeypatch.delenv("BA3C_FUSED_UPDATE", raising=False)
            else:
                monkeypatch.setenv("BA3C_FUSED_UPDATE", env)
            made.append(Ba3cEngine(num_actions=g["A"], channels=g["C"], fc_neurons=g["F"],
                                   fc_splits=g["S"], replace_with_conv=not g["legacy"], ps=g["ps"],
                                   max_batch=1))
        monkeypatch.delenv("BA3C_FUSED_UPDATE", raising=False)
        assert [(n, k) for n, _, k, _ in made[0].layout] == U.tensors(geom)
        assert made[0].layout == made[1].layout
        for _, off, _, _ in made[0].layout:
            assert off % 64 == 0
        _ENGINES[geom] = tuple(made)
    return _ENGINES[geom]


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def dealt(geom, step):
    """(raw gradients, clip64, clip32) per tensor: computed once, read by every case."""
    g = U.dealt_gradients(geom, step)
    out = (g, [U.clip64(x) for x in g], [U.clip32(x) for x in g])
    for part in out:
        for x in part:
            x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def start_params(geom):
    p = U.initial_params(geom)
    for x in p:
        x.setflags(write=False)
    return p


def up(eng, flat):
    return torch.from_numpy(flat).to(eng.device)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def digest(problems):
    """{kind of problem: (how many, the first three)}: an assertion message that shows every
    kind, however many of the first there are."""
    out = {}
    for q in problems:
        n, first = out.get(q[0], (0, []))
        out[q[0]] = (n + 1, first + [q[1:]] if n < 3 else first)
    return out


def report(tag, worst, yard):
    print("flat-update", tag, " ".join("%s gpu=%.2e yardstick=%.2e" % (m, worst[m], yard[m])
                                       for m in sorted(worst)))


# --- a. clip, all forms ----------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_clip_forms_agree_and_match_float64(geom, monkeypatch):
    handles = engines(geom, monkeypatch)
    eng = handles[0]
    layout, size = eng.layout, eng.flat_size
    gaps = U.gap_mask(layout, size)
    assert gaps.any()
    tb, _ = eng.bucket_split()
    nt = len(layout)
    problems = []
    for step in range(U.NSTEPS):           # the same handles throughout: the tags advance
        g, c64, c32 = dealt(geom, step)
        flat = U.pack(layout, size, g, GRAD_GAP)
        got = {}
        for hi, h in enumerate(handles):
            for form in ("whole", "ranges"):
                h.grads.copy_(up(h, flat))
                if form == "whole":
                    h.clip_grads()
                else:
                    h.clip_grads_range(tb, nt)
                    h.clip_grads_range(0, tb)
                got[(hi, form)] = h.grads.cpu().numpy()
        first = got[(0, "whole")]
        for key, v in got.items():
            if not np.array_equal(bits(v), bits(first)):
                problems.append(("not bit-identical to the two-launch clip", step, key,
                                 int((bits(v) != bits(first)).sum())))
            if not np.array_equal(bits(v[gaps]), bits(flat[gaps])):
                problems.append(("alignment gap written", step, key))
        yard = U.floor(max(U.norm_err(a, b) for a, b in zip(c32, c64)))
        assert yard < U.YARDSTICK_CAP
        errs = [U.norm_err(a, b) for a, b in zip(U.unpack(layout, first), c64)]
        report("clip %s step %d" % (geom, step), {"clip": max(errs)}, {"clip": yard})
        for (name, _, _, _), e in zip(layout, errs):
            if not e <= U.GPU_FACTOR * yard:
                problems.append(("clip outside the bound", step, name, e, yard))
    for h in handles:
        assert h.device_errors() == 0
    assert not problems, digest(problems)


# --- b. update, all forms ----------------------------------------------------------------------------
class State(object):
    """Host copies of one form's flat params and slots."""

    def __init__(self, eng, geom, opt):
        lay, size = eng.layout, eng.flat_size
        self.p = U.pack(lay, size, start_params(geom), PARAM_GAP)
        sl = [U.initial_slots(opt, n) for _, _, n, _ in lay]
        self.s = [U.pack(lay, size, [x[i] for x in sl], SLOT_GAP) if sl[0][i] is not None else None
                  for i in (0, 1)]

    def flats(self):
        return [self.p] + [s for s in self.s if s is not None]

    def tensor(self, layout, i):
        off, n = layout[i][1], layout[i][2]
        return tuple(None if f is None else f[off:off + n] for f in [self.p] + self.s)


def run_form(eng, st, opt, hp, gflat, step, fuse_clip, pre_clip=False, grad_scale=1.0, dev_powers=None):
    """One apply of a form from the host state `st` -> the new State, with the gradient buffer
    as the launches left it in `.g`."""
    eng.params.copy_(up(eng, st.p))
    eng.grads.copy_(up(eng, gflat))
    slots = [None if s is None else up(eng, s) for s in st.s]
    h = dict(hp)
    b1p, b2p = U.adam_powers(hp, step) if opt == "adam" else (0.5, 0.5)
    h.update(beta1_power=float(b1p), beta2_power=float(b2p))
    if pre_clip:
        eng.clip_grads()
    eng.apply_update(opt, slots[0], slots[1], h, grad_scale=float(grad_scale), fuse_clip=fuse_clip,
                     dev_powers=dev_powers)
    new = State.__new__(State)
    new.p = eng.params.cpu().numpy()
    new.s = [None if s is None else s.cpu().numpy() for s in slots]
    new.g = eng.grads.cpu().numpy()
    return new


class Tally(object):
    """Worst GPU error and yardstick per measure of a case, and every figure behind them."""

    def __init__(self):
        self.worst, self.yard, self.detail, self.problems = {}, {}, [], []

    def settle(self, tag):
        yard = {m: U.floor(v) for m, v in self.yard.items()}
        for m, v in yard.items():
            assert v < U.YARDSTICK_CAP, (m, v)
        report(tag, self.worst, yard)
        for m, e, form, step, name in self.detail:
            if not e <= U.GPU_FACTOR * yard[m]:
                self.problems.append(("outside the bound", m, form, step, name, e, yard[m]))


def check_step(layout, gaps, before, after, opt, hp, step, raw, clipped, scale, cache, tally, tag):
    """`after` against the float64 update of `before`, per tensor; the gaps unchanged.  `cache`
    ({tensor: (inputs, reference)}) spares the forms that start a step from the same bits a
    second evaluation of the same reference."""
    for a, b in zip(after.flats(), before.flats()):
        if not np.array_equal(bits(a[gaps]), bits(b[gaps])):
            tally.problems.append(("alignment gap written", tag, step))
    if not np.all(bits(after.g[gaps]) == bits(np.float32(GRAD_GAP))):
        tally.problems.append(("alignment gap of the gradient written", tag, step))
    pw = U.adam_powers(hp, step) if opt == "adam" else None
    for i, (name, _, _, _) in enumerate(layout):
        ins = before.tensor(layout, i)
        hit = cache.get(i)
        if hit is not None and all(x is None or U.same_bits(x, y) for x, y in zip(ins, hit[0])):
            r64, y = hit[1]
        else:
            r64, y = U.reference_update(opt, hp, raw[i], ins[0], ins[1], ins[2], pw, scale,
                                        None if clipped is None else (clipped[0][i], clipped[1][i]))
            cache[i] = (ins, (r64, y))
        e = U.update_errs(after.tensor(layout, i), r64, ins[0])
        for m in e:
            tally.yard[m] = max(tally.yard.get(m, 0.0), y[m])
            tally.worst[m] = max(tally.worst.get(m, 0.0), e[m])
            tally.detail.append((m, e[m], tag, step, name))


@pytest.mark.parametrize("opt,k", U.PAIRS)
@pytest.mark.parametrize("geom", GEOMS)
def test_update_forms_agree_and_match_float64(geom, opt, k, monkeypatch):
    fused, unfused = engines(geom, monkeypatch)
    hp = U.HP[opt][k]
    layout, size = fused.layout, fused.flat_size
    gaps = U.gap_mask(layout, size)
    forms = {"A": (fused, dict(fuse_clip=True)),                  # clip_update, or its fallback
             "B": (unfused, dict(fuse_clip=True)),                # sumsq + update with the clip
             "C": (fused, dict(fuse_clip=False, pre_clip=True))}  # sumsq + clip, then update
    state = {f: State(fused, geom, opt) for f in forms}
    dev = {}
    if opt == "adam":
        for f in ("A", "B"):
            e = forms[f][0]
            dev[f] = (State(fused, geom, opt),
                      torch.tensor(U.adam_powers(hp, 0), dtype=torch.float32, device=e.device))
    tally = Tally()
    problems = tally.problems
    for step in range(U.NSTEPS):
        raw, c64, c32 = dealt(geom, step)
        gflat = U.pack(layout, size, raw, GRAD_GAP)
        cache = {}
        new = {}
        for f, (eng, kw) in forms.items():
            new[f] = run_form(eng, state[f], opt, hp, gflat, step, **kw)
            check_step(layout, gaps, state[f], new[f], opt, hp, step, raw, (c64, c32), None, cache,
                       tally, f)
        for f in ("B", "C"):
            for name, a, b in zip(("params", "slot 0", "slot 1"), new["A"].flats(), new[f].flats()):
                if not np.array_equal(bits(a), bits(b)):
                    problems.append(("forms A and %s differ" % f, step, name,
                                     int((bits(a) != bits(b)).sum())))
        for f, (st, powers) in dev.items():
            nd = run_form(forms[f][0], st, opt, hp, gflat, step, fuse_clip=True, dev_powers=powers)
            for name, a, b in zip(("params", "slot 0", "slot 1"), nd.flats(), new[f].flats()):
                if not np.array_equal(bits(a), bits(b)):
                    problems.append(("device powers differ from host powers", f, step, name))
            dev[f] = (nd, powers)
            want = np.array(U.adam_powers(hp, step + 1), np.float32)
            if not np.array_equal(bits(powers.cpu().numpy()), bits(want)):
                problems.append(("device powers off the float32 chain", f, step))
        state = new
    tally.settle("update %s %s hp%d" % (geom, opt, k))
    assert fused.device_errors() == 0 and unfused.device_errors() == 0
    assert not problems, digest(problems)


# --- c. the unfused apply with a gradient scale ---------------------------------------------------
@pytest.mark.parametrize("opt,k", U.PAIRS)
@pytest.mark.parametrize("geom", ["odd", "over"])
def test_unfused_scaled_update_matches_float64(geom, opt, k, monkeypatch):
    eng, _ = engines(geom, monkeypatch)
    hp = U.HP[opt][k]
    layout, size = eng.layout, eng.flat_size
    gaps = U.gap_mask(layout, size)
    scale = np.float32(1.0) / np.float32(3.0)
    st = State(eng, geom, opt)
    tally = Tally()
    problems = tally.problems
    for step in range(2):
        raw = U.dealt_gradients(geom, step, U.deal_scale(geom, step), salt=1)
        gflat = U.pack(layout, size, raw, GRAD_GAP)
        new = run_form(eng, st, opt, hp, gflat, step, fuse_clip=False, grad_scale=scale)
        check_step(layout, gaps, st, new, opt, hp, step, raw, None, scale, {}, tally,
                   "scaled")
        if not np.array_equal(bits(new.g), bits(gflat)):
            problems.append(("the unfused apply wrote the gradient", step))
        st = new
    tally.settle("scaled %s %s hp%d" % (geom, opt, k))
    assert eng.device_errors() == 0
    assert not problems, digest(problems)


# --- d. both sides of every dispatch ran --------------------------------------------------------------
def test_geometries_lie_on_both_sides_of_the_cu_count(monkeypatch):
    counts = {}
    for geom in GEOMS:
        eng, _ = engines(geom, monkeypatch)
        counts[geom] = U.chunk_count([n for _, _, n, _ in eng.layout])
    n = cus()
    U.check_cu_sides(n, counts)
    assert counts["over"] > n          # a. and b. took the fallback launches on the default handle
    assert counts["bench"] <= n        # and the one-launch forms
    tb, _ = engines("over", monkeypatch)[0].bucket_split()
    lay = engines("over", monkeypatch)[0].layout
    assert U.chunk_count([x[2] for x in lay[:tb]]) <= n < U.chunk_count([x[2] for x in lay[tb:]])
