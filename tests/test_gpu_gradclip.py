"""The global-norm gradient clip (gnorm_partials_kernel / gnorm_scale_kernel, csrc/ba3c_small.h,
behind ba3c_clip_grads_global) against its oracle ba3c_amd/gradclip.py on the crafted gradients of
tests/flat_updates.py; the learner step with `Model(max_grad_norm=)`; the learning-rate and
entropy-coefficient schedules on the device; and the launcher's flags and channels.

Bounds of the kernel test.  The norm: the float64 sum of <= 438 partials of <= 4096 exact products
each, summed in a fixed tree, lies within a few 1e-16 relative of the exact sum; 1e-12 is loose by
four orders of magnitude.  f = max_norm / norm is one division (2e-12 carries the norm's bound
through it with room for its rounding), and an element is one product and the final rounding:
|g' - ref64| <= ulp32(ref64) / 2 + 2e-12 |ref64|.  None of them is measured from the kernels.
"""
import functools
import os

import numpy as np
import pytest
import torch

import flat_updates as U
from ba3c_amd import gradclip as G
from ba3c_amd import schedule as S
from oracle import ba3c_oracle as O

pytestmark = pytest.mark.gpu

GEOMS = ("odd", "bench", "over")
CHUNKS = {"odd": 52, "bench": 237, "over": 438}
GAP = 1e30
f32, f64 = np.float32, np.float64

_ENGINES = {}


def flat_engine(geom):
    if geom not in _ENGINES:
        from ba3c_amd.engine import Ba3cEngine
        g = U.GEOMETRIES[geom]
        eng = Ba3cEngine(num_actions=g["A"], channels=g["C"], fc_neurons=g["F"], fc_splits=g["S"],
                         replace_with_conv=not g["legacy"], ps=g["ps"], max_batch=1)
        assert [(n, k) for n, _, k, _ in eng.layout] == U.tensors(geom)
        assert U.chunk_count([n for _, _, n, _ in eng.layout]) == CHUNKS[geom]
        _ENGINES[geom] = eng
    return _ENGINES[geom]


@functools.lru_cache(maxsize=None)
def dealt(geom, step):
    """(gradients, the oracle's norm): computed once, read by every case."""
    g = U.dealt_gradients(geom, step)
    for x in g:
        x.setflags(write=False)
    return g, G.global_norm_numpy(g)


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def test_the_geometries_lie_on_both_sides_of_the_cu_count():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert CHUNKS["bench"] <= cus < CHUNKS["over"]


# --- the kernels against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("step", range(U.NSTEPS))
@pytest.mark.parametrize("geom", GEOMS)
def test_kernels_match_the_oracle(geom, step):
    eng = flat_engine(geom)
    layout, size = eng.layout, eng.flat_size
    gaps = U.gap_mask(layout, size)
    assert gaps.any()
    g, norm = dealt(geom, step)
    assert np.isfinite(norm) and norm > 0.0
    flat = U.pack(layout, size, g, GAP)
    dev = torch.from_numpy(flat).to(eng.device)
    problems = []
    for tag, max_norm in (("0.5", 0.5), ("norm/3", norm / 3.0), ("2*norm", 2.0 * norm)):
        assert abs(norm / max_norm - 1.0) >= 1e-3, (tag, norm)     # a condition on the inputs
        ref, onorm, f = G.clip_numpy(g, max_norm)
        assert onorm == norm
        runs = []
        for _ in range(2):                                         # a second launch on the same input
            eng.grads.copy_(dev)
            stats = eng.clip_grads_global(max_norm)
            runs.append((eng.grads.cpu().numpy(), stats.cpu().numpy().copy()))
        got, (gnorm, gf) = runs[0]
        print("gradclip %s step %d max_norm %s: norm rel err %.2e, f rel err %.2e"
              % (geom, step, tag, abs(gnorm - norm) / norm, abs(gf - f) / f))
        if not abs(gnorm - norm) <= 1e-12 * norm:
            problems.append(("norm", tag, gnorm, norm))
        if not abs(gf - f) <= 2e-12 * f:
            problems.append(("f", tag, gf, f))
        worst = 0.0
        for (name, _, _, _), x, r in zip(layout, U.unpack(layout, got), ref):
            half = 0.5 * np.spacing(np.abs(r).astype(f32)).astype(f64)
            err = np.abs(x.astype(f64) - r)
            bound = half + 2e-12 * np.abs(r)
            worst = max(worst, float((err / bound).max()))
            if not np.all(err <= bound):
                problems.append(("element outside the bound", tag, name, float((err / bound).max())))
        print("gradclip %s step %d max_norm %s: worst element error / bound %.3f" % (geom, step, tag, worst))
        if tag == "2*norm":
            if gf != 1.0:
                problems.append(("f is not exactly 1.0 where nothing is clipped", gf))
            if not np.array_equal(bits(got), bits(flat)):
                problems.append(("the unclipped buffer changed its bits", tag))
        else:
            assert f < 1.0
        if not np.array_equal(bits(got[gaps]), bits(flat[gaps])):
            problems.append(("alignment gap written", tag))
        if not (np.array_equal(bits(runs[1][0]), bits(got))
                and np.array_equal(runs[1][1].view(np.uint64), runs[0][1].view(np.uint64))):
            problems.append(("a second launch gave other bits", tag))
    assert eng.device_errors() == 0
    assert not problems, problems


def test_a_nan_gradient_keeps_its_bits():
    eng = flat_engine("odd")
    g = [x.copy() for x in dealt("odd", 0)[0]]
    g[3][0] = np.nan
    flat = U.pack(eng.layout, eng.flat_size, g, GAP)
    eng.grads.copy_(torch.from_numpy(flat).to(eng.device))
    norm, f = eng.clip_grads_global(0.5).cpu().numpy()
    assert np.isnan(norm) and f == 1.0
    assert np.array_equal(bits(eng.grads.cpu().numpy()), bits(flat))


# --- the step -----------------------------------------------------------------------------------------
B, F, SPLITS, A = 8, 128, 4, 4                      # the shapes of tests/golden/step_B8_F128_S4.npz
ADAM = (1e-3, 0.8, 0.75, 1e-8)


def _batch(seed):
    rs = np.random.RandomState(seed)
    d = lambda x: torch.from_numpy(x).cuda()
    return (d(rs.randint(0, 256, size=(B, 84, 84, 4)).astype(np.uint8)),
            d(rs.randint(0, A, size=B).astype(np.int64)), d(rs.normal(size=B).astype(f32)))


def _trainer(max_grad_norm=None, sync=False, lr=ADAM[0]):
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer, SyncReplicasOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    m = Model(num_actions=A, fc_neurons=F, fc_splits=SPLITS, batch_size=B, max_batch=16,
              max_grad_norm=max_grad_norm)
    m.engine.load_params(O.init_params(F, SPLITS, A, seed=5, dtype=f32))
    opt = AdamOptimizer(lr, *ADAM[1:])
    if sync:
        assert not torch.distributed.is_initialized()
        opt = SyncReplicasOptimizer(opt)
    return Ba3cTrainer(TrainConfig(model=m, optimizer=opt))


def _state(tr):
    inner = getattr(tr.optimizer, "_opt", tr.optimizer)
    torch.cuda.synchronize()
    return [tr.engine.params.clone()] + [s.clone() for s in inner.slots]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _ppo_rows(tr, batch):
    """{R, V_old, l_old, 0} of a behaviour policy a little off the learner's."""
    state, action, R = batch
    probs, _, value = tr.engine.forward(state)
    l_old = torch.log(probs.double()[torch.arange(B), action] + 1e-6) + 0.05 * torch.linspace(-1, 1, B).cuda().double()
    rows = torch.stack([R, value + 0.1, l_old.float(), torch.zeros_like(R)], dim=1).contiguous()
    return rows


def _by_hand(batch, max_norm, rows=None, clip=None):
    """train_grads, then clip_grads_global (max_norm None: the parent's fused clip), then
    apply_update, on a fresh engine; returns (state after, the raw gradient's oracle norm)."""
    tr = _trainer()
    eng, opt = tr.engine, tr.optimizer
    if rows is None:
        eng.train_grads(*batch)
    else:
        eng.train_grads_ppo(batch[0], batch[1], rows, clip)
    norm = G.global_norm_numpy(list(eng.state_dict(eng.grads).values()))
    opt.slots = opt._init_slots(eng)
    if max_norm is not None:
        eng.clip_grads_global(max_norm)
    eng.apply_update("adam", opt.slots[0], opt.slots[1], opt._hparams(), grad_scale=1.0,
                     fuse_clip=max_norm is None)
    return _state(tr), norm


@pytest.mark.parametrize("loss", ["a3c", "ppo"])
def test_the_step_equals_the_three_calls_made_by_hand(loss):
    batch = _batch(300)
    kw = {}
    if loss == "ppo":
        kw = dict(rows=_ppo_rows(_trainer(), batch), clip=0.2)
    parent, norm = _by_hand(batch, None, **kw)
    m = norm / 4.0
    assert 0.0 < m < norm                                         # the clip is active
    hand, _ = _by_hand(batch, m, **kw)
    tr = _trainer(max_grad_norm=m)
    assert not tr._fused_clip
    tr.train_step(*batch, **kw)
    got = _state(tr)
    gnorm, f = tr._procs[0].last_stats.cpu().numpy()
    assert abs(gnorm - norm) <= 1e-12 * norm and f < 1.0
    assert _same(got, hand)
    assert not torch.equal(got[0], parent[0])                     # and it is not the default step
    default = _trainer()
    assert default._fused_clip
    default.train_step(*batch, **kw)
    assert _same(_state(default), parent)                         # max_grad_norm=None: as it was
    for t in (tr, default):
        assert t.engine.device_errors() == 0


def test_sync_replicas_without_a_group_equals_the_single_replica():
    batches = [_batch(310), _batch(311)]
    single, sync = _trainer(max_grad_norm=0.5), _trainer(max_grad_norm=0.5, sync=True)
    for b in batches:
        single.train_step(*b)
        sync.train_step(*b)
    assert _same(_state(single), _state(sync))
    assert sync.optimizer.local_step == 2                         # the flat exchange's path ran


def test_a_captured_replay_equals_the_eager_step():
    bs = [_batch(320 + i) for i in range(3)]
    eager = _trainer(max_grad_norm=0.5)
    for b in bs[1:]:
        eager.train_step(*b)
    cap = _trainer(max_grad_norm=0.5)
    cap.schedules = {"learning_rate": S.parse("const", ADAM[0])}  # a constant schedule captures
    static = tuple(t.clone() for t in bs[0])
    replay = cap.capture_step(*static, warmup=2)
    for b in bs[1:]:
        for dst, src in zip(static, b):
            dst.copy_(src)
        replay()
    assert cap.global_step == eager.global_step == 2
    assert _same(_state(cap), _state(eager))
    assert cap.optimizer.powers() == eager.optimizer.powers()
    assert cap.engine.device_errors() == 0


def test_capture_refuses_a_linear_schedule():
    tr = _trainer(max_grad_norm=0.5)
    tr.schedules = {"learning_rate": S.parse("linear:0", ADAM[0], max_steps=10)}
    with pytest.raises(ValueError, match="schedule"):
        tr.capture_step(*_batch(330))
    assert tr.global_step == 0


# --- schedules on the device ----------------------------------------------------------------------------
def test_two_adam_steps_under_a_learning_rate_schedule():
    bs = [_batch(340), _batch(341)]
    sched = _trainer()
    sched.schedules = {"learning_rate": S.parse("steps:1=5e-4", ADAM[0], steps_per_epoch=1)}
    hand = _trainer()
    for i, b in enumerate(bs):
        sched.train_step(*b)
        hand.optimizer.learning_rate = (ADAM[0], 5e-4)[i]
        hand.train_step(*b)
    assert sched.optimizer.learning_rate == 5e-4
    assert _same(_state(sched), _state(hand))
    flat = _trainer()                                             # and the schedule did something
    for b in bs:
        flat.train_step(*b)
    assert not torch.equal(_state(flat)[0], _state(sched)[0])


def test_two_steps_under_an_entropy_schedule():
    bs = [_batch(350), _batch(351)]
    sched = _trainer()
    sched.schedules = {"entropy_beta": S.parse("steps:1=0.005", 0.02, steps_per_epoch=1)}
    hand = _trainer()
    seen = []
    for i, b in enumerate(bs):
        sched.train_step(*b)
        hand.model.entropy_beta = (0.02, 0.005)[i]
        hand.train_step(*b)
        assert torch.equal(sched.model.scalars, hand.model.scalars)
        seen.append(sched.model.scalars.clone())
    assert sched.model.entropy_beta == 0.005
    assert _same(_state(sched), _state(hand))
    flat = _trainer()                                             # beta 0.01 throughout: another cost
    flat.train_step(*bs[0])
    assert not torch.equal(flat.model.scalars[:1], seen[0][:1])


# --- the launcher -----------------------------------------------------------------------------------------
RUN = ("-e GridBreakout-v0 -b 32 --fc_neurons 128 --fc_splits 4 --simulator_procs 64 --max_steps 6 "
       "--steps_per_epoch 3 --send_debug_every 2").split()
NEW = ("--max_grad_norm 0.5 --lr_schedule linear:0 --entropy_beta 0.02 "
       "--entropy_schedule steps:1=0.005").split()
FILES = ("grad_norm", "grad_clip_fraction", "learning_rate", "entropy_beta")
PARENT_KEYS = {"rank", "world", "global_step", "simulator_steps", "samples_per_s", "last"}


def _rows(path):
    lines = open(path).read().strip().splitlines()
    assert lines[0] == "x,y"
    return [float(r.split(",")[1]) for r in lines[1:]]


def _windows(values, every):
    return [values[i:i + every] for i in range(0, len(values), every)]


def test_the_launcher_writes_the_channels_and_the_json(tmp_path):
    from ba3c_amd.train import main
    out = main(RUN + NEW + ["--experiment_dir", str(tmp_path)])
    n = out["global_step"]
    assert n >= 6 and all(np.isfinite(v) for v in out["last"].values())
    lr = S.parse("linear:0", 0.00015, max_steps=6)
    beta = S.parse("steps:1=0.005", 0.02, steps_per_epoch=3)
    for name, fn in (("learning_rate", lr), ("entropy_beta", beta)):
        want = [sum(w) / len(w) for w in _windows([fn(s) for s in range(n)], 2)]
        got = _rows(str(tmp_path / (name + ".csv")))
        print(name, got)
        assert got == pytest.approx(want, rel=1e-12, abs=0.0)
    norms, fracs = _rows(str(tmp_path / "grad_norm.csv")), _rows(str(tmp_path / "grad_clip_fraction.csv"))
    print("grad_norm", norms, "grad_clip_fraction", fracs)
    assert len(norms) == len(fracs) == len(_windows(list(range(n)), 2))
    assert all(np.isfinite(v) and v > 0.0 for v in norms) and all(v in (0.0, 0.5, 1.0) for v in fracs)
    assert set(out) == PARENT_KEYS | {"grad_clip", "schedule"}
    assert out["grad_clip"] == {"max_norm": 0.5, "grad_norm": norms[-1], "clip_fraction": fracs[-1]}
    assert out["schedule"] == {"learning_rate": lr(n - 1), "entropy_beta": beta(n - 1)}


def test_the_launcher_with_the_ppo_loss(tmp_path):
    from ba3c_amd.train import main
    out = main(RUN + NEW + ["--ppo_clip", "0.2", "--experiment_dir", str(tmp_path)])
    assert out["global_step"] >= 6 and all(np.isfinite(v) for v in out["last"].values())
    assert np.isfinite(out["grad_clip"]["grad_norm"]) and "ppo" in out
    for name in FILES:
        assert os.path.exists(str(tmp_path / (name + ".csv"))), name


def test_the_launcher_without_the_flags_is_the_parents(tmp_path):
    from ba3c_amd.train import main
    out = main(RUN + ["--experiment_dir", str(tmp_path)])
    assert set(out) == PARENT_KEYS
    for name in FILES:
        assert not os.path.exists(str(tmp_path / (name + ".csv"))), name
