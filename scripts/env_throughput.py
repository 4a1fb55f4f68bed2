"""Environment step time on the GPU (GridBreakout / GridBoxing sections): µs per fused
`step_into` of the on-device game (--game breakout: `BreakoutVec`; --game boxing: `BoxingVec`,
timed next to GridBreakout's fused step in the same run) against `SyntheticAtari.step` +
`FrameHistory.push`, and the fused
kernel's achieved bytes/s against this box's measured HBM copy rate (a device-to-device copy, and
an in-place update over the kernel's own footprint).  With --random N also the
evaluation scores of a uniform-random policy (and, for boxing, of a NOOP policy) over N
episodes (under the frame skip / stickiness given).  With --frame_skip K | LO-HI and / or --sticky P also the frame-skip step (one
launch per DECISION, ba3c_amd.frameskip), timed alternately with the one-step fused step in the
same run: µs per decision, µs per game step (at the mean k = (LO + HI) / 2 of the draw) and the
ratios to one and to k one-step launches.  With --view S [S ...] also the colour view
(`Vec.view`, ba3c_amd.view) of all E simulators with a HUD at each scale S, timed alternately with
the fused step in the same run, and its store rate (Hc*S * 252*S bytes per simulator, Hc = 104).
With --duel also two-player GridBoxing (`BoxingDuelVec.step_into`, ba3c_amd.duel) at G = E / 2
games next to `BoxingVec.step_into` at E simulators (by default G = 4096 against E = 8192 and
G = 32 against E = 64: the same players and bytes), timed alternately in the same run.
With --duel the decision launch (`ba3c_boxing_duel_decide`: frame skip, sticky actions per side, drawn
starts) is timed next to `ba3c_boxing_duel_step` too, alternating in the same run: at (1, 1, 0) with
the fixed start against one step, one k = 4 launch against four back-to-back one-step launches,
and the setting of --frame_skip / --sticky / --duel_start (default 2-4, 0.25, 8-14) for the
record; --duel_only skips the single-player tables.
With --returns also `ba3c_lambda_returns` (lambda = 0.95 and 1) next to `ba3c_nstep_returns` on
identical full memories at (simulators, slots) = (100, 6), (1024, 33), (4096, 129), the median
of 20 event-bracketed batches of 20 launches each, alternating; and ms per
`ActorLearner.iterate` on GridBoxing at 100 simulators with the default returns and with
20-step GAE(0.95) returns.
With --ppo also the PPO learner step (`Ba3cTrainer.train_step(..., rows, clip)`, ba3c_amd.ppo) next
to the A3C step on identical batches at (B, F, S) = (32, 128, 4) and (2048, 512, 1), by the same
method (medians of event-bracketed batches of steps, alternating), and ms per
`ActorLearner.iterate` and samples/s on GridBoxing at 100 simulators with the A3C loop and with
--ppo_clip 0.2 at 4 epochs x 4 minibatches; --ppo_only skips the environment tables.  With
--ppo_norm_adv and / or --ppo_vclip EPS the extended step (the normalisation launch and the same
PPO step with those settings on) and the normalisation launch alone are timed in the same
alternation, and the loop once more with those settings.
With --episodes also the episode log of the training simulators (`ba3c_episode_stats`,
ba3c_amd.episodes) alone at 100, 4096 and 65536 simulators (one flag in a hundred set), by the same
medians of event-bracketed batches, and ms per `ActorLearner.iterate` on GridBreakout at 100 and
4096 simulators without and with a log, alternating in the same call; --episodes_only skips the
environment tables.
With --gradclip also the learner step with the reference's fused per-tensor clip next to the step
with the global-norm clip (`Model(max_grad_norm=0.5)`, ba3c_amd.gradclip) on identical batches at
(B, F, S) = (32, 128, 4) and (2048, 512, 1), fresh trainers, alternating, by the same medians; and
the clip's two launches alone at both flat sizes; --gradclip_only skips the environment tables.
Prints one JSON line.

    python scripts/env_throughput.py [--game boxing] [--envs 8192 64] [--iters 200] [--random 20]
                                     [--frame_skip 2-4] [--sticky 0.25] [--view 1 3] [--duel]
                                     [--duel_start 8-14] [--duel_only] [--returns] [--ppo] [--ppo_only]
                                     [--ppo_norm_adv] [--ppo_vclip 0.2] [--episodes] [--episodes_only]
                                     [--gradclip] [--gradclip_only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-ba3c_amd")]

import torch  # noqa: E402

STATE_BYTES = 84 * 84 * 4


def timed(fn, iters, warmup=20):
    """Mean µs per call between two device events around `iters` back-to-back calls."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def duel_table(envs, iters, repeats):
    """--duel: BoxingDuelVec.step_into at G = E / 2 games next to BoxingVec.step_into at E
    simulators (the same number of players, frames and history bytes), alternating."""
    from ba3c_amd.boxing import BoxingVec
    from ba3c_amd.duel import BoxingDuelVec
    from ba3c_amd.rollout import FrameHistory
    out = {}
    for E in envs:
        G = E // 2
        g = torch.Generator(device="cuda").manual_seed(0)
        actions = torch.randint(0, 18, (2 * G,), generator=g, device="cuda")
        duel, hist_d = BoxingDuelVec(G, seed=0), FrameHistory(2 * G, 4, 1)
        duel.reset_history(hist_d)
        solo, hist_s = BoxingVec(2 * G, seed=0), FrameHistory(2 * G, 4, 1)
        solo.reset_history(hist_s)
        t_duel, t_solo = [], []
        for _ in range(repeats):
            t_duel.append(timed(lambda: duel.step_into(actions, hist_d), iters))
            t_solo.append(timed(lambda: solo.step_into(actions, hist_s), iters))
        traffic = 2 * (2 * G) * STATE_BYTES
        out[str(G)] = {"players": 2 * G, "duel_step_into_us": [round(v, 2) for v in t_duel],
                       "boxing_step_into_us": [round(v, 2) for v in t_solo], "state_bytes": traffic,
                       "duel_GBps": round(traffic / min(t_duel) / 1e3, 1),
                       "boxing_GBps": round(traffic / min(t_solo) / 1e3, 1),
                       "duel_over_boxing": round(min(t_duel) / min(t_solo), 3)}
    return out


def duel_decision_table(envs, iters, repeats, skip, start):
    """--duel: BoxingDuelDecisionVec on the decision launch next to the one-step launch at the
    same G, alternating.  skip (lo, hi, q16) and start (h_lo, h_hi): the setting timed for the record."""
    from ba3c_amd.duel import FIXED_START, BoxingDuelDecisionVec, BoxingDuelVec
    from ba3c_amd.rollout import FrameHistory
    out = {}

    def vec(G, skip, start):
        v = BoxingDuelDecisionVec(G, seed=0, frame_skip=2)    # on the decision launch, then the setting
        v.skip, v.start = skip, start
        h = FrameHistory(2 * G, 4, 1)
        v.reset_history(h)
        return v, h
    for E in envs:
        G = E // 2
        g = torch.Generator(device="cuda").manual_seed(0)
        actions = torch.randint(0, 18, (2 * G,), generator=g, device="cuda")
        step, hist_s = BoxingDuelVec(G, seed=0), FrameHistory(2 * G, 4, 1)
        step.reset_history(hist_s)
        legs = {"decide_1_1_0": vec(G, (1, 1, 0), FIXED_START), "decide_4_4_0": vec(G, (4, 4, 0), FIXED_START),
                "decide_setting": vec(G, skip, start)}

        def four():
            for _ in range(4):
                step.step_into(actions, hist_s)
        t = {k: [] for k in list(legs) + ["step", "four_steps"]}
        for _ in range(repeats):
            t["step"].append(timed(lambda: step.step_into(actions, hist_s), iters))
            for k, (v, h) in legs.items():
                t[k].append(timed(lambda: v.step_into(actions, h), iters))
            t["four_steps"].append(timed(four, iters))
        row = {k + "_us": [round(x, 2) for x in v] for k, v in t.items()}
        row.update(setting={"skip": list(skip), "start": list(start)},
                   decide_over_step=round(min(t["decide_1_1_0"]) / min(t["step"]), 3),
                   k4_over_four_steps=round(min(t["decide_4_4_0"]) / min(t["four_steps"]), 3),
                   setting_over_step=round(min(t["decide_setting"]) / min(t["step"]), 3))
        out[str(G)] = row
    return out


def timed_median(fn, batches=20, per=20, warmup=20):
    """Median over `batches` of the mean µs per call of `per` back-to-back calls between two
    device events (events around batches, not single launches: DESIGN.md §5's event gap)."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(batches):
        out.append(timed(fn, per, warmup=0))
    return sorted(out)[len(out) // 2]


RETURNS_SHAPES = [(100, 6), (1024, 33), (4096, 129)]


def returns_table(repeats):
    """--returns: `ba3c_lambda_returns` at lambda = 0.95 and lambda = 1 next to
    `ba3c_nstep_returns` on identical full memories (every simulator holds `slots` transitions,
    one in three over), alternating; the lambda = 1 outputs are compared with the n-step ones."""
    import ctypes

    from ba3c_amd import _lib
    lib = _lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {}
    for E, T in RETURNS_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(E)
        reward = torch.randint(-2, 3, (E, T), generator=g, device="cuda").to(torch.float64)
        value = torch.randn(E, T, generator=g, device="cuda") * 3
        start = torch.randint(0, T, (E,), generator=g, device="cuda").to(torch.int32)
        length = torch.full((E,), T, dtype=torch.int32, device="cuda")
        over = (torch.arange(E, device="cuda") % 3 == 0).to(torch.uint8)
        outs = {}

        def leg(name, lam=None):
            """Buffers and arguments built once: the timed call is the entry point alone."""
            o = outs[(name, lam)] = [
                torch.zeros(E * T, dtype=torch.float32, device="cuda"),
                torch.zeros(E * T, dtype=torch.int32, device="cuda"),
                torch.zeros(E * T, dtype=torch.float32, device="cuda"),
                torch.zeros(E * T, dtype=torch.uint8, device="cuda"),
                torch.zeros(1, dtype=torch.int32, device="cuda")]
            a = [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), P(reward), P(value),
                 P(start), P(length), P(over), E, T, ctypes.c_double(0.99)]
            a += [] if lam is None else [ctypes.c_double(lam)]
            a += [P(t) for t in o]
            fn = getattr(lib, name)
            return lambda: fn(*a)
        legs = {"nstep_us": leg("ba3c_nstep_returns"),
                "lambda_0.95_us": leg("ba3c_lambda_returns", 0.95),
                "lambda_1_us": leg("ba3c_lambda_returns", 1.0)}
        for fn in legs.values():
            _lib.check(fn())
        t = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():
                t[k].append(timed_median(fn))
        same = all(torch.equal(a, b) for a, b in zip(outs[("ba3c_nstep_returns", None)],
                                                     outs[("ba3c_lambda_returns", 1.0)]))
        row = {k: [round(v, 2) for v in vs] for k, vs in t.items()}
        row["datapoints"] = int(outs[("ba3c_nstep_returns", None)][4].item())
        row["lambda_1_equals_nstep"] = bool(same)
        for k in ("lambda_0.95_us", "lambda_1_us"):
            row[k.replace("_us", "_over_nstep")] = round(min(t[k]) / min(t["nstep_us"]), 3)
        out["%dx%d" % (E, T)] = row
    return out


PPO_SHAPES = [(32, 128, 4), (2048, 512, 1)]


def ppo_step_table(repeats, clip=0.2, norm_adv=False, vclip=0.0):
    """--ppo: µs per learner step (pass + fused clip + Adam apply) with the A3C loss and with the
    clipped-surrogate loss on the same batch: rows = {R, the forward's value, sample_logp's logp,
    0} of the policy before the timed steps, so the ratios move as the steps train.
    norm_adv / vclip (--ppo_norm_adv / --ppo_vclip): also the extended step — the normalisation
    launch (when asked for) and the same step, the same heads kernel, with those settings on —
    and the normalisation launch alone, in the same alternation."""
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    out = {}
    for B, F, S in PPO_SHAPES:
        m = Model(num_actions=4, fc_neurons=F, fc_splits=S, batch_size=B, max_batch=B, seed=0)
        tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-5, 0.8, 0.75, 1e-8)))
        g = torch.Generator(device="cuda").manual_seed(B)
        st = torch.randint(0, 256, (B, 84, 84, 4), generator=g, device="cuda").to(torch.uint8)
        R = torch.randn(B, generator=g, device="cuda")
        u = torch.rand(B, generator=g, device="cuda", dtype=torch.float64)
        probs, probsT, value = m.engine.forward(st)
        ac, logp, _ = m.engine.sample_logp(probsT, probs, u)
        rows = torch.stack([R, value, logp, torch.zeros_like(R)], dim=1).contiguous()
        legs = {"a3c_us": lambda: tr.train_step(st, ac, R),
                "ppo_us": lambda: tr.train_step(st, ac, None, rows=rows, clip=clip)}
        if norm_adv or vclip:
            def ext():
                if norm_adv:
                    m.engine.ppo_norm_adv(rows)
                tr.train_step(st, ac, None, rows=rows, clip=clip, vclip=vclip, adv_from_row=norm_adv)
            legs["ppo_ext_us"] = ext
            legs["norm_adv_us"] = lambda: m.engine.ppo_norm_adv(rows)
        t = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():
                t[k].append(timed_median(fn))
        row = {k: [round(v, 2) for v in vs] for k, vs in t.items()}
        row["ppo_over_a3c"] = round(min(t["ppo_us"]) / min(t["a3c_us"]), 4)
        if "ppo_ext_us" in t:
            row["ppo_ext_over_ppo"] = round(min(t["ppo_ext_us"]) / min(t["ppo_us"]), 4)
        row["clip_fraction_after"] = round(float(((m.ratio - 1).abs() > clip).float().mean().item()), 4)
        out["B%d_F%d_S%d" % (B, F, S)] = row
        tr.check_device_errors()
    return out


def gradclip_table(repeats, max_norm=0.5):
    """--gradclip: ms per learner step (pass + clip + Adam apply) with the reference's fused
    per-tensor clip and with the global-norm clip (`Model(max_grad_norm=)`: two launches, then the
    unfused apply) on the same batch, fresh trainers, alternating, by medians of event-bracketed
    batches of steps; and the clip's two launches alone on the step's gradient, µs per call of
    both and per launch: with every call clipping (max_norm shrinks by 0.1 % per call, so the
    stores run) and with none (max_norm far above the norm: the stores are skipped)."""
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    out = {}
    for B, F, S in PPO_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B)
        st = torch.randint(0, 256, (B, 84, 84, 4), generator=g, device="cuda").to(torch.uint8)
        ac = torch.randint(0, 4, (B,), generator=g, device="cuda")
        R = torch.randn(B, generator=g, device="cuda")

        def trainer(m):
            model = Model(num_actions=4, fc_neurons=F, fc_splits=S, batch_size=B, max_batch=B, seed=0,
                          max_grad_norm=m)
            return Ba3cTrainer(TrainConfig(model=model, optimizer=AdamOptimizer(1e-5, 0.8, 0.75, 1e-8)))
        plain, clipped = trainer(None), trainer(max_norm)
        legs = {"fused_average_norm_clip_ms": lambda: plain.train_step(st, ac, R),
                "global_norm_clip_ms": lambda: clipped.train_step(st, ac, R)}
        t = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():
                t[k].append(timed_median(fn) / 1e3)
        row = {k: [round(v, 4) for v in vs] for k, vs in t.items()}
        row["global_over_fused"] = round(min(t["global_norm_clip_ms"]) / min(t["fused_average_norm_clip_ms"]), 4)
        row["added_us"] = round((min(t["global_norm_clip_ms"]) - min(t["fused_average_norm_clip_ms"])) * 1e3, 2)
        norm, f = clipped._procs[0].last_stats.tolist()
        row["last_norm"], row["last_f"] = norm, f
        eng = clipped.engine
        row["flat_bytes"] = 4 * eng.flat_size
        shrink = [min(norm, max_norm)]                    # the norm the step's clip left

        def clipping():
            shrink[0] *= 0.999
            eng.clip_grads_global(shrink[0])
        kernels = {"clipping_us": clipping, "not_clipping_us": lambda: eng.clip_grads_global(1e30)}
        tk = {k: [] for k in kernels}
        for _ in range(repeats):
            for k, fn in kernels.items():
                tk[k].append(timed_median(fn))
        for k, vs in tk.items():
            row[k] = [round(v, 2) for v in vs]
            row[k.replace("_us", "_us_per_launch")] = round(min(vs) / 2.0, 2)
        # the back-to-back calls above are bound by the host's issue rate (a Python call per pair of
        # launches); the probe brackets each pair with events on the device (their 5-6 us gap included)
        for k, fn in kernels.items():
            eng.probe_enable("clip")
            for _ in range(200):
                fn()
            ms, n = eng.probe_read()
            eng.probe_enable(None)
            row[k.replace("_us", "_probe_us")] = round(1e3 * ms / max(n, 1), 2)
        out["B%d_F%d_S%d" % (B, F, S)] = row
        plain.check_device_errors()
        clipped.check_device_errors()
    return out


def iterate_table(settings, iters=420, warmup=42, E=100):
    """--returns / --ppo: ms per ActorLearner.iterate on GridBoxing at E simulators (README flags:
    B = 32, F = 128, S = 4, Adam) per (local_time_max, gae_lambda[, ppo.Setting]) setting: a host
    clock around `iters` iterations ending in a device synchronise (420 = a multiple of both
    rollout periods)."""
    import time

    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.boxing import BoxingVec
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    out = {}
    for setting in settings:
        ltm, lam = setting[:2]
        ppo = setting[2] if len(setting) > 2 else None
        m = Model(num_actions=18, fc_neurons=128, fc_splits=4, batch_size=32, max_batch=max(32, E), seed=0)
        tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
        al = ActorLearner(tr, n_envs=E, batch_size=32, seed=0, env=BoxingVec(E, seed=0),
                          local_time_max=ltm, gae_lambda=lam, ppo=ppo)
        al.run(warmup)
        torch.cuda.synchronize()
        steps0, t0 = al.train_steps, time.time()
        al.run(iters)
        torch.cuda.synchronize()
        dt = time.time() - t0
        key = "local_time_max=%d,gae_lambda=%g" % (ltm, lam)
        if ppo is not None:
            key += ",ppo_clip=%g,epochs=%d,minibatches=%d" % tuple(ppo)[:3]
            if ppo.norm_adv or ppo.vclip:
                key += ",norm_adv=%d,vclip=%g" % (ppo.norm_adv, ppo.vclip)
        out.setdefault(key, []).append({
            "ms_per_iterate": round(dt * 1e3 / iters, 3), "iterations": iters,
            "train_steps": al.train_steps - steps0,
            "samples_per_s": round((al.train_steps - steps0) * 32 / dt, 1)})
    return out


EPISODE_SIZES = [100, 4096, 65536]
# (simulators, batch size, timed iterations): windows of about two seconds each
EPISODE_LOOPS = [(100, 32, 2000), (4096, 1024, 300)]


def episodes_table(repeats):
    """--episodes: µs per `ba3c_episode_stats` launch, the entry point alone on buffers built once;
    one flag in a hundred is set, so the ring takes entries at every launch."""
    import ctypes

    from ba3c_amd import _lib
    from ba3c_amd.episodes import EpisodeLog
    lib = _lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {}
    for E in EPISODE_SIZES:
        g = torch.Generator(device="cuda").manual_seed(E)
        reward = torch.randint(-2, 3, (E,), generator=g, device="cuda").to(torch.float64)
        over = (torch.arange(E, device="cuda") % 100 == 7).to(torch.uint8)
        log = EpisodeLog(E)
        a = [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), P(reward), P(over), E, P(log.ret),
             P(log.len), P(log.log_score), P(log.log_len), P(log.log_env), log.cap, P(log.head)]
        fn = lambda: lib.ba3c_episode_stats(*a)
        _lib.check(fn())
        us = [timed_median(fn) for _ in range(repeats)]
        out[str(E)] = {"us": [round(v, 2) for v in us], "flags_set": int(over.sum().item()),
                       "bytes": 21 * E, "cap": log.cap}
    return out


def episodes_iterate_table(repeats=3, warmup=42):
    """--episodes: ms per ActorLearner.iterate on GridBreakout (F = 128, S = 4, Adam) without and
    with an EpisodeLog, fresh loops of the same seed, alternating; a host clock around the
    iterations ending in a device synchronise, as iterate_table."""
    import time

    from ba3c_amd.actor_learner import ActorLearner
    from ba3c_amd.breakout import BreakoutVec
    from ba3c_amd.episodes import EpisodeLog
    from ba3c_amd.model import Model
    from ba3c_amd.optimizer import AdamOptimizer
    from ba3c_amd.trainer import Ba3cTrainer, TrainConfig
    out = {}
    for E, B, iters in EPISODE_LOOPS:
        row = {"batch_size": B, "iterations": iters, "without_ms": [], "with_ms": []}
        for _ in range(repeats):
            for key in ("without_ms", "with_ms"):
                m = Model(num_actions=4, fc_neurons=128, fc_splits=4, batch_size=B, max_batch=max(B, E), seed=0)
                tr = Ba3cTrainer(TrainConfig(model=m, optimizer=AdamOptimizer(1e-3, 0.8, 0.75, 1e-8)))
                log = EpisodeLog(E) if key == "with_ms" else None
                al = ActorLearner(tr, n_envs=E, batch_size=B, seed=0, env=BreakoutVec(E, seed=0), episodes=log)
                al.run(warmup)
                torch.cuda.synchronize()
                t0 = time.time()
                al.run(iters)
                torch.cuda.synchronize()
                row[key].append(round((time.time() - t0) * 1e3 / iters, 4))
                if log is not None:
                    row["episodes_logged"] = int(log.head.item())
                del al, tr, m
        row["with_over_without"] = round(min(row["with_ms"]) / min(row["without_ms"]), 4)
        out[str(E)] = row
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", action="store_true",
                    help="also time ba3c_episode_stats alone and one ActorLearner iteration on "
                         "GridBreakout without and with an episode log")
    ap.add_argument("--episodes_only", action="store_true", help="--episodes: skip the environment tables")
    ap.add_argument("--returns", action="store_true",
                    help="also time ba3c_lambda_returns next to ba3c_nstep_returns, and one "
                         "ActorLearner iteration with 5-step n-step and 20-step GAE(0.95) returns")
    ap.add_argument("--ppo", action="store_true",
                    help="also time the PPO learner step next to the A3C step on identical batches, "
                         "and one ActorLearner iteration with and without --ppo_clip 0.2 (4 x 4)")
    ap.add_argument("--ppo_only", action="store_true", help="--ppo: skip the environment tables")
    ap.add_argument("--ppo_norm_adv", action="store_true",
                    help="--ppo: also time the extended step with the advantage normalisation launch")
    ap.add_argument("--ppo_vclip", type=float, default=0.0,
                    help="--ppo: also time the extended step with this value clip (0: off)")
    ap.add_argument("--gradclip", action="store_true",
                    help="also time the learner step without and with --max_grad_norm 0.5, and the "
                         "global-norm clip's two launches alone")
    ap.add_argument("--gradclip_only", action="store_true", help="--gradclip: skip the environment tables")
    ap.add_argument("--duel", action="store_true",
                    help="also time two-player GridBoxing at G = E / 2 games against BoxingVec at E")
    ap.add_argument("--envs", type=int, nargs="+", default=[8192, 64])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--random", type=int, default=0)
    ap.add_argument("--game", choices=["breakout", "boxing"], default="breakout")
    ap.add_argument("--frame_skip", default="1")
    ap.add_argument("--sticky", type=float, default=0.0)
    ap.add_argument("--view", type=int, nargs="+", default=[])
    ap.add_argument("--duel_start", default=None, help="--duel: the start gap of the setting timed")
    ap.add_argument("--duel_only", action="store_true", help="--duel: skip the single-player tables")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs the GPU: a CPU run measures nothing"
    from ba3c_amd.actor_learner import SyntheticAtari
    from ba3c_amd.breakout import BreakoutVec
    from ba3c_amd.flags import GAMES, GRID_BOXING, GRID_BREAKOUT
    from ba3c_amd.frameskip import setting
    from ba3c_amd.rollout import FrameHistory
    skip = setting(args.frame_skip, args.sticky)          # (lo, hi, q16), None: off
    name = GRID_BOXING if args.game == "boxing" else GRID_BREAKOUT
    Vec, A = GAMES[name][:2]
    out = {"game": name, "iters": args.iters, "envs": {}}
    if skip is not None:
        out["frame_skip"], out["sticky_q16"] = list(skip[:2]), skip[2]

    # HBM copy rate: a device-to-device copy the size of E=8192 states (read + write)
    n = 8192 * STATE_BYTES
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    us = min(timed(lambda: dst.copy_(src), 50) for _ in range(args.repeats))
    out["copy_bytes"] = 2 * n
    out["copy_GBps"] = round(2 * n / us / 1e3, 1)
    # the same traffic over the fused kernel's own footprint: one buffer updated in place
    us = min(timed(lambda: src.add_(1), 50) for _ in range(args.repeats))
    out["inplace_GBps"] = round(2 * n / us / 1e3, 1)
    del src, dst
    if args.view:
        # the view only stores: a fill the size of its largest output (E = 8192, S = max) as yardstick
        fill = torch.empty(8192 * (104 * max(args.view)) * (252 * max(args.view)), dtype=torch.uint8, device="cuda")
        us = min(timed(lambda: fill.zero_(), 20, 3) for _ in range(args.repeats))
        out["fill_bytes"] = fill.numel()
        out["fill_GBps"] = round(fill.numel() / us / 1e3, 1)
        del fill

    for E in ([] if (args.duel and args.duel_only) or (args.ppo and args.ppo_only)
              or (args.episodes and args.episodes_only)
              or (args.gradclip and args.gradclip_only) else args.envs):
        g = torch.Generator(device="cuda").manual_seed(0)
        actions = torch.randint(0, A, (E,), generator=g, device="cuda")
        env, hist = Vec(E, seed=0), FrameHistory(E, 4, 1)
        env.reset_history(hist)
        if Vec is not BreakoutVec:                        # the yardstick: GridBreakout's fused step
            actions_b = torch.randint(0, 4, (E,), generator=g, device="cuda")
            env_b, hist_b = BreakoutVec(E, seed=0), FrameHistory(E, 4, 1)
            env_b.reset_history(hist_b)
        if skip is not None:
            env_k = Vec(E, seed=0, frame_skip=skip[:2], sticky=skip[2] / 65536.0)
            hist_k = FrameHistory(E, 4, 1)
            env_k.reset_history(hist_k)
        syn, hist_s = SyntheticAtari(E, 4, seed=0), FrameHistory(E, 4, 1)

        def synthetic():
            frames, _, over = syn.step(actions)
            hist_s.push(frames, over)
        # alternate them so that all see the same machine state
        fused, base, brk, skipped = [], [], [], []
        viewed = {S: [] for S in args.view}
        hud = torch.randint(0, 256, (E, 20), generator=g, device="cuda").to(torch.uint8)
        for _ in range(args.repeats):
            fused.append(timed(lambda: env.step_into(actions, hist), args.iters))
            for S in args.view:                           # fewer calls: an image is up to 64x a frame
                viewed[S].append(timed(lambda: env.view(scale=S, hud=hud), max(args.iters // 10, 10), 3))
            if skip is not None:
                skipped.append(timed(lambda: env_k.step_into(actions, hist_k), args.iters))
            if Vec is not BreakoutVec:
                brk.append(timed(lambda: env_b.step_into(actions_b, hist_b), args.iters))
            base.append(timed(synthetic, args.iters))
        traffic = 2 * E * STATE_BYTES                     # the history is read and written once
        out["envs"][str(E)] = {
            "fused_step_into_us": [round(v, 2) for v in fused],
            "synthetic_step_plus_push_us": [round(v, 2) for v in base],
            "state_bytes": traffic,
            "fused_GBps": round(traffic / min(fused) / 1e3, 1),
        }
        if skipped:
            mean_k = (skip[0] + skip[1]) / 2.0
            out["envs"][str(E)].update({
                "skip_decision_us": [round(v, 2) for v in skipped],
                "skip_game_step_us": [round(v / mean_k, 2) for v in skipped],
                "mean_k": mean_k,
                "skip_over_one_step": round(min(skipped) / min(fused), 3),
                "skip_over_k_one_steps": round(min(skipped) / (mean_k * min(fused)), 3),
            })
        for S, us in viewed.items():
            n_bytes = E * (104 * S) * (252 * S)
            out["envs"][str(E)]["view_S%d" % S] = {
                "us": [round(v, 2) for v in us], "out_bytes": n_bytes,
                "store_GBps": round(n_bytes / min(us) / 1e3, 1),
                "over_fused_step": round(min(us) / min(fused), 2)}
        if brk:
            out["envs"][str(E)]["breakout_fused_step_into_us"] = [round(v, 2) for v in brk]
            out["envs"][str(E)]["fused_over_breakout"] = round(min(fused) / min(brk), 3)
    if args.duel:
        from ba3c_amd.duel import FIXED_START, start_from_gap
        out["duel"] = duel_table(args.envs, args.iters, args.repeats)
        start = start_from_gap(args.duel_start or "8-14") or FIXED_START
        out["duel_decision"] = duel_decision_table(args.envs, args.iters, args.repeats,
                                                   skip or (2, 4, 16384), start)
    if args.returns:
        out["returns"] = returns_table(args.repeats)
        out["iterate"] = iterate_table([(5, 1.0), (20, 0.95), (5, 1.0), (20, 0.95)])
    if args.ppo:
        from ba3c_amd.ppo import Setting
        out["ppo_step"] = ppo_step_table(args.repeats, norm_adv=args.ppo_norm_adv, vclip=args.ppo_vclip)
        on = Setting(clip=0.2, epochs=4, minibatches=4)
        legs = [(5, 1.0), (5, 1.0, on)]
        if args.ppo_norm_adv or args.ppo_vclip:
            legs.append((5, 1.0, on._replace(norm_adv=args.ppo_norm_adv, vclip=args.ppo_vclip)))
        out["ppo_iterate"] = iterate_table(legs * 2)
    if args.episodes:
        out["episode_stats"] = episodes_table(args.repeats)
        out["episodes_iterate"] = episodes_iterate_table()
    if args.gradclip:
        out["gradclip"] = gradclip_table(args.repeats)
    if args.random:
        from ba3c_amd.evaluate import eval_with_envs, uniform_policy
        from ba3c_amd.model import Model
        m = Model(num_actions=A, fc_neurons=128, fc_splits=4, batch_size=32, max_batch=32, seed=0)
        torch.manual_seed(0)
        fs = dict(frame_skip=skip[:2], sticky=skip[2] / 65536.0) if skip is not None else {}
        mean, mx = eval_with_envs(m.engine, args.random, min(args.random, 20), seed=0,
                                  policy=uniform_policy(A), game=name, **fs)
        out["random_policy"] = {"episodes": args.random, "mean_score": mean, "max_score": mx}
        if args.game == "boxing":
            def noop(state):                              # argmax 0 = NOOP (FIRE every 30th step:
                p = torch.zeros(state.shape[0], A, dtype=torch.float32, device=state.device)
                p[:, 0] = 1.0                             # the evaluation's PreventStuckPlayer)
                return p
            mean, mx = eval_with_envs(m.engine, args.random, min(args.random, 20), seed=0,
                                      policy=noop, game=name, **fs)
            out["noop_policy"] = {"episodes": args.random, "mean_score": mean, "max_score": mx}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
