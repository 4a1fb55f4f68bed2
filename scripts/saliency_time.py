"""conv0's input gradient: ms per ba3c_conv0_input_grad call (prep launch +
kernel) on the dp0 a training pass left at B = 1, 32 and 2048 — HIP events around batches of
calls after warm-up, five rounds, without and with the map output — its fraction of the fp16x3
path peak priced on the algorithmic 45.16 MFLOP per image, and conv1's input gradient at the same
batch (the BA3C_K_CONV1_DGRAD probe inside train_grads; at small batches that kernel shares a
launch the probe does not bracket: 0 launches).  One JSON line per batch.
    python scripts/saliency_time.py
--perturb times perturbation saliency instead at B = 1 and 32: ms per
Ba3cEngine.perturb_maps call (289 B forwards in chunks of max_batch = 2048) and per launch of
ba3c_perturb_states (all 289 B states at once, with its store rate) and of ba3c_perturb_scores, the
same way: HIP events around batches of calls after warm-up, five rounds, sorted.
    python scripts/saliency_time.py --perturb
--intgrad times integrated gradients at B = 1 and 32, max_batch = 2048: ms per
Ba3cEngine.integrated_grads call at K = 8, 32 and 128 ("blur"), beside one input_grads call and one
perturb_maps call on the same states, ms per launch of ba3c_ig_states (all B K path states at once,
with its store rate) and of ba3c_ig_accumulate at K = 32, and the completeness gap
|sum(attr) - (V(x) - V(x0))| of the value at each K, as [median, largest] over the states of its
ratio to |V(x) - V(x0)| and to sum |attr|: on the timed states (uniform noise) and, at B = 32, on
tests/atari_frames.py's drawn Breakout frames.
    python scripts/saliency_time.py --intgrad"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-ba3c_amd")]
from ba3c_amd.engine import Ba3cEngine
from oracle import ba3c_oracle as O



def rounds_ms(fn, reps, warm=10):
    """Sorted ms per call of five rounds of `reps` calls between HIP events, after `warm` calls."""
    for _ in range(warm):
        fn()
    rounds = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / reps)
    return sorted(rounds)


def perturb_times():
    from ba3c_amd import _lib as L
    from ba3c_amd.perturb import NC
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for B in (1, 32):
        eng = Ba3cEngine(num_actions=18, fc_neurons=128, fc_splits=4, max_batch=2048)
        eng.load_params(O.init_params(128, 4, 18, seed=7, dtype=np.float32))
        st = torch.from_numpy(np.random.RandomState(B).randint(0, 256, size=(B, 84, 84, 4)).astype(np.uint8)).cuda()
        N = B * NC
        out = torch.empty(N, 84, 84, 4, dtype=torch.uint8, device="cuda")
        p0, v0, p, v = (torch.rand(*s, device="cuda") for s in ((B, 18), (B,), (N, 18), (N,)))
        mp = torch.empty(B, 84, 84, device="cuda")
        res = {"perturb_maps_v_ms": rounds_ms(lambda: eng.perturb_maps(st, "v"), 20, 3),
               "perturb_maps_pi_newest_ms": rounds_ms(lambda: eng.perturb_maps(st, "pi", newest=True), 20, 3)}
        for newest in (0, 1):
            res["states_newest%d_ms" % newest] = rounds_ms(lambda: L.check(eng.lib.ba3c_perturb_states(
                None, ptr(st), B, 0, N, newest, ptr(out))), 50)
        for which in (0, 1):
            res["scores_which%d_ms" % which] = rounds_ms(lambda: L.check(eng.lib.ba3c_perturb_scores(
                None, ptr(p0), ptr(v0), ptr(p), ptr(v), B, 18, which, ptr(mp), None)), 200)
        res["states_store_GBps"] = N * 28224 / (res["states_newest0_ms"][2] * 1e-3) / 1e9
        print(B, json.dumps(res), flush=True)
        del eng


def intgrad_times():
    from ba3c_amd import _lib as L
    from ba3c_amd import intgrad as IG
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for B in (1, 32):
        eng = Ba3cEngine(num_actions=18, fc_neurons=128, fc_splits=4, max_batch=2048)
        eng.load_params(O.init_params(128, 4, 18, seed=7, dtype=np.float32))
        host = np.random.RandomState(B).randint(0, 256, size=(B, 84, 84, 4)).astype(np.uint8)
        st = torch.from_numpy(host).cuda()
        ac = torch.zeros(B, dtype=torch.int64, device="cuda")
        seeds = torch.tensor([0.0, 1.0], device="cuda").repeat(B, 1)

        def gaps(frames, K):
            x, x0 = (torch.from_numpy(a).cuda() for a in (frames, IG.baseline_numpy(frames, "blur")))
            v = eng.forward(x)[2].double() - eng.forward(x0)[2].double()
            attr = eng.integrated_grads(x, ac, seeds, steps=K).double()
            gap = (attr.sum(dim=(1, 2, 3)) - v).abs()
            return [[float(r.median()), float(r.max())] for r in (gap / v.abs(), gap / attr.abs().sum(dim=(1, 2, 3)))]
        res = {"input_grads_ms": rounds_ms(lambda: eng.input_grads(st, ac, seeds), 50),
               "perturb_maps_v_ms": rounds_ms(lambda: eng.perturb_maps(st, "v"), 20, 3)}
        for K in (8, 32, 128):
            res["integrated_grads_K%d_ms" % K] = rounds_ms(lambda: eng.integrated_grads(st, ac, seeds, steps=K), 20, 3)
            res["gap_noise_K%d" % K] = gaps(host, K)
            if B == 32:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from atari_frames import atari_frames
                res["gap_drawn_K%d" % K] = gaps(atari_frames(B, 5), K)
        N = B * 32
        out = torch.empty(N, 84, 84, 4, dtype=torch.uint8, device="cuda")
        g = torch.rand(N, 84, 84, 4, device="cuda")
        acc = torch.zeros(B, 84, 84, 4, dtype=torch.float64, device="cuda")
        attr = torch.empty(B, 84, 84, 4, device="cuda")
        for base in (0, 1):
            res["states_baseline%d_ms" % base] = rounds_ms(lambda: L.check(eng.lib.ba3c_ig_states(
                None, ptr(st), B, 32, base, 0, N, ptr(out))), 50)
            res["accumulate_baseline%d_ms" % base] = rounds_ms(lambda: L.check(eng.lib.ba3c_ig_accumulate(
                None, ptr(st), B, 32, base, 0, N, ptr(g), ptr(acc), ptr(attr))), 50)
        res["states_store_GBps"] = N * 28224 / (res["states_baseline1_ms"][2] * 1e-3) / 1e9
        res["accumulate_read_GBps"] = N * 28224 * 4 / (res["accumulate_baseline1_ms"][2] * 1e-3) / 1e9
        print(B, json.dumps(res), flush=True)
        del eng


if "--intgrad" in sys.argv[1:]:
    intgrad_times()
    sys.exit(0)

if "--perturb" in sys.argv[1:]:
    perturb_times()
    sys.exit(0)

PEAK = 838.9e12                      # fp16x3 path, fp32-equivalent
FLOP = 2 * 7056 * 4 * 800            # algorithmic, per image
out = {}
for B, F, S in ((1, 128, 4), (32, 128, 4), (2048, 512, 1)):
    rs = np.random.RandomState(B)
    eng = Ba3cEngine(num_actions=4, fc_neurons=F, fc_splits=S, max_batch=B)
    eng.load_params(O.init_params(F, S, 4, seed=7, dtype=np.float32))
    st = torch.from_numpy(rs.randint(0, 256, size=(B, 84, 84, 4)).astype(np.uint8)).cuda()
    ac = torch.from_numpy(rs.randint(0, 4, size=B).astype(np.int64)).cuda()
    R = torch.from_numpy(rs.normal(size=B).astype(np.float32)).cuda()
    eng.probe_enable("conv1_dgrad")
    for _ in range(30):
        eng.train_grads(st, ac, R)
    torch.cuda.synchronize()
    eng.probe_read()
    for _ in range(50):
        eng.train_grads(st, ac, R)
    ms1, n1 = eng.probe_read()
    merged = eng.kernel_merged("conv1_dgrad")
    eng.probe_enable(None)
    dx = torch.empty(B, 84, 84, 4, device="cuda")
    mp = torch.empty(B, 84, 84, device="cuda")
    reps = 200 if B < 2048 else 40
    res = {}
    for name, m in (("dx", None), ("dx+map", mp)):
        for _ in range(20):
            eng.conv0_input_grad(B, out=dx, map=m)
        rounds = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                eng.conv0_input_grad(B, out=dx, map=m)
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) / reps)
        res[name] = sorted(rounds)
    med = res["dx"][2]
    out[B] = dict(conv0d_ms=res, frac_fp16x3_peak=B * FLOP / (med * 1e-3) / PEAK,
                  conv1_dgrad_ms=ms1 / max(n1, 1), conv1_dgrad_launches=n1, conv1_dgrad_merged=merged)
    print(B, json.dumps(out[B]), flush=True)
    del eng
