"""The t-SNE path: ms per ba3c_tsne_sqdist (pre-pass + Gram), per
ba3c_tsne_affinities (bisection + symmetrisation) and per ba3c_tsne_step (the pair of launches of
an iteration, without and with the KL) at N = 1024, 4096 and 8192 for D = 128 and 512 (the
iteration does not see D and is timed once per N).  HIP events around 20 calls after 5 warm-up
calls, five rounds: [median, fastest, slowest].  The iteration's one N^2 stream is P: its read rate
is N^2 * 4 bytes over the step's median.  A 64 MB P (N = 4096) fits the 256 MB last-level cache, so
its rate is not an HBM rate; the 256 MB P of N = 8192 does not fit.  One JSON line per (N, D).
--pca times the PCA path at the same N and D instead: ba3c_pca_scatter (its
four launches, next to sqdist), one sweep (ba3c_pca_components at 2 sweeps minus at 1 sweep, per
statistic), the Ritz step (the rest of the 1-sweep call: Q0's orthonormalisation, the last multiply
and pca_ritz_kernel) and ba3c_pca_project (its three launches).
    python scripts/tsne_time.py [--pca]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-ba3c_amd")]
from ba3c_amd import pca as P
from ba3c_amd import tsne as T


def rounds_ms(fn, reps=20, warm=5):
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
    rounds.sort()
    return [rounds[2], rounds[0], rounds[4]]


for n in (1024, 4096, 8192):
    for d in (128, 512):
        rs = np.random.RandomState(n + d)
        x = rs.normal(size=(n, d)).astype(np.float32)
        x[:, 0] += 10.0 * (np.arange(n) % 8)
        x = torch.from_numpy(x).cuda()
        work = T._workspace(n, d)
        res = {"n": n, "d": d, "sqdist_ms": rounds_ms(lambda: T.sqdist(x, work))}
        if "--pca" in sys.argv[1:]:
            work = P._workspace(n, d)
            res["scatter_ms"] = rounds_ms(lambda: P.scatter(x, work))
            c = P.scatter(x, work)
            q0 = torch.from_numpy(P.q0_numpy(d)).cuda()
            one, two = (rounds_ms(lambda: P.components(c, 2, sw, q0=q0, work=work)) for sw in (1, 2))
            res["sweep_ms"] = [b - a for a, b in zip(one, two)]
            res["ritz_ms"] = [a - s for a, s in zip(one, res["sweep_ms"])]
            comps, eig, _, resid = P.components(c, 2, 32, work=work)
            res["project_ms"] = rounds_ms(lambda: P.project(x, comps, eig, None, work))
            res["resid_32_sweeps"] = resid.cpu().numpy().tolist()
            print(json.dumps(res), flush=True)
            continue
        dist = T.sqdist(x, work)
        res["affinities_ms"] = rounds_ms(lambda: T.affinities(dist, 30, work))
        if d == 128:
            p, _ = T.affinities(dist, 30, work)
            y, vel, gains = (torch.from_numpy(v).cuda() for v in T.initial_numpy(n, 0))
            kl = torch.zeros(1, dtype=torch.float64, device="cuda")
            res["step_ms"] = rounds_ms(lambda: T.step(p, y, vel, gains, 12.0, 0.5, 200.0, work))
            res["step_kl_ms"] = rounds_ms(lambda: T.step(p, y, vel, gains, 12.0, 0.5, 200.0, work, kl))
            res["p_read_GBps"] = n * n * 4 / (res["step_ms"][0] * 1e-3) / 1e9
            res["p_MB"] = n * n * 4 / 2 ** 20
            assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(kl).all())
        print(json.dumps(res), flush=True)
