"""Environment step time on the GPU (GridBreakout / GridBoxing sections): µs per fused
`step_into` of the on-device game (--game breakout: `BreakoutVec`; --game boxing: `BoxingVec`,
timed next to GridBreakout's fused step in the same run) against `SyntheticAtari.step` +
`FrameHistory.push`, and the fused
kernel's achieved bytes/s against this box's measured HBM copy rate (a device-to-device copy, and
an in-place update over the kernel's own footprint).  With --random N also the
evaluation scores of a uniform-random policy (and, for boxing, of a NOOP policy) over N
episodes.  Prints one JSON line.

    python scripts/env_throughput.py [--game boxing] [--envs 8192 64] [--iters 200] [--random 20]
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[8192, 64])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--random", type=int, default=0)
    ap.add_argument("--game", choices=["breakout", "boxing"], default="breakout")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs the GPU: a CPU run measures nothing"
    from ba3c_amd.actor_learner import SyntheticAtari
    from ba3c_amd.breakout import BreakoutVec
    from ba3c_amd.flags import GAMES, GRID_BOXING, GRID_BREAKOUT
    from ba3c_amd.rollout import FrameHistory
    name = GRID_BOXING if args.game == "boxing" else GRID_BREAKOUT
    Vec, A = GAMES[name][:2]
    out = {"game": name, "iters": args.iters, "envs": {}}

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

    for E in args.envs:
        g = torch.Generator(device="cuda").manual_seed(0)
        actions = torch.randint(0, A, (E,), generator=g, device="cuda")
        env, hist = Vec(E, seed=0), FrameHistory(E, 4, 1)
        env.reset_history(hist)
        if Vec is not BreakoutVec:                        # the yardstick: GridBreakout's fused step
            actions_b = torch.randint(0, 4, (E,), generator=g, device="cuda")
            env_b, hist_b = BreakoutVec(E, seed=0), FrameHistory(E, 4, 1)
            env_b.reset_history(hist_b)
        syn, hist_s = SyntheticAtari(E, 4, seed=0), FrameHistory(E, 4, 1)

        def synthetic():
            frames, _, over = syn.step(actions)
            hist_s.push(frames, over)
        # alternate them so that all see the same machine state
        fused, base, brk = [], [], []
        for _ in range(args.repeats):
            fused.append(timed(lambda: env.step_into(actions, hist), args.iters))
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
        if brk:
            out["envs"][str(E)]["breakout_fused_step_into_us"] = [round(v, 2) for v in brk]
            out["envs"][str(E)]["fused_over_breakout"] = round(min(fused) / min(brk), 3)
    if args.random:
        from ba3c_amd.evaluate import eval_with_envs, uniform_policy
        from ba3c_amd.model import Model
        m = Model(num_actions=A, fc_neurons=128, fc_splits=4, batch_size=32, max_batch=32, seed=0)
        torch.manual_seed(0)
        mean, mx = eval_with_envs(m.engine, args.random, min(args.random, 20), seed=0,
                                  policy=uniform_policy(A), game=name)
        out["random_policy"] = {"episodes": args.random, "mean_score": mean, "max_score": mx}
        if args.game == "boxing":
            def noop(state):                              # argmax 0 = NOOP (FIRE every 30th step:
                p = torch.zeros(state.shape[0], A, dtype=torch.float32, device=state.device)
                p[:, 0] = 1.0                             # the evaluation's PreventStuckPlayer)
                return p
            mean, mx = eval_with_envs(m.engine, args.random, min(args.random, 20), seed=0,
                                      policy=noop, game=name)
            out["noop_policy"] = {"episodes": args.random, "mean_score": mean, "max_score": mx}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
