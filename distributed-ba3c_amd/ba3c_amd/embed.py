"""Embed the states a policy meets: a two-dimensional t-SNE of the last hidden layer, coloured by
the value (Mnih et al. 2015, Fig. 4).  Episodes are played along the evaluation's decision path
(record.open_players, so the states are those an evaluation or a recording with the same arguments
meets), every K-th decision's state is kept until there are N, `Ba3cEngine.features` gives their
fc1 activations and `tsne.embed` the map, all on the device.

    python -m ba3c_amd.embed --load CKPT -e GridBoxing-v0 --num_actions 18 --fc_neurons 128 \\
        --fc_splits 4 --states 2048 --every 4 --perplexity 30 --iters 1000 --out boxing_tsne.npz
    python -m ba3c_amd.embed --random -e GridBreakout-v0 --states 512 --out random_tsne.npz
    python -m ba3c_amd.embed --random -e GridBreakout-v0 --states 512 --method pca --out random_pca.npz

--init pca starts the map from the first two principal-component scores (ba3c_amd/pca.py) instead
of the seed's draw; --method pca writes those two scores as y and runs no t-SNE.

The .npz holds y float32 [N, 2], value float32 [N], action int64 [N], episode and step int64 [N]
(the simulator's running episode count and the decision within it) and kl float64 (tsne.embed's
trace); where PCA ran also explained float64 [2] (the explained-variance ratios) and pca_resid.
With PIL a scatter of y coloured by value (blue low, red high) is written next to it as
.png; without PIL only the .npz.
"""
import json
import os

import numpy as np

from . import pca, tsne
from .breakout import DEFAULT_LIMIT
from .flags import ALL_GAMES, build_parser, resolve


def collect_states(engine, game, n_states, every=1, n_envs=None, seed=0, limit=DEFAULT_LIMIT, frame_skip=1,
                   sticky=0.0, policy=None):
    """Play until `n_states` states are kept: every `every`-th decision of each simulator.
    -> (state uint8 device [N,84,84,4], action int64 [N], episode int64 [N], step int64 [N])."""
    import torch

    from .record import open_players
    n_envs = int(n_envs) if n_envs else max(1, min(20, engine.max_batch))
    assert n_states >= 1 and every >= 1
    env, hist, players = open_players(engine, game, n_envs, seed, limit, frame_skip, sticky, policy)
    episode, step = np.zeros(n_envs, np.int64), np.zeros(n_envs, np.int64)
    states, meta = [], []

    def before_step(probs, value, act):
        keep = np.nonzero(step % every == 0)[0]
        if keep.size:
            states.append(hist.state[torch.from_numpy(keep).to(engine.device)].clone())
            meta.append(np.stack([act.cpu().numpy()[keep], episode[keep], step[keep]], axis=1))

    while sum(s.shape[0] for s in states) < n_states:
        _, over = players.step(env, hist, before_step)
        over = over.cpu().numpy().astype(bool)
        step[:] = np.where(over, 0, step + 1)
        episode += over
    meta = np.concatenate(meta)[:n_states]
    return torch.cat(states)[:n_states].contiguous(), meta[:, 0], meta[:, 1], meta[:, 2]


def embed_states(engine, state, perplexity=30, iters=1000, seed=0, init="random", method="tsne"):
    """-> dict of y, value and kl for `state` (uint8 device [N,84,84,4]); where PCA ran (init
    "pca" or method "pca": y is then the two scores and no t-SNE runs) also explained (the two
    explained-variance ratios) and pca_resid."""
    import torch
    feats = engine.features(state)
    value = torch.cat([engine.forward(state[i:i + engine.max_batch])[2].clone()
                       for i in range(0, state.shape[0], engine.max_batch)])
    fit = {}
    if method == "pca":
        fit = pca.fit(feats.contiguous(), min(2, feats.shape[1]), seed=seed)
        y, kl = torch.nn.functional.pad(fit["scores"], (0, 2 - fit["scores"].shape[1])), np.zeros(0)
    else:
        y, kl = tsne.embed(feats, perplexity=perplexity, iters=iters, seed=seed, init=init, pca_out=fit)
    out = {"y": y.cpu().numpy(), "value": value.cpu().numpy(), "kl": kl}
    if fit:
        out.update(explained=fit["ratio"].cpu().numpy(), pca_resid=fit["resid"].cpu().numpy())
        if out["pca_resid"].max() > pca.RESID_WARN:
            print("warning: PCA residual %.3g exceeds %g: more sweeps are needed" %
                  (out["pca_resid"].max(), pca.RESID_WARN), flush=True)
    return out


def scatter_png(path, y, value, size=512, dot=2):
    """Write the scatter with PIL.  -> False (and nothing written) where PIL is missing."""
    try:
        from PIL import Image
    except ImportError:
        return False
    img = np.full((size, size, 3), 255, np.uint8)
    span = np.maximum(y.max(axis=0) - y.min(axis=0), 1e-30)
    xy = ((y - y.min(axis=0)) / span * (size - 2 * dot - 1)).astype(np.int64) + dot
    t = (value - value.min()) / max(float(value.max() - value.min()), 1e-30)
    rgb = np.stack([255 * t, 64 * np.ones_like(t), 255 * (1 - t)], axis=1).astype(np.uint8)
    for (x, yy), c in zip(xy, rgb):
        img[size - 1 - yy - dot:size - yy + dot, x - dot:x + dot + 1] = c
    Image.fromarray(img).save(path)
    return True


def embed_parser():
    p = build_parser()
    p.description = "t-SNE of the fc1 features of the states a policy meets in an on-device game"
    p.add_argument("--states", type=int, default=2048, help="N, in [8, 8192]")
    p.add_argument("--every", type=int, default=4, help="keep every K-th decision's state")
    p.add_argument("--perplexity", type=float, default=30.0)
    p.add_argument("--iters", type=int, default=1000)
    p.add_argument("--out", default="tsne.npz")
    p.add_argument("--random", action="store_true", help="a uniform-random policy: no --load needed")
    p.add_argument("--limit", type=int, default=DEFAULT_LIMIT, help="LimitLengthPlayer's game steps")
    p.add_argument("--init", choices=("random", "pca"), default="random",
                   help="t-SNE's start: the seed's draw, or the first two principal-component scores")
    p.add_argument("--method", choices=("tsne", "pca"), default="tsne",
                   help="pca: y is the two leading principal-component scores and no t-SNE runs")
    return p


def main(argv=None):
    args = resolve(embed_parser().parse_args(argv))
    if args.environment not in ALL_GAMES:
        raise SystemExit("embedding needs an on-device game: pass -e %s" % " or -e ".join(sorted(ALL_GAMES)))
    if not args.random and not args.load:
        raise SystemExit("pass --load CHECKPOINT, or --random for a uniform-random policy")
    if not tsne.MIN_N <= args.states <= tsne.MAX_N or not 1 <= args.perplexity <= (args.states - 1) / 3.0:
        raise SystemExit("--states must be in [8, 8192] and --perplexity in [1, (states - 1) / 3]")
    from .evaluate import uniform_policy
    from .train import build
    model, _, _ = build(args)
    seed = 0 if args.seed is None else args.seed
    policy = uniform_policy(args.num_actions) if args.random else None
    state, action, episode, step = collect_states(model.engine, args.environment, args.states, args.every,
                                                  seed=seed, limit=args.limit, frame_skip=args.frame_skip,
                                                  sticky=args.sticky, policy=policy)
    out = embed_states(model.engine, state, args.perplexity, args.iters, seed, args.init, args.method)
    out.update(action=action, episode=episode, step=step)
    d = os.path.dirname(args.out)
    if d:
        os.makedirs(d, exist_ok=True)
    np.savez_compressed(args.out, **out)
    files = [args.out]
    png = os.path.splitext(args.out)[0] + ".png"
    if scatter_png(png, out["y"], out["value"]):
        files.append(png)
    else:
        print("PIL is not installed: no scatter image, only %s" % args.out, flush=True)
    res = {"game": args.environment, "states": int(state.shape[0]), "kl": float(out["kl"][-1]) if len(out["kl"]) else None,
           "files": files}
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
