"""`python -m ba3c_amd.train` — the single-node launcher on the reference's flag surface
(run_job.py:13-148 -> distributed_tensorpack_mkl.sh -> OpenAIGym/train.py:649-724, get_config
:505-638).  What it builds, per flag group:

- model geometry and `-b`: the Model (train.py:517).
- `-o` and its hyper-parameters: the optimizer (:582-597).
- `--use_sync -g N`: SyncReplicasOptimizer (:598-606), here an RCCL all-reduce over the node's GPUs.
- `-e`, `--simulator_procs`: the actor-learner loop (simulator master + predictor + BatchData,
  :520-534) on the synthetic on-device environment or on a game of flags.GAMES.
- `--frame_skip` / `--sticky`: ALE's frame skip and sticky actions, for training and evaluation.
- `--self_play`, `--duel_frame_skip` / `--duel_sticky` / `--duel_start`: two-player GridBoxing
  (ba3c_amd.duel), both sides played by the learner.
- `--local_time_max` / `--gamma` / `--gae_lambda`: the returns' rollout length, discount and GAE
  lambda (ba3c_amd.returns).
- `--ppo_clip` and the other `--ppo_*`: the clipped-surrogate loss over replayed pools (ba3c_amd.ppo).
- `--max_grad_norm`: the clip of the whole gradient's norm (ba3c_amd.gradclip) in place of the
  reference's per-tensor clip; `--entropy_beta`, `--lr_schedule` / `--entropy_schedule`: the entropy
  coefficient and the two schedules (ba3c_amd.schedule).
- `--online_score N`: the training simulators' own episodes, logged on the device (ba3c_amd.episodes).
- `--nr_eval N`: the Evaluator callback every --steps_per_epoch steps.
- `--send_debug_every`, `--experiment_dir`: DebugLogCallback's metrics channels (ba3c_amd.metrics).
- `--save_every`, `--models_dir`, `--load`: PeriodicPerStepCallback(ModelSaver) (:608-630) and
  SaverRestore (:706-707).

One process per GPU: launch N > 1 with
    torchrun --nproc-per-node N --master-addr 127.0.0.1 -m ba3c_amd.train --use_sync -g N ...
The process group ('nccl' = RCCL) is created before any other GPU work.  Each rank seeds its
numpy stream with its worker index (train.py:678-679); variables start identical on every
rank (rank 0's are broadcast).
"""
import json
import os
import socket
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

from .flags import GAMES, build_parser, resolve


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def model_config(args):
    """The Model / engine geometry the flags select (train.py:95, :216-243)."""
    return dict(num_actions=args.num_actions, channels=args.channels, fc_neurons=args.fc_neurons,
                fc_splits=args.fc_splits, replace_with_conv=bool(args.replace_with_conv),
                ps=args.ps, batch_size=args.batch_size)


def optimizer_config(args):
    """`-o` and its hyper-parameters (train.py:582-597)."""
    return dict(name=args.optimizer, lr=args.lr, beta1=args.beta1, beta2=args.beta2,
                epsilon=args.epsilon)


def check_distributed(args, world):
    """Synchronous data parallelism only (the asynchronous PS mode has no all-reduce
    equivalent): --use_sync with 1 <= --ngrads <= world size.  --ngrads below the world size
    keeps the reference's backup workers (train.py:601-602): each step averages the first
    `ngrads` ranks' gradients and drops the rest as stale (SyncReplicasOptimizer)."""
    if world > 1 and not args.use_sync:
        raise SystemExit("world size %d: multi-GPU training is synchronous (RCCL all-reduce); "
                         "pass --use_sync -g %d" % (world, world))
    if args.use_sync and not 1 <= args.ngrads <= world:
        raise SystemExit("--ngrads %d must be in [1, %d] (the number of GPU processes)"
                         % (args.ngrads, world))
    if world > 1 and args.ppo is not None and args.ppo.target_kl > 0:
        raise SystemExit("--ppo_target_kl with world size %d: replicas that stop at different "
                         "epochs would leave the all-reduce unmatched; it is single-replica" % world)


def build(args, rank=0, world=1, device=None):
    """Model + optimizer + trainer + actor-learner loop (+ callbacks) for this rank."""
    from .checkpoint import ModelSaver, PeriodicPerStepCallback, SaverRestore
    from .model import Model
    from .optimizer import SyncReplicasOptimizer, make_optimizer
    from .trainer import Ba3cTrainer, TrainConfig

    mc = model_config(args)
    seed = rank if args.seed is None else args.seed
    model = Model(conv_init=args.conv_init, fc_init=args.fc_init, seed=seed,
                  max_batch=max(args.batch_size, args.simulator_procs),
                  max_grad_norm=args.max_grad_norm, **mc)
    model.entropy_beta = args.entropy_beta
    oc = optimizer_config(args)
    opt = make_optimizer(oc["name"], oc["lr"], beta1=oc["beta1"], beta2=oc["beta2"],
                         epsilon=oc["epsilon"])
    if args.use_sync:
        opt = SyncReplicasOptimizer(opt, replicas_to_aggregate=args.ngrads, total_num_replicas=world)
    trainer = Ba3cTrainer(TrainConfig(model=model, optimizer=opt, step_per_epoch=args.steps_per_epoch,
                                      max_epoch=args.max_epoch))
    trainer.schedules = args.schedules
    if args.load:
        SaverRestore(args.load).init(trainer)
        if isinstance(opt, SyncReplicasOptimizer):
            opt.broadcast_variables(trainer.engine)
    savers = []
    if args.save_every and rank == 0:
        savers.append(PeriodicPerStepCallback(ModelSaver(args.models_dir), args.save_every))
    return model, trainer, savers


def main(argv=None):
    args = resolve(build_parser().parse_args(argv))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    check_distributed(args, world)
    torch.cuda.set_device(local)
    own_group = False
    if args.use_sync and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        dist.init_process_group("nccl", rank=rank, world_size=world,
                                device_id=torch.device("cuda", local))
        own_group = True
    try:
        return _run(args, rank, world)
    finally:
        if own_group:
            dist.destroy_process_group()


def _run(args, rank, world):
    from .actor_learner import ActorLearner
    from .metrics import CsvChannels, GradClipMetrics, PpoMetrics, ScheduleMetrics, StepMetrics
    np.random.seed(rank)                                      # train.py:679
    model, trainer, savers = build(args, rank, world)
    client = CsvChannels(args.experiment_dir) if rank == 0 else None

    evaluator = None
    if args.nr_eval and rank == 0:
        from .evaluate import Evaluator
        evaluator = Evaluator(trainer.engine, args.nr_eval, client, seed=1000 + rank,
                              game=args.environment, frame_skip=args.play_frame_skip,
                              sticky=args.play_sticky)

    def on_step(tr):
        metrics(tr)                                           # built below, before the first step
        for cb in savers:
            cb.trigger_step(tr)
        if evaluator is not None and tr.global_step % args.steps_per_epoch == 0:
            evaluator()                                       # Evaluator._trigger_epoch

    max_steps = args.max_steps or args.steps_per_epoch * args.max_epoch
    t0 = time.time()
    al = log = None
    if not args.dummy:
        env = None
        if args.online_score:
            from .episodes import EpisodeLog, EpisodeMetrics
            log = EpisodeLog(args.simulator_procs, device=trainer.engine.device)
        if args.self_play:
            # --simulator_procs players in half as many two-player games; both sides learn
            from .duel import BoxingDuelDecisionVec, start_from_gap
            env = BoxingDuelDecisionVec(args.simulator_procs // 2, seed=rank, device=trainer.engine.device,
                                        frame_skip=args.play_frame_skip, sticky=args.play_sticky,
                                        start=start_from_gap(args.duel_start))
        elif args.environment in GAMES:
            env = GAMES[args.environment][0](args.simulator_procs, seed=rank,
                                             device=trainer.engine.device,
                                             frame_skip=args.frame_skip, sticky=args.sticky)
        al = ActorLearner(trainer, n_envs=args.simulator_procs, batch_size=args.batch_size,
                          seed=rank, rs=np.random.RandomState(rank), on_train_step=on_step,
                          dummy_predictor=bool(args.dummy_predictor), env=env,
                          local_time_max=args.local_time_max, gamma=args.gamma,
                          gae_lambda=args.gae_lambda, ppo=args.ppo, stop_at=max_steps, episodes=log)
    pool_trainer = al.pool_trainer if al is not None else None
    metrics = StepMetrics(trainer, args.batch_size, args.send_debug_every, client,
                          ppo=PpoMetrics(args.ppo.clip, pool_trainer, client) if pool_trainer else None,
                          episodes=EpisodeMetrics(log, args.online_score, client) if log is not None else None,
                          gradclip=(GradClipMetrics(model.get_gradient_processor()[0], client)
                                    if args.max_grad_norm else None),
                          schedule=ScheduleMetrics(client) if args.log_schedule else None)
    if al is None:
        # --dummy 1: a constant synthetic batch, no simulators (train/multigpu.py:70-75)
        dev = trainer.engine.device
        B = args.batch_size
        state = torch.ones(B, 84, 84, trainer.engine.channels, dtype=torch.uint8, device=dev)
        action = torch.zeros(B, dtype=torch.int64, device=dev)
        R = torch.zeros(B, dtype=torch.float32, device=dev)
        while trainer.global_step < max_steps:
            trainer.train_step(state, action, R)
            on_step(trainer)
        sim_steps = 0
    else:
        while trainer.global_step < max_steps:
            al.iterate()
        sim_steps = al.steps
    metrics.flush()
    if metrics.episodes is not None:
        metrics.episodes.flush()                              # what finished after the last fetch
    torch.cuda.synchronize()
    wall = time.time() - t0
    if client is not None:
        client.close()
    out = {"rank": rank, "world": world, "global_step": trainer.global_step,
           "simulator_steps": sim_steps, "samples_per_s": round(
               trainer.global_step * args.batch_size * world / max(wall, 1e-9), 1),
           "last": metrics.last}
    if args.ppo is not None:
        out["ppo"] = dict(args.ppo._asdict(), **(metrics.last_ppo or {}))
    if metrics.episodes is not None:
        out["episodes"] = metrics.episodes.as_dict()
    if metrics.gradclip is not None:
        out["grad_clip"] = metrics.gradclip.last or {"max_norm": args.max_grad_norm}
    if metrics.schedule is not None:
        out["schedule"] = metrics.schedule.last
    if evaluator is not None:
        out["eval"] = evaluator.history
    if rank == 0:
        print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
