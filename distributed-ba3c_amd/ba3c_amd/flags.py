"""The reference's flag surface for this path: run_job.py:13-48 (user CLI) and
OpenAIGym/parse.py:9-70 (worker flags), reduced to what the learner/predictor hot path and
its single-node launcher (`python -m ba3c_amd.train`) consume.  Slurm / TF-server / Neptune
flags are accepted and ignored."""
import argparse
import math

from . import duel, frameskip, ppo, schedule
from .boxing import BoxingVec
from .breakout import BreakoutVec

GRID_BREAKOUT = "GridBreakout-v0"
GRID_BOXING = "GridBoxing-v0"
# -e name -> (vector class, the game's number of actions, envs.get_player's game key)
GAMES = {GRID_BREAKOUT: (BreakoutVec, 4, "breakout"), GRID_BOXING: (BoxingVec, 18, "boxing")}
MAX_LOCAL_TIME = 128                  # ba3c_lambda_returns holds local_time_max + 1 <= 129 ring slots
STATE_BYTES = 84 * 84 * 4             # one stacked state of the rollout ring
MAX_RING_BYTES = 16 * 2 ** 30         # simulator_procs x (local_time_max + 1) states
DEFAULT_ENTROPY_BETA = 0.01           # Model.entropy_beta (train.py:296-297)


def string_to_bool(s):        # parse.py:5-6
    return str(s).lower() == "true"


def frame_skip_arg(s):
    """--frame_skip K -> K, --frame_skip LO-HI -> (LO, HI); the range is checked by resolve."""
    try:
        lo, hi = frameskip.parse_skip(str(s))
    except ValueError:
        raise argparse.ArgumentTypeError("expected K or LO-HI, got %r" % s)
    return lo if "-" not in str(s) else (lo, hi)


def duel_start_arg(s):
    """--duel_start GAP -> (GAP, GAP), --duel_start LO-HI -> (LO, HI); the range is checked by resolve."""
    try:
        return duel.parse_gap(s)
    except ValueError:
        raise argparse.ArgumentTypeError("expected GAP or LO-HI, got %r" % s)


def build_parser():
    p = argparse.ArgumentParser(description="BA3C learner/predictor on MI355X")
    # run_job.py flags
    p.add_argument("--batch_size", "-b", type=int, default=128)
    p.add_argument("--optimizer", "-o", default="adam",
                   choices=["adam", "gd", "adagrad", "adadelta", "momentum", "rms"])
    p.add_argument("--lr", "-l", "--learning_rate", dest="lr", type=float, default=0.00015)
    p.add_argument("--fc_neurons", type=int, default=256)
    p.add_argument("--fc_splits", type=int, default=1)
    p.add_argument("--use_normal_fc", action="store_true")
    p.add_argument("--replace_with_conv", type=string_to_bool, default=None)
    p.add_argument("--ps", type=int, default=1)
    p.add_argument("--use_sync", action="store_true")
    p.add_argument("--ngrads", "-g", "--num_grad", dest="ngrads", type=int, default=None)
    p.add_argument("--epsilon", type=float, default=1e-8)
    p.add_argument("--beta1", type=float, default=0.9)
    p.add_argument("--beta2", type=float, default=0.999)
    p.add_argument("--adam_debug", action="store_true")
    p.add_argument("--environment", "-e", "--env", dest="environment", default="Breakout-v0",
                   help="GridBreakout-v0 / GridBoxing-v0: the on-device Breakout / Boxing "
                        "(ba3c_amd.breakout, ba3c_amd.boxing); any other name: the synthetic "
                        "environment")
    p.add_argument("--channels", type=int, default=1)
    p.add_argument("--num_actions", type=int, default=4)
    p.add_argument("--predict_batch_size", type=int, default=16)
    p.add_argument("--conv_init", default="normal", choices=["normal", "uniform", "xavier"])
    p.add_argument("--fc_init", default="uniform", choices=["normal", "uniform"])
    p.add_argument("--simulator_procs", type=int, default=100)
    p.add_argument("--save_every", type=int, default=0)
    # parse.py worker flags of the training loop
    p.add_argument("--load", default=None)
    p.add_argument("--max_steps", type=int, default=None)
    p.add_argument("--steps_per_epoch", type=int, default=250)
    p.add_argument("--max_epoch", type=int, default=1000)
    p.add_argument("--send_debug_every", type=int, default=100)
    p.add_argument("--nr_eval", type=int, default=0,
                   help="episodes the Evaluator plays every --steps_per_epoch learner steps on "
                        "rank 0 (0: off; needs -e GridBreakout-v0 or GridBoxing-v0)")
    p.add_argument("--frame_skip", type=frame_skip_arg, default=1,
                   help="game steps per policy decision: K, or LO-HI for a uniform draw per "
                        "decision (ALE's -v0: 2-4); 1 <= LO <= HI <= 16; needs an on-device game")
    p.add_argument("--sticky", type=float, default=0.0,
                   help="probability that a game step repeats the previous step's action "
                        "(ALE's repeat_action_probability: 0.25); needs an on-device game")
    p.add_argument("--self_play", action="store_true",
                   help="train -e GridBoxing-v0 by self-play: --simulator_procs players (an even "
                        "number) in --simulator_procs / 2 two-player games (ba3c_amd.duel); "
                        "--nr_eval still plays the scripted opponent")
    p.add_argument("--duel_frame_skip", type=frame_skip_arg, default=1,
                   help="--self_play's --frame_skip: game steps per decision of the two-player "
                        "games, K or LO-HI (--nr_eval then plays the scripted opponent under it too)")
    p.add_argument("--duel_sticky", type=float, default=0.0,
                   help="--self_play's --sticky: each side repeats its own previous step's action "
                        "with this probability")
    p.add_argument("--duel_start", type=duel_start_arg, default=(38, 38),
                   help="two-player GridBoxing: the gap in pixels between the boxers of a fresh "
                        "episode, GAP or LO-HI for a uniform draw per episode; even numbers 8..38 "
                        "(38: the fixed start; 14 and below: within reach); needs --self_play")
    p.add_argument("--local_time_max", type=int, default=5,
                   help="decisions per rollout segment (train.py:102 LOCAL_TIME_MAX), 1..128")
    p.add_argument("--gamma", type=float, default=0.99,
                   help="discount per decision (train.py:94 GAMMA), in (0, 1]")
    p.add_argument("--gae_lambda", type=float, default=1.0,
                   help="lambda of the returns the learner fits (ba3c_amd.returns), in [0, 1]: "
                        "1 is the reference's n-step return, below 1 the policy advantage is "
                        "GAE(lambda) and the value target TD(lambda)")
    p.add_argument("--ppo_clip", type=float, default=0.0,
                   help="clip eps of the clipped-surrogate (PPO) loss, in (0, 1); 0: off, the A3C "
                        "loss and one gradient step per datapoint (ba3c_amd.ppo)")
    p.add_argument("--ppo_epochs", type=int, default=None,
                   help="passes over each pool of datapoints (default %d); needs --ppo_clip"
                        % ppo.DEFAULT_EPOCHS)
    p.add_argument("--ppo_minibatches", type=int, default=None,
                   help="minibatches of --batch_size datapoints per pool (default %d); needs "
                        "--ppo_clip" % ppo.DEFAULT_MINIBATCHES)
    p.add_argument("--ppo_norm_adv", action="store_true",
                   help="normalise each minibatch's advantages to mean 0, std 1 before its step; "
                        "needs --ppo_clip")
    p.add_argument("--ppo_vclip", type=float, default=0.0,
                   help="eps of the clipped value loss, >= 0; 0: off; needs --ppo_clip")
    p.add_argument("--ppo_target_kl", type=float, default=0.0,
                   help="abandon a pool's remaining epochs once an epoch's mean KL estimate "
                        "(ppo.stop_kl) exceeds this, >= 0; 0: off; needs --ppo_clip (single replica)")
    p.add_argument("--online_score", type=int, default=0,
                   help="log the episodes the training simulators finish, on the device, and write "
                        "their mean per N consecutive episodes to the online_score channel (the "
                        "reference: 10) with train_score_mean / train_score_max / "
                        "train_episode_length / train_episodes per flush; 0: off; not with --dummy")
    p.add_argument("--max_grad_norm", type=float, default=0.0,
                   help="clip the whole gradient's norm to this (ba3c_amd.gradclip; PPO codebases: "
                        "0.5) in place of the reference's per-tensor clip_by_average_norm(g, 0.1); "
                        "finite and > 0; 0: off")
    p.add_argument("--entropy_beta", type=float, default=None,
                   help="the entropy coefficient (default %g, train.py:296), finite and >= 0"
                        % DEFAULT_ENTROPY_BETA)
    p.add_argument("--lr_schedule", default=None, metavar="SPEC",
                   help="the learning rate over the run, from --lr (ba3c_amd.schedule): const, "
                        "linear:END (reached at the run's last step) or steps:E1=V1,E2=V2,... (Vk "
                        "from epoch Ek on; the reference's: steps:20=0.0005,60=0.0001)")
    p.add_argument("--entropy_schedule", default=None, metavar="SPEC",
                   help="the entropy coefficient over the run, from --entropy_beta, in "
                        "--lr_schedule's forms (the reference's: steps:40=0.005,80=0.001)")
    p.add_argument("--dummy", type=int, default=0)
    p.add_argument("--dummy_predictor", type=int, default=0)
    p.add_argument("--models_dir", default="models")
    p.add_argument("--experiment_dir", "--exp_dir", dest="experiment_dir", default=".")
    p.add_argument("--seed", type=int, default=None,
                   help="variable initialiser seed (default: the worker index, train.py:678-679)")
    # accepted for compatibility, no effect on the single-node path
    for name in ("--njobs", "-n", "--cores", "-c", "--nr_towers", "--nr_predict_towers",
                 "--intra_op_par", "--inter_op_par", "--mkl", "--cpu", "--sync", "--queue_size",
                 "--port", "--tf_port", "--threads_to_trace"):
        p.add_argument(name, type=int, default=None, help=argparse.SUPPRESS)
    for name in ("--name", "--tags", "-t", "--log_dir", "--train_log_path", "--gpu", "--early_stopping",
                 "-s", "--task"):
        p.add_argument(name, default=None, help=argparse.SUPPRESS)
    for name in ("--offline", "--intel_tf", "--short", "--debug_charts", "--save_output",
                 "--eval_node", "--record_node", "--schedule_hyper"):
        p.add_argument(name, action="store_true", help=argparse.SUPPRESS)
    return p


def resolve(args, duel_tool=False):
    """Apply the reference's implicit rules: --use_normal_fc disables replace_with_conv
    (run_job.py:131); --adam_debug sets beta2 := beta1 (train.py:460-461); --use_sync needs
    --ngrads (run_job.py:55-57).  An on-device game (GAMES) needs --channels 1 and --num_actions
    >= its own number of actions; --nr_eval, --frame_skip and --sticky need one of them.
    --self_play needs GridBoxing, an even --simulator_procs and neither --frame_skip nor --sticky:
    its two-player games take --duel_frame_skip / --duel_sticky, which like --duel_start need
    --self_play (duel_tool: the match tool, which plays two-player games without it and under
    --frame_skip / --sticky).  args.play_frame_skip / args.play_sticky are the run's setting
    either way, for the games and for --nr_eval alike.
    --gae_lambda in [0, 1], --local_time_max in 1..128, --gamma in (0, 1], and the states ring
    they imply at most 16 GiB; they apply to every -e, with and without --self_play.
    --ppo_clip in [0, 1) (0: off); --ppo_epochs / --ppo_minibatches >= 1 and only with
    --ppo_clip > 0 (default 4 each); the pool's --ppo_minibatches x --batch_size states at most
    16 GiB; not with --dummy (no simulators, nothing to replay).  --ppo_norm_adv, --ppo_vclip
    (>= 0 and finite, 0: off) and --ppo_target_kl (the same) only with --ppo_clip > 0.  args.ppo
    is the run's ppo.Setting, or None when off; it applies to every -e and to --self_play.
    --online_score >= 0 (0: off), for every -e and --self_play; not with --dummy (no simulators).
    --max_grad_norm finite and >= 0 (0: off; args.max_grad_norm is then None); --entropy_beta finite
    and >= 0; --lr_schedule / --entropy_schedule in ba3c_amd.schedule's forms with finite values, a
    learning rate > 0 (but linear:0) and a coefficient >= 0; linear needs the run's step count
    (--max_steps, or --steps_per_epoch x --max_epoch) >= 1.  args.schedules is the trainer's
    {"learning_rate": fn, "entropy_beta": fn} when either schedule was given, else None;
    args.log_schedule whether --entropy_beta or a schedule was given (the learning_rate and
    entropy_beta channels are then written).  --schedule_hyper stays accepted and ignored."""
    if args.replace_with_conv is None:
        args.replace_with_conv = not args.use_normal_fc
    if args.adam_debug:
        args.beta2 = args.beta1
    if args.use_sync and args.ngrads is None:
        raise SystemExit("if using SyncReplicasOptimizer you have to specify --ngrads argument")
    if args.environment in GAMES:
        name, A = args.environment, GAMES[args.environment][1]
        if args.channels != 1:
            raise SystemExit("-e %s renders grayscale frames: it requires --channels 1" % name)
        if args.num_actions < A:
            raise SystemExit("-e %s has %d actions: it requires --num_actions >= %d" % (name, A, A))
    elif args.nr_eval:
        raise SystemExit("--nr_eval needs a game to evaluate: pass -e %s" % " or -e ".join(sorted(GAMES)))
    try:
        skip = frameskip.setting(args.frame_skip, args.sticky)
    except ValueError as e:
        raise SystemExit("--frame_skip / --sticky: %s" % e)
    if skip is not None and args.environment not in GAMES:
        raise SystemExit("--frame_skip / --sticky need an on-device game: pass -e %s"
                         % " or -e ".join(sorted(GAMES)))
    if args.self_play:
        if args.environment != GRID_BOXING:
            raise SystemExit("--self_play is two-player GridBoxing: pass -e %s" % GRID_BOXING)
        if args.simulator_procs % 2:
            raise SystemExit("--self_play counts players, two per game: --simulator_procs must be even")
        if skip is not None:
            raise SystemExit("--self_play has no --frame_skip / --sticky: its games take "
                             "--duel_frame_skip / --duel_sticky")
    try:
        duel_skip = frameskip.setting(args.duel_frame_skip, args.duel_sticky)
    except ValueError as e:
        raise SystemExit("--duel_frame_skip / --duel_sticky: %s" % e)
    if duel_skip is not None and not args.self_play:
        raise SystemExit("--duel_frame_skip / --duel_sticky are two-player GridBoxing's: they need --self_play")
    args.play_frame_skip, args.play_sticky = ((args.duel_frame_skip, args.duel_sticky) if args.self_play
                                              else (args.frame_skip, args.sticky))
    try:
        start = duel.start_from_gap(args.duel_start)
    except ValueError as e:
        raise SystemExit("--duel_start: %s" % e)
    if start is not None and not (args.self_play or duel_tool):
        raise SystemExit("--duel_start is two-player GridBoxing's: it needs --self_play")
    # written so that a NaN fails either range
    if not 0.0 <= args.gae_lambda <= 1.0:
        raise SystemExit("--gae_lambda %r: lambda must be in [0, 1]" % args.gae_lambda)
    if not 1 <= args.local_time_max <= MAX_LOCAL_TIME:
        raise SystemExit("--local_time_max %d: must be in 1..%d" % (args.local_time_max, MAX_LOCAL_TIME))
    if not 0.0 < args.gamma <= 1.0:
        raise SystemExit("--gamma %r: the discount must be in (0, 1]" % args.gamma)
    ring = args.simulator_procs * (args.local_time_max + 1) * STATE_BYTES
    if ring > MAX_RING_BYTES:
        raise SystemExit("--simulator_procs %d x --local_time_max %d: the states ring would take "
                         "%.1f GiB (limit 16 GiB)"
                         % (args.simulator_procs, args.local_time_max, ring / 2.0 ** 30))
    if not 0.0 <= args.ppo_clip < 1.0:
        raise SystemExit("--ppo_clip %r: the clip must be in [0, 1) (0: off)" % args.ppo_clip)
    on = args.ppo_clip > 0.0
    for name in ("ppo_epochs", "ppo_minibatches"):
        v = getattr(args, name)
        if v is not None and not on:
            raise SystemExit("--%s needs --ppo_clip > 0" % name)
        if v is not None and v < 1:
            raise SystemExit("--%s %d: must be >= 1" % (name, v))
    # written so that a NaN or an infinity fails
    for name in ("ppo_vclip", "ppo_target_kl"):
        v = getattr(args, name)
        if not 0.0 <= v < float("inf"):
            raise SystemExit("--%s %r: must be >= 0 and finite (0: off)" % (name, v))
        if v > 0.0 and not on:
            raise SystemExit("--%s needs --ppo_clip > 0" % name)
    if args.ppo_norm_adv and not on:
        raise SystemExit("--ppo_norm_adv needs --ppo_clip > 0")
    if args.online_score < 0:
        raise SystemExit("--online_score %d: episodes per online_score row, must be >= 0 (0: off)"
                         % args.online_score)
    if args.online_score and args.dummy:
        raise SystemExit("--online_score logs the simulators' episodes: it cannot go with --dummy")
    # written so that a NaN or an infinity fails
    if not 0.0 <= args.max_grad_norm < float("inf"):
        raise SystemExit("--max_grad_norm %r: must be finite and > 0 (0: off)" % args.max_grad_norm)
    args.max_grad_norm = args.max_grad_norm or None
    args.log_schedule = (args.entropy_beta is not None or args.lr_schedule is not None
                         or args.entropy_schedule is not None)
    if args.entropy_beta is None:
        args.entropy_beta = DEFAULT_ENTROPY_BETA
    if not 0.0 <= args.entropy_beta < float("inf"):
        raise SystemExit("--entropy_beta %r: must be finite and >= 0" % args.entropy_beta)
    if args.lr_schedule is not None and not (math.isfinite(args.lr) and args.lr > 0.0):
        raise SystemExit("--lr_schedule starts from --lr %r: it must be finite and > 0" % args.lr)
    run_steps = args.max_steps or args.steps_per_epoch * args.max_epoch     # as train._run
    fns = {}
    for flag, key, start in (("lr_schedule", "learning_rate", args.lr),
                             ("entropy_schedule", "entropy_beta", args.entropy_beta)):
        try:
            fn = schedule.parse(getattr(args, flag), start, max_steps=run_steps,
                                steps_per_epoch=args.steps_per_epoch)
        except ValueError as e:
            raise SystemExit("--%s: %s (linear needs --max_steps or --steps_per_epoch x "
                             "--max_epoch >= 1)" % (flag, e))
        for v in fn.values:
            if key == "learning_rate" and not (v > 0.0 or (fn.kind == "linear" and v == 0.0)):
                raise SystemExit("--%s %s: a learning rate must be > 0 (only linear:0 may end at 0)"
                                 % (flag, getattr(args, flag)))
            if key == "entropy_beta" and not v >= 0.0:
                raise SystemExit("--%s %s: an entropy coefficient must be >= 0"
                                 % (flag, getattr(args, flag)))
        fns[key] = fn
    args.schedules = fns if (args.lr_schedule is not None or args.entropy_schedule is not None) else None
    args.ppo = None
    if on:
        if args.dummy:
            raise SystemExit("--ppo_clip replays rollouts: it cannot go with --dummy")
        K = ppo.DEFAULT_EPOCHS if args.ppo_epochs is None else args.ppo_epochs
        M = ppo.DEFAULT_MINIBATCHES if args.ppo_minibatches is None else args.ppo_minibatches
        pool = M * args.batch_size * STATE_BYTES
        if pool > MAX_RING_BYTES:
            raise SystemExit("--ppo_minibatches %d x --batch_size %d: the pool's states would take "
                             "%.1f GiB (limit 16 GiB)" % (M, args.batch_size, pool / 2.0 ** 30))
        args.ppo = ppo.Setting(clip=args.ppo_clip, epochs=K, minibatches=M,
                               norm_adv=bool(args.ppo_norm_adv), vclip=args.ppo_vclip,
                               target_kl=args.ppo_target_kl)
    return args
