"""Recorded matches of two-player GridBoxing on the MI355X (ba3c_amd.record.record_match): a
recording replays bit for bit on the CPU oracle, shows what `duel.match` plays with the same
arguments, round-trips through its .npz, and its frames are the oracle's view of the replayed
rows as the chosen side sees them.  `python -m ba3c_amd.duel --record` runs in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from duel_policy import hit_and_run_policy, noop_policy

pytestmark = pytest.mark.gpu

PLAIN = dict(frame_skip=1, sticky=0.0, start=None)
SKIPPED = dict(frame_skip=(2, 4), sticky=0.25, start=(4, 7))


@pytest.mark.parametrize("how,side", [(PLAIN, "a"), (SKIPPED, "b")])
def test_a_recorded_match_replays_and_shows_what_match_plays(how, side, tmp_path):
    from ba3c_amd import boxing as K
    from ba3c_amd import duel as D
    from ba3c_amd.record import MatchEpisode, record_match
    from ba3c_amd.view import hud_from_policy, view_numpy
    traces = record_match(hit_and_run_policy, noop_policy, 3, 4, seed=2, limit=40, scale=2, every=3,
                          max_frames=9, side=side, **how)
    played = D.match(hit_and_run_policy, noop_policy, n_games=4, episodes=3, seed=2, limit=40, **how)
    assert [t.score for t in traces] == played["scores"] and len(traces) == played["episodes"] >= 3
    skipped = how is SKIPPED
    for i, t in enumerate(traces):
        assert (t.aux0 is not None) == skipped and t.skip == ((2, 4, 16384) if skipped else None)
        assert t.start == ((4, 7) if skipped else None) and t.side == side and t.limit == 40
        assert t.actions.shape == (t.steps, 2) and t.probs.shape == (t.steps, 2, 18)
        assert t.values.shape == (t.steps, 2) and t.rewards.shape == (t.steps,)
        assert (t.probs.sum(2) == 1).all() and not t.values.any()             # one-hot scripts, no value
        assert (t.actions[:29] == t.probs[:29].argmax(2)).mean() > 0.9       # (eps-greedy, PreventStuck)
        rows, rewards, score = t.replay()
        assert (rewards == t.rewards).all() and score == t.score
        # the final row is the next episode's first: fresh, or drawn from the row's own rng
        if skipped:
            assert rows[-1, 2] - rows[-1, 0] in (8, 10, 12, 14) and rows[-1, 1] == rows[-1, 3]
            assert t.steps <= 20 and rows[-1, 9] != rows[0, 9]
        else:
            assert rows[-1, :9].tolist() == [20, 42, 58, 42, 0, 0, 0, 0, 0] and t.steps == 40
        assert (rows[:-1, 8] < 40).all() and not rows[-1, 4:9].any()
        # frames: every third decision, as `side` sees the replayed rows, its output in the HUD
        assert t.frame_steps.tolist() == list(range(0, t.steps, 3))[:9]
        assert t.frames.shape == (len(t.frame_steps), 208, 168, 3) and t.frames.dtype == np.uint8
        p = 0 if side == "a" else 1
        for j, s in enumerate(t.frame_steps.tolist()):
            hud = hud_from_policy(torch.from_numpy(t.probs[s:s + 1, p]), torch.from_numpy(t.actions[s:s + 1, p]),
                                  torch.from_numpy(t.values[s:s + 1, p])).numpy()
            seen = rows[s:s + 1] if side == "a" else D.mirror_rows(rows[s:s + 1])
            assert (t.frames[j] == view_numpy(seen, K.PALETTE, 2, hud)[0]).all(), (i, j)
        files = t.save(str(tmp_path / ("match_%d" % i)))
        assert files[0].endswith(".npz") and all(os.path.getsize(f) > 0 for f in files)
        back = MatchEpisode.load(files[0])
        for k in ("row0", "aux0", "actions", "rewards", "probs", "values", "frames", "frame_steps"):
            a, b = getattr(t, k), getattr(back, k)
            assert (a is None and b is None) or (a.dtype == b.dtype and (a == b).all()), k
        assert (back.limit, back.skip, back.start, back.side, back.score, back.steps) == (
            t.limit, t.skip, t.start, t.side, t.score, t.steps)
        assert all((x == y).all() for x, y in zip(back.replay()[:2], (rows, rewards)))
    # the next episode of a game starts from the row (and aux row) the previous one ended on
    assert any((t.row0[:9] != [20, 42, 58, 42, 0, 0, 0, 0, 0]).any() for t in traces) == skipped


def test_the_match_tool_records_in_a_child_process(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(root, "distributed-ba3c_amd"), env.get("PYTHONPATH", "")])
    out_dir = tmp_path / "rec"
    argv = ("--random_b --fc_neurons 128 --fc_splits 4 --episodes 2 --games 2 --limit 30 --seed 3 "
            "--frame_skip 2-4 --sticky 0.25 --duel_start 8-14 --scale 1 --every 2 --max_frames 5 "
            "--side b").split()
    argv += ["--record", str(out_dir), "--models_dir", str(tmp_path / "models"),
             "--experiment_dir", str(tmp_path / "exp")]
    r = subprocess.run([sys.executable, "-m", "ba3c_amd.duel"] + argv, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["episodes"] == len(out["scores"]) >= 2 and out["side_b"] == "random"
    npz = [f for f in out["files"] if f.endswith(".npz")]
    assert len(npz) == out["episodes"] and all(os.path.isfile(f) for f in out["files"])
    from ba3c_amd.record import MatchEpisode
    for f, score in zip(npz, out["scores"]):
        t = MatchEpisode.load(f)
        rows, rewards, replayed = t.replay()
        assert replayed == t.score == score and (rewards == t.rewards).all()
        assert t.skip == (2, 4, 16384) and t.start == (4, 7) and t.side == "b" and len(t.frames) <= 5
