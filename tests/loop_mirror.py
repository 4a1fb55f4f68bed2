"""The host simulator master beside an ActorLearner: the one wrapper the loop tests share."""
import numpy as np


class LoopMirror(object):
    """Wraps `put` of the loop's queue (A3C) or pool (PPO) and `on_state` / `on_reward` of its
    buf, and feeds `mirror` (an oracle SimulatorMasterMirror or a LambdaMasterMirror) simulator
    by simulator with what they were given; transition e of step t carries the state id (t, e).
    consumed: the (action, R) pairs put, in order; queued(): the mirror's, to compare with;
    rows: the PPO rows put along with them, one array per put.
    drawn: per step (actions, values, logp or None) as on_state got them; rewards, overs: per
    step the arrays on_reward got.  on_step(rewards, overs), if given, runs in on_reward before
    the mirror is fed.  Without PPO on_state takes exactly the loop's three positional arguments."""

    def __init__(self, loop, mirror, on_step=None):
        self.mirror = mirror
        self.consumed, self.rows, self.drawn, self.rewards, self.overs = [], [], [], [], []
        sink = loop.queue if loop.pool is None else loop.pool
        orig_put, orig_on_state, orig_on_reward = sink.put, loop.buf.on_state, loop.buf.on_reward

        def put(dps):
            self.consumed.extend(zip(dps.action.cpu().numpy().tolist(), dps.R.cpu().numpy().tolist()))
            if dps.rows is not None:
                self.rows.append(dps.rows.cpu().numpy())
            orig_put(dps)

        def on_state(states, actions, values, **logp):
            assert sorted(logp) == ([] if loop.pool is None else ["logp"])
            a, v = actions.cpu().numpy(), values.cpu().numpy()
            for e in range(len(a)):
                mirror.on_state(e, (len(self.drawn), e), int(a[e]), np.float32(v[e]))
            self.drawn.append((a, v, logp["logp"].cpu().numpy() if logp else None))
            orig_on_state(states, actions, values, **logp)

        def on_reward(rew, over):
            r, o = rew.cpu().numpy(), over.cpu().numpy()
            if on_step is not None:
                on_step(r, o)
            self.rewards.append(r)
            self.overs.append(o)
            for e in range(len(r)):
                mirror.on_message(e, float(r[e]), bool(o[e]))
            return orig_on_reward(rew, over)
        sink.put, loop.buf.on_state, loop.buf.on_reward = put, on_state, on_reward

    def episodes_over(self):
        return sum(int(o.sum()) for o in self.overs)

    def queued(self):
        return [(k["action"], float(np.float32(R))) for k, R, _, _ in self.mirror.queue]
