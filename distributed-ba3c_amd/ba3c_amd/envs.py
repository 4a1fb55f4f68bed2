"""Players of the simulator side: the RLEnvironment / ProxyPlayer
contract (RL/envbase.py:13-141) and the wrappers OpenAIGym/train.py:113-128 stacks around the
game (RL/history.py:12-55, RL/common.py:14-83).

They run inside each simulator process on the host, exactly where the reference runs them;
only their states cross into the learner (ba3c_amd.simulator).  gym/ALE are not installable
here, so `SyntheticAtariPlayer` stands in for GymEnv + the 84x84 resize (grayscale uint8
frames, integer rewards incl. values the returns clip, episodes of 20..80 steps).
"""
from collections import defaultdict, deque

import numpy as np

FRAME_HISTORY = 4          # train.py:95 (--frame_history default)
IMAGE_SIZE = (84, 84)      # train.py:92


class DiscreteActionSpace(object):
    """RL/envbase.py:108-124: `sample()` draws from the space's own RNG."""

    def __init__(self, num, seed=None):
        self.num = int(num)
        self.rng = np.random.RandomState(seed)

    def sample(self):
        return self.rng.randint(self.num)

    def num_actions(self):
        return self.num

    def __repr__(self):
        return "DiscreteActionSpace({})".format(self.num)


class RLEnvironment(object):
    """RL/envbase.py:13-72."""

    def __init__(self):
        self.reset_stat()

    def current_state(self):
        raise NotImplementedError()

    def action(self, act):
        """Perform `act`; returns (reward, isOver).  Starts a new episode when isOver."""
        raise NotImplementedError()

    def restart_episode(self):
        raise NotImplementedError()

    def finish_episode(self):
        pass

    def get_action_space(self):
        raise NotImplementedError()

    def reset_stat(self):
        self.stats = defaultdict(list)

    def play_one_episode(self, func, stat="score"):
        """envbase.py:54-72: run `func(state) -> action` until the episode ends."""
        if not isinstance(stat, list):
            stat = [stat]
        while True:
            s = self.current_state()
            r, over = self.action(func(s))
            if over:
                out = [self.stats[k] for k in stat]
                self.reset_stat()
                return out if len(out) > 1 else out[0]


class ProxyPlayer(RLEnvironment):
    """RL/envbase.py:126-155: forwards everything to `player`."""

    def __init__(self, player):
        self.player = player

    def reset_stat(self):
        self.player.reset_stat()

    def current_state(self):
        return self.player.current_state()

    def action(self, act):
        return self.player.action(act)

    @property
    def stats(self):
        return self.player.stats

    def restart_episode(self):
        self.player.restart_episode()

    def finish_episode(self):
        self.player.finish_episode()

    def get_action_space(self):
        return self.player.get_action_space()


class HistoryFramePlayer(ProxyPlayer):
    """RL/history.py:12-55: the state is the last `hist_len` frames concatenated on the
    channel axis, zero frames in front at the start of an episode."""

    def __init__(self, player, hist_len):
        super(HistoryFramePlayer, self).__init__(player)
        self.history = deque(maxlen=hist_len)
        self.history.append(self._frame())

    def _frame(self):
        s = self.player.current_state()
        return s.reshape(s.shape[0], s.shape[1], 1) if s.ndim != 3 else s

    def current_state(self):
        assert len(self.history) != 0
        pad = [np.zeros_like(self.history[0])] * (self.history.maxlen - len(self.history))
        return np.concatenate(pad + list(self.history), axis=2)

    def action(self, act):
        r, over = self.player.action(act)
        s = self._frame()
        self.history.append(s)
        if over:                              # s is the first frame of a new episode
            self.history.clear()
            self.history.append(s)
        return r, over

    def restart_episode(self):
        super(HistoryFramePlayer, self).restart_episode()
        self.history.clear()
        self.history.append(self._frame())


class PreventStuckPlayer(ProxyPlayer):
    """RL/common.py:14-40: after `nr_repeat` identical actions in a row, play `action`
    instead (e.g. FIRE to start Breakout).  The repeat window is cleared on episode end."""

    def __init__(self, player, nr_repeat, action):
        super(PreventStuckPlayer, self).__init__(player)
        self.act_que = deque(maxlen=nr_repeat)
        self.trigger_action = action

    def action(self, act):
        self.act_que.append(act)
        if self.act_que.count(self.act_que[0]) == self.act_que.maxlen:
            act = self.trigger_action
        r, over = self.player.action(act)
        if over:
            self.act_que.clear()
        return r, over

    def restart_episode(self):
        super(PreventStuckPlayer, self).restart_episode()
        self.act_que.clear()


class LimitLengthPlayer(ProxyPlayer):
    """RL/common.py:42-64: end (and restart) the episode after `limit` actions."""

    def __init__(self, player, limit):
        super(LimitLengthPlayer, self).__init__(player)
        self.limit = limit
        self.cnt = 0

    def action(self, act):
        r, over = self.player.action(act)
        self.cnt += 1
        if self.cnt >= self.limit:
            over = True
            self.finish_episode()
            self.restart_episode()
        if over:
            self.cnt = 0
        return r, over

    def restart_episode(self):
        self.player.restart_episode()
        self.cnt = 0


class AutoRestartPlayer(ProxyPlayer):
    """RL/common.py:66-74: finish + restart the underlying player on episode end."""

    def action(self, act):
        r, over = self.player.action(act)
        if over:
            self.player.finish_episode()
            self.player.restart_episode()
        return r, over


class MapPlayerState(ProxyPlayer):
    """RL/common.py:76-83: `current_state` passed through `func` (train.py:116-119 resizes)."""

    def __init__(self, player, func):
        super(MapPlayerState, self).__init__(player)
        self.func = func

    def current_state(self):
        return self.func(self.player.current_state())


class SyntheticAtariPlayer(RLEnvironment):
    """Stand-in for GymEnv (gym/ALE absent): one game whose frame at step t is a moving byte
    pattern, reward 1 when the action matches a per-step target (3 every 7th step, which the
    returns clip), episodes of 20..80 steps; auto-restarts like GymEnv and records the
    episode 'score' stat the evaluation reads."""

    def __init__(self, idx=0, num_actions=4, seed=0):
        super(SyntheticAtariPlayer, self).__init__()
        self.idx = int(idx)
        self.A = int(num_actions)
        self.rng = np.random.RandomState(seed)
        self.space = DiscreteActionSpace(self.A, seed=seed + 1)
        yy, xx = np.mgrid[0:IMAGE_SIZE[0], 0:IMAGE_SIZE[1]]
        self._base = 3 * xx + 5 * yy
        self.restart_episode()

    def restart_episode(self):
        self.t = 0
        self.length = int(self.rng.randint(20, 81))
        self.score = 0.0

    def finish_episode(self):
        self.stats["score"].append(self.score)

    def current_state(self):
        return ((self._base + 7 * self.t + 11 * self.idx) & 255).astype(np.uint8)

    def action(self, act):
        hit = float(int(act) == (self.t + self.idx) % self.A)
        r = 3.0 * hit if self.t % 7 == 6 else hit
        self.score += r
        self.t += 1
        over = self.t >= self.length
        if over:
            self.finish_episode()
            self.restart_episode()
        return r, over

    def get_action_space(self):
        return self.space


class BreakoutPlayer(RLEnvironment):
    """GridBreakout (ba3c_amd.breakout holds the rules and constants) as one host player, for
    the simulator processes: the same integer rules as scalar Python ints.  Auto-restarts like
    GymEnv and records the episode 'score' stat in finish_episode.  `limit` (None: none) ends
    an episode after that many steps; get_player leaves that to LimitLengthPlayer.
    `last_events` names what the last action() met, from: wall, ceiling, brick7, brick4,
    brick1, paddle, lost, over_lives, over_clear, over_limit."""

    def __init__(self, idx=0, num_actions=4, seed=0, limit=None):
        super(BreakoutPlayer, self).__init__()
        from . import breakout as K
        self.K = K
        self.idx = int(idx)
        self.limit = limit
        self.rng = (int(seed) * 1000 + self.idx) % (1 << 32)
        self.space = DiscreteActionSpace(int(num_actions), seed=seed + 1)
        self.last_events = set()
        self.last_ep_score = None
        self.restart_episode()

    def restart_episode(self):
        K = self.K
        self.px = K.PX_START
        self.bx = self.by = self.vx = self.vy = self.in_play = 0
        self.lives = K.LIVES
        self.score = 0
        self.t = 0
        self.bricks = [K.FULL_ROW] * K.ROWS

    def finish_episode(self):
        self.stats["score"].append(self.score)

    def game_row(self):
        """The episode state as the device's int32 row (breakout.py layout)."""
        rng = self.rng - (1 << 32) if self.rng >= (1 << 31) else self.rng
        return [self.px, self.bx, self.by, self.vx, self.vy, self.in_play, self.lives, self.score,
                self.t, rng] + list(self.bricks)

    def current_state(self):
        K = self.K
        f = np.zeros((K.H, K.W), np.uint8)
        for i in range(self.lives):
            f[K.LIVES_Y:K.LIVES_Y + 2, 4 * i:4 * i + 2] = K.LIVES_SHADE
        for r in range(K.ROWS):
            y0 = K.BRICK_Y0 + K.BRICK_H * r
            for c in range(K.COLS):
                if (self.bricks[r] >> c) & 1:
                    f[y0:y0 + K.BRICK_H, K.BRICK_W * c:K.BRICK_W * (c + 1)] = K.SHADE[r]
        f[K.PADDLE_Y:K.PADDLE_Y + K.PADDLE_H, self.px:self.px + K.PADDLE_W] = 255
        if self.in_play:
            f[self.by:self.by + K.BALL, self.bx:self.bx + K.BALL] = 255
        return f

    def action(self, act):
        K = self.K
        ev = set()
        act = int(act)
        reward = 0
        if act == K.RIGHT:
            self.px = min(self.px + K.PADDLE_STEP, K.PX_MAX)
        elif act == K.LEFT:
            self.px = max(self.px - K.PADDLE_STEP, 0)
        if not self.in_play:
            if act == K.FIRE:
                self.rng = (self.rng * K.LCG_A + K.LCG_C) % (1 << 32)
                self.bx = 8 + ((self.rng >> 16) % 68)
                self.by = 40
                self.vx = 1 if (self.rng >> 8) & 1 else -1
                self.vy = 2
                self.in_play = 1
        else:
            nx, ny = self.bx + self.vx, self.by + self.vy
            if nx < 0:
                nx, self.vx = -nx, -self.vx
                ev.add("wall")
            elif nx > 82:
                nx, self.vx = 164 - nx, -self.vx
                ev.add("wall")
            if ny < 0:
                ny, self.vy = -ny, -self.vy
                ev.add("ceiling")
            for cx, cy in ((nx, ny), (nx + 1, ny), (nx, ny + 1), (nx + 1, ny + 1)):
                if 18 <= cy < 36:
                    r, c = (cy - 18) // 3, cx // 6
                    if (self.bricks[r] >> c) & 1:
                        self.bricks[r] &= ~(1 << c)
                        reward += K.VAL[r]
                        self.vy = -self.vy
                        ny = self.by
                        ev.add("brick%d" % K.VAL[r])
                        break
            if (self.vy > 0 and self.by + 1 < 78 and ny + 1 >= 78 and nx + 1 >= self.px
                    and nx <= self.px + 11):
                ny, self.vy = 76, -2
                d = nx + 1 - (self.px + 6)
                self.vx = -2 if d < -3 else -1 if d < 0 else 1 if d < 3 else 2
                ev.add("paddle")
            self.bx, self.by = nx, ny
            if self.by > 82:
                self.in_play = 0
                self.lives -= 1
                ev.add("lost")
        self.score += reward
        self.t += 1
        if self.lives == 0:
            ev.add("over_lives")
        if not any(self.bricks):
            ev.add("over_clear")
        if self.limit is not None and self.t >= self.limit:
            ev.add("over_limit")
        over = bool(ev & {"over_lives", "over_clear", "over_limit"})
        if over:
            self.last_ep_score = self.score
            self.finish_episode()
            self.restart_episode()
        self.last_events = ev
        return float(reward), over

    def get_action_space(self):
        return self.space


class BoxingPlayer(RLEnvironment):
    """GridBoxing (ba3c_amd.boxing holds the rules and constants) as one host player, for the
    simulator processes: the same integer rules as scalar Python ints.  Auto-restarts like
    GymEnv and records the episode 'score' stat (agent minus opponent) in finish_episode.
    `limit` (None: none) ends an episode after that many steps; get_player leaves that to
    LimitLengthPlayer.  `last_events` names what the last action() met, from: hit1, hit2, miss,
    got1, got2, ko_win, ko_loss, over_clock, over_limit."""

    def __init__(self, idx=0, num_actions=18, seed=0, limit=None):
        super(BoxingPlayer, self).__init__()
        from . import boxing as K
        self.K = K
        self.idx = int(idx)
        self.limit = limit
        self.rng = (int(seed) * 1000 + self.idx) % (1 << 32)
        self.space = DiscreteActionSpace(int(num_actions), seed=seed + 1)
        self.last_events = set()
        self.last_ep_score = None
        self.restart_episode()

    def restart_episode(self):
        K = self.K
        self.ax, self.ay, self.ox, self.oy = K.AX0, K.AY0, K.OX0, K.OY0
        self.a_cd = self.o_cd = self.a_score = self.o_score = self.t = 0

    def finish_episode(self):
        self.stats["score"].append(self.a_score - self.o_score)

    def game_row(self):
        """The episode state as the device's int32 row (boxing.py layout)."""
        rng = self.rng - (1 << 32) if self.rng >= (1 << 31) else self.rng
        return [self.ax, self.ay, self.ox, self.oy, self.a_cd, self.o_cd, self.a_score,
                self.o_score, self.t, rng, 0, 0, 0, 0, 0, 0]

    def current_state(self):
        K = self.K
        f = np.zeros((K.H, K.W), np.uint8)
        f[K.RING_Y0, K.RING_X0:K.RING_X1 + 1] = f[K.RING_Y1, K.RING_X0:K.RING_X1 + 1] = K.DIM
        f[K.RING_Y0:K.RING_Y1 + 1, K.RING_X0] = f[K.RING_Y0:K.RING_Y1 + 1, K.RING_X1] = K.DIM
        f[K.CLOCK_Y, :max(K.W - self.t // K.CLOCK_DIV, 0)] = K.DIM
        f[K.O_BAR_Y:K.O_BAR_Y + 2, K.W - self.o_score // 2:] = K.OPP_SHADE
        f[K.A_BAR_Y:K.A_BAR_Y + 2, :self.a_score // 2] = K.AGENT_SHADE
        # later paints win: opponent arm, opponent body, agent arm, agent body
        for x, y, cd, arm_left, shade in (
                (self.ox, self.oy, self.o_cd, self.ox >= self.ax, K.OPP_SHADE),
                (self.ax, self.ay, self.a_cd, not self.ax <= self.ox, K.AGENT_SHADE)):
            if cd >= K.ARM_CD:
                x0 = x - K.ARM_W if arm_left else x + K.BODY_W
                f[y + K.ARM_ROW:y + K.ARM_ROW + K.ARM_H, x0:x0 + K.ARM_W] = shade
            f[y:y + K.BODY_H, x:x + K.BODY_W] = shade
        return f

    def _pts(self):
        K = self.K
        gx, gy = abs(self.ax - self.ox), abs(self.ay - self.oy)
        if gy > K.REACH_Y or gx > K.REACH_FAR:
            return 0
        return 2 if gx <= K.REACH_NEAR else 1

    def action(self, act):
        K = self.K
        ev = set()
        act = int(act)
        if not 0 <= act < K.NUM_ACTIONS:
            act = K.NOOP
        clamp = lambda v, lo, hi: min(max(v, lo), hi)
        sign = lambda v: (v > 0) - (v < 0)
        reward = 0
        dx = (act in K.RIGHT_SET) - (act in K.LEFT_SET)
        dy = (act in K.DOWN_SET) - (act in K.UP_SET)
        self.a_cd = max(self.a_cd - 1, 0)
        self.o_cd = max(self.o_cd - 1, 0)
        self.rng = (self.rng * K.LCG_A + K.LCG_C) % (1 << 32)
        r = self.rng >> 16
        self.ax = clamp(self.ax + K.AGENT_STEP * dx, K.X_MIN, K.X_MAX)
        self.ay = clamp(self.ay + K.AGENT_STEP * dy, K.Y_MIN, K.Y_MAX)
        if r & 3:
            s, gap = sign(self.ax - self.ox), abs(self.ax - self.ox)
            ody = sign(self.ay - self.oy)
            if gap > K.CLOSE_FAR:
                odx = s
            elif gap < K.CLOSE_NEAR:
                odx = -s if s != 0 else 1
            else:
                odx = 0
        else:
            odx, ody = ((r >> 2) % 3) - 1, ((r >> 4) % 3) - 1
        self.ox = clamp(self.ox + K.OPP_STEP * odx, K.X_MIN, K.X_MAX)
        self.oy = clamp(self.oy + K.OPP_STEP * ody, K.Y_MIN, K.Y_MAX)
        if act in K.FIRE_SET and self.a_cd == 0:
            self.a_cd = K.COOLDOWN
            p = self._pts()
            ev.add("hit%d" % p if p else "miss")
            if p:
                reward += p
                self.a_score += p
                self.ox = clamp(self.ox + (K.KNOCK if self.ox >= self.ax else -K.KNOCK),
                                K.X_MIN, K.X_MAX)
        if self.o_cd == 0 and ((r >> 8) & 1) == 0 and self._pts() > 0:
            self.o_cd = K.COOLDOWN
            p = self._pts()
            ev.add("got%d" % p)
            reward -= p
            self.o_score += p
            self.ax = clamp(self.ax + (K.KNOCK if self.ax > self.ox else -K.KNOCK),
                            K.X_MIN, K.X_MAX)
        self.t += 1
        if self.a_score >= K.KO:
            ev.add("ko_win")
        if self.o_score >= K.KO:
            ev.add("ko_loss")
        if self.t >= K.CLOCK:
            ev.add("over_clock")
        if self.limit is not None and self.t >= self.limit:
            ev.add("over_limit")
        over = bool(ev & {"ko_win", "ko_loss", "over_clock", "over_limit"})
        if over:
            self.last_ep_score = self.a_score - self.o_score
            self.finish_episode()
            self.restart_episode()
        self.last_events = ev
        return float(reward), over

    def get_action_space(self):
        return self.space


class FrameSkipPlayer(ProxyPlayer):
    """Frame skip and sticky actions around a BreakoutPlayer / BoxingPlayer: ba3c_amd.frameskip's
    decision as scalar Python ints, for the simulator processes.  One action() draws k in
    [lo, hi], plays k game steps of the wrapped player (each repeats the previous effective
    action when its 16-bit draw is below q16, else plays `act`), sums their rewards and stops at
    an episode's end.  `aux_row()` is the device's aux row [rng2, prev], next to the wrapped
    player's `game_row()`.  The wrapped player's `limit` counts game steps, not decisions."""

    def __init__(self, player, lo, hi, q16, seed=0, idx=0):
        super(FrameSkipPlayer, self).__init__(player)
        from . import frameskip as F
        F.check(lo, hi, q16)
        self.F = F
        self.lo, self.hi, self.q16 = int(lo), int(hi), int(q16)
        self.rng2 = F.initial_rng2(seed, idx)
        self.prev = 0

    def game_row(self):
        return self.player.game_row()

    def aux_row(self):
        rng2 = self.rng2 - (1 << 32) if self.rng2 >= (1 << 31) else self.rng2
        return [rng2, self.prev]

    def action(self, act):
        F = self.F
        act = int(act)
        if not 0 <= act < F.ACTION_BOUND:
            act = 0
        self.rng2 = F.lcg(self.rng2)
        k = self.lo + ((self.rng2 >> 16) % (self.hi - self.lo + 1))
        reward, over = 0.0, False
        for _ in range(k):
            self.rng2 = F.lcg(self.rng2)
            if ((self.rng2 >> 8) & 0xFFFF) >= self.q16:
                self.prev = act
            r, over = self.player.action(self.prev)
            reward += r
            if over:                          # the player has restarted: drop the rest
                self.prev = 0
                break
        return reward, over

    def restart_episode(self):
        super(FrameSkipPlayer, self).restart_episode()
        self.prev = 0


# game key -> the host player of get_player / SyntheticSimulatorWorker
PLAYERS = {"synthetic": SyntheticAtariPlayer, "breakout": BreakoutPlayer, "boxing": BoxingPlayer}


def get_player(idx=0, num_actions=4, seed=0, train=False, frame_history=FRAME_HISTORY,
               limit=40000, game="synthetic", frame_skip=1, sticky=0.0):
    """OpenAIGym/train.py:113-128 with the synthetic game (or game="breakout": GridBreakout,
    game="boxing": GridBoxing): history of `frame_history` frames, PreventStuckPlayer(30, 1)
    for evaluation players, LimitLengthPlayer(40000).
    A non-default `frame_skip` (K or (lo, hi)) / `sticky` (a probability) puts a FrameSkipPlayer
    under the history, for GridBreakout / GridBoxing only; `limit` then counts game steps as it
    does on the device: the game's own player ends the episode, in place of LimitLengthPlayer."""
    if game not in PLAYERS:
        raise ValueError("unknown game %r (%s)" % (game, ", ".join(sorted(PLAYERS))))
    from .frameskip import setting
    skip = setting(frame_skip, sticky)
    if skip is None:
        pl = PLAYERS[game](idx, num_actions, seed)
    elif game == "synthetic":
        raise ValueError("frame_skip / sticky need game='breakout' or game='boxing'")
    else:
        pl = FrameSkipPlayer(PLAYERS[game](idx, num_actions, seed, limit=limit), *skip, seed=seed, idx=idx)
    pl = HistoryFramePlayer(pl, frame_history)
    if not train:
        pl = PreventStuckPlayer(pl, 30, 1)
    return pl if skip is not None else LimitLengthPlayer(pl, limit)
