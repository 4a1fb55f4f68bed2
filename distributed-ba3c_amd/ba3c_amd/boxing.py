"""GridBoxing: a small integer-only Boxing that lives on the GPU (`-e GridBoxing-v0`).

The second on-device game next to GridBreakout (ba3c_amd.breakout): ALE's full 18-action set,
rewards of both signs ("mine minus theirs") and a scripted adversary; an episode ends on a
knock-out (either side reaching 100 points), on the clock or on the step limit.  This module
holds the rules ONCE: the constants, `step_numpy` / `render_numpy` (a vectorised CPU statement,
the oracle of the HIP kernel in csrc/ba3c_boxing.h) and `BoxingVec`, E simulators on the device
with BreakoutVec's interface.  `ba3c_amd.envs.BoxingPlayer` restates the same rules as scalar
Python ints for the simulator processes; tests hold the three statements equal bit for bit.

State: `game[e] = [ax, ay, ox, oy, a_cd, o_cd, a_score, o_score, t, rng, 0, 0, 0, 0, 0, 0]`,
16 int32; a* is the agent, o* the scripted opponent; the six padding ints are written as 0.
Frame: 84x84 grayscale uint8.  Each boxer is a 6x8 px body (6 wide, 8 tall) whose top-left
(x, y) satisfies x in [4, 74] and y in [14, 70].
Fresh episode: ax, ay, ox, oy = 20, 42, 58, 42; cooldowns, scores and t zero; rng is kept.

Actions: ALE's 18.  0 NOOP, 1 FIRE, 2 UP, 3 RIGHT, 4 LEFT, 5 DOWN, 6 UPRIGHT, 7 UPLEFT,
8 DOWNRIGHT, 9 DOWNLEFT, 10 UPFIRE, 11 RIGHTFIRE, 12 LEFTFIRE, 13 DOWNFIRE, 14 UPRIGHTFIRE,
15 UPLEFTFIRE, 16 DOWNRIGHTFIRE, 17 DOWNLEFTFIRE; any other value is NOOP.  An action is
range-checked and then tested against the five component masks UP / DOWN / RIGHT / LEFT / FIRE
(`(MASK >> a) & 1`); it never indexes memory.

step(a), in exactly this order:

    reward = 0
    dx = right - left; dy = down - up                       # each in {-1, 0, 1}
    a_cd = max(a_cd - 1, 0); o_cd = max(o_cd - 1, 0)
    rng = (rng * 1664525 + 1013904223) mod 2^32; r = rng >> 16
    ax = clamp(ax + 2*dx, 4, 74); ay = clamp(ay + 2*dy, 14, 70)
    if r & 3:                                               # 3 steps in 4: close in
        s = sign(ax - ox); gap = |ax - ox|; ody = sign(ay - oy)
        odx = s if gap > 11 else (-s if s != 0 else 1) if gap < 8 else 0
    else:                                                   # 1 in 4: wander
        odx = ((r >> 2) % 3) - 1; ody = ((r >> 4) % 3) - 1
    ox = clamp(ox + odx, 4, 74); oy = clamp(oy + ody, 14, 70)
    pts() = 0 if |ay - oy| > 4 or |ax - ox| > 14 else (2 if |ax - ox| <= 9 else 1)
    if fire and a_cd == 0:
        a_cd = 8; p = pts()
        if p: reward += p; a_score += p; ox = clamp(ox + (3 if ox >= ax else -3), 4, 74)
    if o_cd == 0 and ((r >> 8) & 1) == 0 and pts() > 0:     # pts() after the knock-back above
        o_cd = 8; p = pts(); reward -= p; o_score += p
        ax = clamp(ax + (3 if ax > ox else -3), 4, 74)
    t += 1
    over = a_score >= 100 or o_score >= 100 or t >= 1680 or t >= limit
    ep_score = a_score - o_score                            # in [-101, 101]
    if over: reset to a fresh episode (rng kept)

render: pixel (y, x) takes the first match of: agent body (255); agent arm (255) while
a_cd >= 6, a 4x2 px bar at body rows 3..4 leaving the side that faces the opponent (the agent
faces right if ax <= ox); opponent body (130); opponent arm (130) by the same rule with o_cd
(the opponent faces left if ox >= ax); agent score bar (y in {2, 3}, x < a_score // 2, 255);
opponent score bar (y in {5, 6}, x >= 84 - o_score // 2, 130); clock bar (y = 8,
x < 84 - t // 20, 60); the 1 px ring outline (60) along y = 12 and y = 79 for x in [2, 81] and
along x = 2 and x = 81 for y in [12, 79]; else 0.  The frame a step returns is the frame AFTER
the step, so on `over` it is the new episode's first frame (as in GridBreakout).
"""
import numpy as np

from .gamevec import GameVec

H = W = 84
BODY_W, BODY_H = 6, 8
X_MIN, X_MAX, Y_MIN, Y_MAX = 4, 74, 14, 70
AX0, AY0, OX0, OY0 = 20, 42, 58, 42
AGENT_STEP, OPP_STEP = 2, 1
COOLDOWN, ARM_CD = 8, 6                  # a punch costs 8 steps; the arm shows while cd >= 6
ARM_W, ARM_H, ARM_ROW = 4, 2, 3
REACH_Y, REACH_FAR, REACH_NEAR = 4, 14, 9   # |dy| <= 4; |dx| <= 14 scores 1, |dx| <= 9 scores 2
CLOSE_FAR, CLOSE_NEAR = 11, 8            # the opponent closes in above 11 and backs off below 8
KNOCK = 3
KO, CLOCK = 100, 1680
AGENT_SHADE, OPP_SHADE, DIM = 255, 130, 60
A_BAR_Y, O_BAR_Y, CLOCK_Y, CLOCK_DIV = 2, 5, 8, 20
RING_X0, RING_X1, RING_Y0, RING_Y1 = 2, 81, 12, 79
NUM_ACTIONS = 18
NOOP, FIRE = 0, 1
UP_SET = (2, 6, 7, 10, 14, 15)
DOWN_SET = (5, 8, 9, 13, 16, 17)
RIGHT_SET = (3, 6, 8, 11, 14, 16)
LEFT_SET = (4, 7, 9, 12, 15, 17)
FIRE_SET = (1, 10, 11, 12, 13, 14, 15, 16, 17)
UP_MASK, DOWN_MASK, RIGHT_MASK, LEFT_MASK, FIRE_MASK = (
    sum(1 << i for i in s) for s in (UP_SET, DOWN_SET, RIGHT_SET, LEFT_SET, FIRE_SET))
LCG_A, LCG_C = 1664525, 1013904223
DEFAULT_LIMIT = 40000                    # LimitLengthPlayer(40000), train.py:127
# column indices of a game row
AX, AY, OX, OY, A_CD, O_CD, A_SCORE, O_SCORE, T, RNG = range(10)
ROW_INTS = 16
# the colour of every shade for ba3c_amd.view: grey (i, i, i) except the shades render draws
COLOURS = {0: (88, 144, 72), AGENT_SHADE: (240, 240, 240), OPP_SHADE: (20, 20, 20),
           DIM: (200, 160, 60)}
PALETTE = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
for _shade, _rgb in COLOURS.items():
    PALETTE[_shade] = _rgb
PALETTE.setflags(write=False)


def action_id(dx, dy, fire):
    """The action whose components are (dx, dy, fire): dx = right - left, dy = down - up."""
    for a in range(NUM_ACTIONS):
        if (((RIGHT_MASK >> a) & 1) - ((LEFT_MASK >> a) & 1) == dx
                and ((DOWN_MASK >> a) & 1) - ((UP_MASK >> a) & 1) == dy
                and (FIRE_MASK >> a) & 1 == int(bool(fire))):
            return a
    raise ValueError((dx, dy, fire))


def initial_game(n_envs, seed=0):
    """[E,16] int32 rows of fresh episodes; env e's generator starts at seed*1000 + e."""
    g = np.zeros((int(n_envs), ROW_INTS), np.int32)
    g[:, AX], g[:, AY], g[:, OX], g[:, OY] = AX0, AY0, OX0, OY0
    rng = (np.int64(seed) * 1000 + np.arange(n_envs, dtype=np.int64)) & 0xFFFFFFFF
    g[:, RNG] = rng.astype(np.uint32).view(np.int32)
    return g


def _clamp(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi)


def _pts(ax, ay, ox, oy):
    gx, gy = np.abs(ax - ox), np.abs(ay - oy)
    return np.where((gy > REACH_Y) | (gx > REACH_FAR), 0, np.where(gx <= REACH_NEAR, 2, 1))


def step_numpy(game, actions, limit=DEFAULT_LIMIT):
    """One step of every row of `game` ([E,16] int32, updated in place) under `actions` [E].
    Returns (reward float64 [E], over bool [E], ep_score int32 [E], 0 where not over)."""
    E = game.shape[0]
    a = np.asarray(actions).astype(np.int64).reshape(E)
    g = game.astype(np.int64)
    ax, ay, ox, oy, a_cd, o_cd, a_score, o_score, t = (g[:, i].copy() for i in range(9))
    rng = g[:, RNG] & 0xFFFFFFFF
    reward = np.zeros(E, np.int64)

    sh = np.where((a >= 0) & (a < NUM_ACTIONS), a, NOOP)
    up, down, right, left, fire = (((m >> sh) & 1) for m in
                                   (UP_MASK, DOWN_MASK, RIGHT_MASK, LEFT_MASK, FIRE_MASK))
    dx, dy = right - left, down - up
    a_cd = np.maximum(a_cd - 1, 0)
    o_cd = np.maximum(o_cd - 1, 0)
    rng = (rng * LCG_A + LCG_C) & 0xFFFFFFFF
    r = rng >> 16
    ax = _clamp(ax + AGENT_STEP * dx, X_MIN, X_MAX)
    ay = _clamp(ay + AGENT_STEP * dy, Y_MIN, Y_MAX)
    s, gap = np.sign(ax - ox), np.abs(ax - ox)
    close_dx = np.where(gap > CLOSE_FAR, s, np.where(gap < CLOSE_NEAR, np.where(s != 0, -s, 1), 0))
    chase = (r & 3) != 0
    odx = np.where(chase, close_dx, ((r >> 2) % 3) - 1)
    ody = np.where(chase, np.sign(ay - oy), ((r >> 4) % 3) - 1)
    ox = _clamp(ox + OPP_STEP * odx, X_MIN, X_MAX)
    oy = _clamp(oy + OPP_STEP * ody, Y_MIN, Y_MAX)

    punch = (fire == 1) & (a_cd == 0)
    a_cd = np.where(punch, COOLDOWN, a_cd)
    p = np.where(punch, _pts(ax, ay, ox, oy), 0)
    reward += p
    a_score = a_score + p
    ox = np.where(p > 0, _clamp(ox + np.where(ox >= ax, KNOCK, -KNOCK), X_MIN, X_MAX), ox)

    q = _pts(ax, ay, ox, oy)
    counter = (o_cd == 0) & (((r >> 8) & 1) == 0) & (q > 0)
    o_cd = np.where(counter, COOLDOWN, o_cd)
    q = np.where(counter, q, 0)
    reward -= q
    o_score = o_score + q
    ax = np.where(counter, _clamp(ax + np.where(ax > ox, KNOCK, -KNOCK), X_MIN, X_MAX), ax)

    t = t + 1
    over = (a_score >= KO) | (o_score >= KO) | (t >= CLOCK) | (t >= int(limit))
    ep_score = np.where(over, a_score - o_score, 0).astype(np.int32)

    fresh = (AX0, AY0, OX0, OY0, 0, 0, 0, 0, 0)
    cols = (ax, ay, ox, oy, a_cd, o_cd, a_score, o_score, t)
    for i, (v, f) in enumerate(zip(cols, fresh)):
        game[:, i] = np.where(over, f, v).astype(np.int32)
    game[:, RNG] = rng.astype(np.uint32).view(np.int32)
    game[:, RNG + 1:] = 0
    return reward.astype(np.float64), over, ep_score


def render_numpy(game):
    """[E,84,84] uint8 frames of the rows of `game`, painted in reverse priority order: ring,
    clock, score bars, opponent (arm, body), agent (arm, body)."""
    g = np.asarray(game).astype(np.int64)
    E = g.shape[0]
    x = np.arange(W).reshape(1, 1, W)
    y = np.arange(H).reshape(1, H, 1)
    col = lambda i: g[:, i].reshape(E, 1, 1)
    ax, ay, ox, oy = col(AX), col(AY), col(OX), col(OY)
    frame = np.zeros((E, H, W), np.uint8)

    def paint(mask, shade):
        frame[np.broadcast_to(mask, frame.shape)] = shade

    def box(x0, y0, w, h):
        return (x >= x0) & (x < x0 + w) & (y >= y0) & (y < y0 + h)

    in_x, in_y = (x >= RING_X0) & (x <= RING_X1), (y >= RING_Y0) & (y <= RING_Y1)
    paint((((y == RING_Y0) | (y == RING_Y1)) & in_x) | (((x == RING_X0) | (x == RING_X1)) & in_y), DIM)
    paint((y == CLOCK_Y) & (x < W - col(T) // CLOCK_DIV), DIM)
    paint((y >= O_BAR_Y) & (y < O_BAR_Y + 2) & (x >= W - col(O_SCORE) // 2), OPP_SHADE)
    paint((y >= A_BAR_Y) & (y < A_BAR_Y + 2) & (x < col(A_SCORE) // 2), AGENT_SHADE)
    o_arm_x = np.where(ox >= ax, ox - ARM_W, ox + BODY_W)         # the opponent faces left
    paint((col(O_CD) >= ARM_CD) & box(o_arm_x, oy + ARM_ROW, ARM_W, ARM_H), OPP_SHADE)
    paint(box(ox, oy, BODY_W, BODY_H), OPP_SHADE)
    a_arm_x = np.where(ax <= ox, ax + BODY_W, ax - ARM_W)         # the agent faces right
    paint((col(A_CD) >= ARM_CD) & box(a_arm_x, ay + ARM_ROW, ARM_W, ARM_H), AGENT_SHADE)
    paint(box(ax, ay, BODY_W, BODY_H), AGENT_SHADE)
    return frame


class BoxingVec(GameVec):
    """E GridBoxing simulators in HBM (ba3c_amd.gamevec.GameVec), BreakoutVec's interface: every
    step is one HIP launch (ba3c_boxing_step), or with `frame_skip` / `sticky` one decision of
    ba3c_amd.frameskip (ba3c_boxing_step_skip, aux rows in `aux`)."""

    A = NUM_ACTIONS
    PALETTE = PALETTE
    STEP, DECIDE = "ba3c_boxing_step", "ba3c_boxing_step_skip"
    RENDER, VIEW = "ba3c_boxing_render", "ba3c_boxing_view"
    initial_game = staticmethod(initial_game)
