"""GridPong: a small integer-only Pong that lives on the GPU (`-e GridPong-v0`).

The third on-device game next to GridBreakout (ba3c_amd.breakout) and GridBoxing
(ba3c_amd.boxing): a rally game against a tracking opponent with rewards of +1 / -1 per point, an
episode score in [-21, 21] and a long horizon between a decision and its reward.  This module
holds the rules ONCE: the constants, `step_numpy` / `render_numpy` (a vectorised CPU statement,
the oracle of the HIP kernel in csrc/ba3c_gridpong.h) and `PongVec`, E simulators on the device
with BreakoutVec's interface.  `ba3c_amd.envs.PongPlayer` restates the same rules as scalar
Python ints for the simulator processes; tests hold the three statements equal bit for bit.

State: `game[e] = [py, oy, bx, by, vx, vy, mine, theirs, t, rng, hits, serve, 0, 0, 0, 0]`,
16 int32; the four padding ints are written as 0.
py / oy: top row of the agent's / the opponent's paddle, in pixels, in [12, 72].  A paddle is
2 px wide and 10 px tall; the agent's covers x in [76, 78) (the right side, as in ALE), the
opponent's x in [6, 8).  (bx, by): the top-left of the 2x2 px ball in EIGHTHS of a pixel (it is
drawn at (bx >> 3, by >> 3)); (vx, vy): its velocity in eighths of a pixel per step.  mine /
theirs: the points of the episode; t: its steps; rng: the LCG's uint32 bits; hits: the paddle
hits of the rally; serve: the steps until the ball is served (0: the ball is in play).
The court: walls in rows 10..11 and 82..83, so the ball's top row stays in [12, 80]
(by in [96, 640]).
Fresh episode: py = oy = 42, (bx, by) = (328, 368), (vx, vy) = (+10, 0) (the first serve goes to
the agent), scores, t and hits zero, serve = 16; rng is kept.

Actions: ALE Pong's 6.  0 NOOP, 1 FIRE, 2 RIGHT (the paddle moves up), 3 LEFT (down),
4 RIGHTFIRE, 5 LEFTFIRE; any other value is NOOP.  An action is range-checked and then tested
against the three component masks UP / DOWN / FIRE (`(MASK >> a) & 1`); it never indexes memory.

step(a), in exactly this order:

    reward = 0
    rng = (rng * 1664525 + 1013904223) mod 2^32; r = rng >> 16          # the step's ONE draw
    py = clamp(py + 2 * (down - up), 12, 72)
    target = (by >> 3) + 1 if serve == 0 else 47                        # the ball's centre row
    ody = 0 if (r & 7) < 2 else clamp(target - (oy + 5), -1, 1)         # 2 steps in 8: a lapse
    oy = clamp(oy + ody, 12, 72)
    if serve > 0:
        serve -= 1
        if fire or serve == 0:                                          # the serve
            serve = 0; k = (r >> 3) & 7; m = 1 + ((r >> 6) & 1)
            by, vy = ((33 + k) << 3, -m) if (r >> 7) & 1 else ((59 - k) << 3, +m)
    else:
        nx = bx + vx; ny = by + vy
        if ny < 96: ny = 192 - ny; vy = -vy                             # the walls
        elif ny > 640: ny = 1280 - ny; vy = -vy
        b = ny >> 3
        if vx > 0 and bx + 16 <= 608 < nx + 16 and 0 <= b - py + 1 <= 10:      # the agent's face
            d = b - py + 1; nx = 1184 - nx; hit = -1
        elif vx < 0 and nx < 64 <= bx and 0 <= b - oy + 1 <= 10:               # the opponent's
            d = b - oy + 1; nx = 128 - nx; hit = +1
        if hit:
            hits += 1; vx = hit * min(10 + 2 * (hits >> 2), 14)
            vy = (VY_TABLE >> 4d) & 15, negative if d < 5
        bx, by = nx, ny
        if bx >= 624: theirs += 1; reward = -1; vx = +10                # past the agent
        elif bx <= 32: mine += 1; reward = +1; vx = -10                 # past the opponent
        if reward: (bx, by) = (328, 368); vy = 0; hits = 0; serve = 16  # served to the loser
    t += 1
    over = mine >= 21 or theirs >= 21 or t >= limit
    ep_score = mine - theirs                                            # in [-21, 21]
    if over: reset to a fresh episode (rng kept)

VY_TABLE holds |vy| for d = 0..10, four bits each: 12, 9, 6, 4, 2, 1, 2, 4, 6, 9, 12.  |vx| is
10 for the first four hits of a rally, 12 for the next four and 14 after that: below the 16
eighths of a paddle's thickness, so the ball never crosses one in a step.  A serve leaves the
centre line just above or below the centre rows, moving outward, and reaches the far side after
27 steps at row 40 at most (52 at least): a paddle left at the centre (rows 42..51) does not
meet it, as in ALE, and the opponent reaches it from the centre it returns to while it waits.

render: pixel (y, x) takes the first match of: the agent's paddle (255) or, in rows 2..3, the
agent's score bar x < 4 * mine (255); the ball while serve == 0 (255); the opponent's paddle
(130) or, in rows 5..6, the opponent's score bar x >= 84 - 4 * theirs (130); the walls, rows
10..11 and 82..83 (60); the net, x in 41..42 in rows 12..81 where (y - 12) & 4 == 0 (60); else 0.
The bars lie in rows no moving object reaches.  The frame a step returns is the frame AFTER the
step, so on `over` it is the new episode's first frame (as in the other games).
"""
import numpy as np

from .gamevec import GameVec

H = W = 84
SUB = 3                                  # positions and velocities are in 1 / 8 px
PADDLE_W, PADDLE_H, PADDLE_STEP, OPP_STEP = 2, 10, 2, 1
AGENT_X, OPP_X = 76, 6                   # the paddles' left columns
Y_MIN, Y_MAX = 12, 72                    # a paddle's top row
PY0 = 42
BALL = 2
BY_MIN, BY_MAX = 12 << SUB, 80 << SUB    # the ball's top, in eighths
AGENT_FACE, OPP_FACE = AGENT_X << SUB, (OPP_X + PADDLE_W) << SUB          # 608, 64
AGENT_PAST, OPP_PAST = (AGENT_X + PADDLE_W) << SUB, (OPP_X << SUB) - (BALL << SUB)   # 624, 32
BX0, BY0 = 41 << SUB, 46 << SUB          # 328, 368
CENTRE_ROW = 47
V0, V_STEP, V_CAP, HITS_SHIFT = 10, 2, 14, 2
VY_MAGS = (12, 9, 6, 4, 2, 1, 2, 4, 6, 9, 12)
VY_TABLE = sum(m << (4 * d) for d, m in enumerate(VY_MAGS))
LAPSE_OF_8 = 2                           # the opponent holds still while (r & 7) < 2
SERVE_DELAY = 16
SERVE_TOP, SERVE_BOTTOM = 33, 59         # serve rows 33 + k / 59 - k, k in 0..7
WIN = 21
AGENT_SHADE, OPP_SHADE, DIM = 255, 130, 60
A_BAR_Y, O_BAR_Y, BAR_UNIT = 2, 5, 4
WALL_TOP, WALL_BOTTOM = 10, 82           # two rows each
NET_X, NET_W = 41, 2
NUM_ACTIONS = 6
NOOP, FIRE, UP, DOWN, UPFIRE, DOWNFIRE = range(6)     # ALE: RIGHT is up, LEFT is down
ACTIONS = ("NOOP", "FIRE", "RIGHT", "LEFT", "RIGHTFIRE", "LEFTFIRE")
UP_SET, DOWN_SET, FIRE_SET = (2, 4), (3, 5), (1, 4, 5)
UP_MASK, DOWN_MASK, FIRE_MASK = (sum(1 << i for i in s) for s in (UP_SET, DOWN_SET, FIRE_SET))
LCG_A, LCG_C = 1664525, 1013904223
DEFAULT_LIMIT = 40000                    # LimitLengthPlayer(40000), train.py:127
# column indices of a game row
PY, OY, BX, BY, VX, VY, MINE, THEIRS, T, RNG, HITS, SERVE = range(12)
ROW_INTS = 16
FRESH = (PY0, PY0, BX0, BY0, V0, 0, 0, 0, 0, None, 0, SERVE_DELAY)        # None: rng is kept
# the colour of every shade for ba3c_amd.view: grey (i, i, i) except the shades render draws
COLOURS = {0: (144, 72, 17), AGENT_SHADE: (92, 186, 92), OPP_SHADE: (213, 130, 74),
           DIM: (236, 236, 236)}
PALETTE = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
for _shade, _rgb in COLOURS.items():
    PALETTE[_shade] = _rgb
PALETTE.setflags(write=False)


def initial_game(n_envs, seed=0):
    """[E,16] int32 rows of fresh episodes; env e's generator starts at seed*1000 + e."""
    g = np.zeros((int(n_envs), ROW_INTS), np.int32)
    for i, v in enumerate(FRESH):
        if v is not None:
            g[:, i] = v
    rng = (np.int64(seed) * 1000 + np.arange(n_envs, dtype=np.int64)) & 0xFFFFFFFF
    g[:, RNG] = rng.astype(np.uint32).view(np.int32)
    return g


def _clamp(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi)


def step_numpy(game, actions, limit=DEFAULT_LIMIT):
    """One step of every row of `game` ([E,16] int32, updated in place) under `actions` [E].
    Returns (reward float64 [E], over bool [E], ep_score int32 [E], 0 where not over)."""
    E = game.shape[0]
    a = np.asarray(actions).astype(np.int64).reshape(E)
    g = game.astype(np.int64)
    py, oy, bx, by, vx, vy, mine, theirs, t = (g[:, i].copy() for i in range(9))
    hits, serve = g[:, HITS].copy(), g[:, SERVE].copy()
    rng = g[:, RNG] & 0xFFFFFFFF

    sh = np.where((a >= 0) & (a < NUM_ACTIONS), a, NOOP)
    up, down, fire = (((m >> sh) & 1) for m in (UP_MASK, DOWN_MASK, FIRE_MASK))
    rng = (rng * LCG_A + LCG_C) & 0xFFFFFFFF
    r = rng >> 16
    py = _clamp(py + PADDLE_STEP * (down - up), Y_MIN, Y_MAX)
    waiting = serve > 0
    target = np.where(waiting, CENTRE_ROW, (by >> SUB) + 1)
    ody = np.where((r & 7) < LAPSE_OF_8, 0, _clamp(target - (oy + PADDLE_H // 2), -OPP_STEP, OPP_STEP))
    oy = _clamp(oy + ody, Y_MIN, Y_MAX)

    # waiting rows: count down, serve on FIRE or at 0
    serve = np.where(waiting, serve - 1, serve)
    now = waiting & ((fire == 1) | (serve == 0))
    k, m = (r >> 3) & 7, 1 + ((r >> 6) & 1)
    top = ((r >> 7) & 1) == 1
    serve = np.where(now, 0, serve)
    s_by = np.where(top, (SERVE_TOP + k) << SUB, (SERVE_BOTTOM - k) << SUB)
    s_vy = np.where(top, -m, m)

    # rows in play: move, walls, paddles, points
    nx, ny = bx + vx, by + vy
    lo_wall, hi_wall = ny < BY_MIN, ny > BY_MAX
    ny = np.where(lo_wall, 2 * BY_MIN - ny, np.where(hi_wall, 2 * BY_MAX - ny, ny))
    wvy = np.where(lo_wall | hi_wall, -vy, vy)
    b = ny >> SUB
    da, do = b - py + 1, b - oy + 1
    edge = BALL << SUB
    hit_a = (vx > 0) & (bx + edge <= AGENT_FACE) & (nx + edge > AGENT_FACE) & (da >= 0) & (da <= PADDLE_H)
    hit_o = (vx < 0) & (bx >= OPP_FACE) & (nx < OPP_FACE) & (do >= 0) & (do <= PADDLE_H)
    hit = hit_a | hit_o
    d = np.where(hit_a, da, np.where(hit_o, do, 0))
    nx = np.where(hit_a, 2 * (AGENT_FACE - edge) - nx, np.where(hit_o, 2 * OPP_FACE - nx, nx))
    hits_p = np.where(hit, hits + 1, hits)
    speed = np.minimum(V0 + V_STEP * (hits_p >> HITS_SHIFT), V_CAP)
    pvx = np.where(hit_a, -speed, np.where(hit_o, speed, vx))
    mag = (np.int64(VY_TABLE) >> (4 * d)) & 15
    pvy = np.where(hit, np.where(d < PADDLE_H // 2, -mag, mag), wvy)
    lost, won = nx >= AGENT_PAST, nx <= OPP_PAST
    point = lost | won
    reward = np.where(waiting, 0, np.where(lost, -1, np.where(won, 1, 0)))
    play = ~waiting
    theirs = theirs + (play & lost)
    mine = mine + (play & won)
    p_bx = np.where(point, BX0, nx)
    p_by = np.where(point, BY0, ny)
    p_vx = np.where(lost, V0, np.where(won, -V0, pvx))
    p_vy = np.where(point, 0, pvy)
    p_hits = np.where(point, 0, hits_p)
    p_serve = np.where(point, SERVE_DELAY, 0)

    bx = np.where(play, p_bx, bx)
    by = np.where(play, p_by, np.where(now, s_by, by))
    vx = np.where(play, p_vx, vx)
    vy = np.where(play, p_vy, np.where(now, s_vy, vy))
    hits = np.where(play, p_hits, hits)
    serve = np.where(play, p_serve, serve)

    t = t + 1
    over = (mine >= WIN) | (theirs >= WIN) | (t >= int(limit))
    ep_score = np.where(over, mine - theirs, 0).astype(np.int32)
    cols = {PY: py, OY: oy, BX: bx, BY: by, VX: vx, VY: vy, MINE: mine, THEIRS: theirs, T: t,
            HITS: hits, SERVE: serve}
    for i, v in cols.items():
        game[:, i] = np.where(over, FRESH[i], v).astype(np.int32)
    game[:, RNG] = rng.astype(np.uint32).view(np.int32)
    game[:, SERVE + 1:] = 0
    return reward.astype(np.float64), over, ep_score


def render_numpy(game):
    """[E,84,84] uint8 frames of the rows of `game`, painted in reverse priority order: net,
    walls, opponent (bar, paddle), ball, agent (bar, paddle)."""
    g = np.asarray(game).astype(np.int64)
    E = g.shape[0]
    x = np.arange(W).reshape(1, 1, W)
    y = np.arange(H).reshape(1, H, 1)
    col = lambda i: g[:, i].reshape(E, 1, 1)
    frame = np.zeros((E, H, W), np.uint8)

    def paint(mask, shade):
        frame[np.broadcast_to(mask, frame.shape)] = shade

    def box(x0, y0, w, h):
        return (x >= x0) & (x < x0 + w) & (y >= y0) & (y < y0 + h)

    court = (y >= WALL_TOP + 2) & (y < WALL_BOTTOM)
    paint(court & (((y - (WALL_TOP + 2)) & 4) == 0) & (x >= NET_X) & (x < NET_X + NET_W), DIM)
    paint(((y >= WALL_TOP) & (y < WALL_TOP + 2)) | ((y >= WALL_BOTTOM) & (y < WALL_BOTTOM + 2)), DIM)
    paint((y >= O_BAR_Y) & (y < O_BAR_Y + 2) & (x >= W - BAR_UNIT * col(THEIRS)), OPP_SHADE)
    paint(box(OPP_X, col(OY), PADDLE_W, PADDLE_H), OPP_SHADE)
    paint((col(SERVE) == 0) & box(col(BX) >> SUB, col(BY) >> SUB, BALL, BALL), AGENT_SHADE)
    paint((y >= A_BAR_Y) & (y < A_BAR_Y + 2) & (x < BAR_UNIT * col(MINE)), AGENT_SHADE)
    paint(box(AGENT_X, col(PY), PADDLE_W, PADDLE_H), AGENT_SHADE)
    return frame


class PongVec(GameVec):
    """E GridPong simulators in HBM (ba3c_amd.gamevec.GameVec), BreakoutVec's interface: every
    step is one HIP launch (ba3c_gridpong_step), or with `frame_skip` / `sticky` one decision of
    ba3c_amd.frameskip (ba3c_gridpong_step_skip, aux rows in `aux`)."""

    A = NUM_ACTIONS
    PALETTE = PALETTE
    STEP, DECIDE = "ba3c_gridpong_step", "ba3c_gridpong_step_skip"
    RENDER, VIEW = "ba3c_gridpong_render", "ba3c_gridpong_view"
    initial_game = staticmethod(initial_game)
