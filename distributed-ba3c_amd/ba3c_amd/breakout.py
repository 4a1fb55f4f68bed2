"""GridBreakout: a small integer-only Breakout that lives on the GPU (`-e GridBreakout-v0`).

gym/ALE are absent here, so this game stands where the reference has GymEnv + the 84x84 resize
(RL/gymenv.py, OpenAIGym/train.py:113-128).  This module holds the rules ONCE: the constants,
`step_numpy` / `render_numpy` (a vectorised CPU statement, the oracle of the HIP kernel in
csrc/ba3c_breakout.h) and `BreakoutVec`, E simulators on the device with SyntheticAtari's
interface.  `ba3c_amd.envs.BreakoutPlayer` restates the same rules as scalar Python ints for
the simulator processes; tests hold the three statements equal bit for bit.

State: `game[e] = [px, bx, by, vx, vy, in_play, lives, score, t, rng, b0..b5]`, 16 int32.
Frame: 84x84 grayscale uint8.  Bricks: 6 rows x 14 columns of 6x3 px, brick (r, c) covering
x in [6c, 6c+6), y in [18+3r, 21+3r); b_r bit c = alive.  Paddle: 12x2 px at y in {78, 79},
x in [px, px+12), px in [0, 72].  Ball: 2x2 px, top-left (bx, by).  5 lives per episode.
Actions: 0 NOOP, 1 FIRE, 2 RIGHT, 3 LEFT; any other value is NOOP.

step(a), in exactly this order:

    reward = 0
    if a == 2: px = min(px + 3, 72)
    elif a == 3: px = max(px - 3, 0)
    if not in_play:
        if a == 1:
            rng = (rng * 1664525 + 1013904223) mod 2^32
            bx = 8 + ((rng >> 16) % 68); by = 40
            vx = +1 if (rng >> 8) & 1 else -1; vy = 2; in_play = 1
    else:
        nx = bx + vx; ny = by + vy
        if nx < 0: nx = -nx; vx = -vx
        elif nx > 82: nx = 164 - nx; vx = -vx
        if ny < 0: ny = -ny; vy = -vy
        for (cx, cy) in ((nx,ny), (nx+1,ny), (nx,ny+1), (nx+1,ny+1)):     # first hit only
            if 18 <= cy < 36:
                r = (cy - 18) // 3; c = cx // 6
                if (b_r >> c) & 1:
                    b_r &= ~(1 << c); reward += VAL[r]; vy = -vy; ny = by; break
        if vy > 0 and by + 1 < 78 and ny + 1 >= 78 and nx + 1 >= px and nx <= px + 11:
            ny = 76; vy = -2; d = nx + 1 - (px + 6)
            vx = -2 if d < -3 else -1 if d < 0 else 1 if d < 3 else 2
        bx, by = nx, ny
        if by > 82: in_play = 0; lives -= 1
    score += reward; t += 1
    over = (lives == 0) or (all b_r == 0) or (t >= limit)
    if over: ep_score = score; reset (px=36, ball and score and t zero, lives=5, bricks full;
                                      rng is kept)

render: pixel (y, x) takes the first match of: ball (in_play, 255), paddle (255), live brick
(its row shade), lives bar (y in {2,3}, x in [4i, 4i+2) for i < lives, 128), else 0.  The frame
a step returns is the frame AFTER the step, so on `over` it is the new episode's first frame
(GymEnv's auto-restart; what HistoryFramePlayer / ba3c_history_push expect).
"""
import numpy as np

from .gamevec import GameVec

H = W = 84
ROWS, COLS = 6, 14
BRICK_W, BRICK_H, BRICK_Y0 = 6, 3, 18
FULL_ROW = 0x3FFF
VAL = (7, 7, 4, 4, 1, 1)
SHADE = (230, 200, 170, 140, 110, 80)
PADDLE_Y, PADDLE_W, PADDLE_H, PX_MAX, PX_START, PADDLE_STEP = 78, 12, 2, 72, 36, 3
BALL = 2
LIVES = 5
LIVES_Y, LIVES_SHADE = 2, 128
NOOP, FIRE, RIGHT, LEFT = 0, 1, 2, 3
NUM_ACTIONS = 4
MAX_SCORE = COLS * sum(VAL)          # 336
LCG_A, LCG_C = 1664525, 1013904223
DEFAULT_LIMIT = 40000                # LimitLengthPlayer(40000), train.py:127
# column indices of a game row
PX, BX, BY, VX, VY, IN_PLAY, N_LIVES, SCORE, T, RNG, B0 = range(11)
ROW_INTS = 16
# the colour of every shade for ba3c_amd.view: grey (i, i, i) except the shades render draws
COLOURS = {0: (0, 0, 0), 255: (236, 236, 236), LIVES_SHADE: (214, 214, 64),
           230: (200, 72, 72), 200: (198, 108, 58), 170: (180, 122, 48),
           140: (162, 162, 42), 110: (72, 160, 72), 80: (66, 72, 200)}
PALETTE = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
for _shade, _rgb in COLOURS.items():
    PALETTE[_shade] = _rgb
PALETTE.setflags(write=False)


def initial_game(n_envs, seed=0):
    """[E,16] int32 rows of fresh episodes; env e's serve generator starts at seed*1000 + e."""
    g = np.zeros((int(n_envs), ROW_INTS), np.int32)
    g[:, PX] = PX_START
    g[:, N_LIVES] = LIVES
    g[:, B0:B0 + ROWS] = FULL_ROW
    rng = (np.int64(seed) * 1000 + np.arange(n_envs, dtype=np.int64)) & 0xFFFFFFFF
    g[:, RNG] = rng.astype(np.uint32).view(np.int32)
    return g


def step_numpy(game, actions, limit=DEFAULT_LIMIT):
    """One step of every row of `game` ([E,16] int32, updated in place) under `actions` [E].
    Returns (reward float64 [E], over bool [E], ep_score int32 [E], 0 where not over)."""
    E = game.shape[0]
    a = np.asarray(actions).astype(np.int64).reshape(E)
    ar = np.arange(E)
    g = game.astype(np.int64)
    px, bx, by, vx, vy, inp, lives, score, t = (g[:, i].copy() for i in range(9))
    rng = g[:, RNG] & 0xFFFFFFFF
    b = g[:, B0:B0 + ROWS].copy()
    reward = np.zeros(E, np.int64)

    px = np.where(a == RIGHT, np.minimum(px + PADDLE_STEP, PX_MAX),
                  np.where(a == LEFT, np.maximum(px - PADDLE_STEP, 0), px))
    playing = inp != 0
    serve = ~playing & (a == FIRE)
    rng = np.where(serve, (rng * LCG_A + LCG_C) & 0xFFFFFFFF, rng)

    # the ball's move, computed for every row and kept only where it was in play
    nx, ny = bx + vx, by + vy
    lo, hi = nx < 0, nx > 82
    nx = np.where(lo, -nx, np.where(hi, 164 - nx, nx))
    vx2 = np.where(lo | hi, -vx, vx)
    top = ny < 0
    ny = np.where(top, -ny, ny)
    vy2 = np.where(top, -vy, vy)
    hit = np.zeros(E, bool)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        cx, cy = nx + dx, ny + dy
        band = (cy >= BRICK_Y0) & (cy < BRICK_Y0 + ROWS * BRICK_H)
        r = np.clip((cy - BRICK_Y0) // BRICK_H, 0, ROWS - 1)
        c = np.clip(cx // BRICK_W, 0, COLS - 1)
        h = playing & ~hit & band & (((b[ar, r] >> c) & 1) == 1)
        b[ar[h], r[h]] &= ~(1 << c[h])
        reward += np.where(h, np.asarray(VAL, np.int64)[r], 0)
        hit |= h
    vy2 = np.where(hit, -vy2, vy2)
    ny = np.where(hit, by, ny)
    pad = ((vy2 > 0) & (by + 1 < PADDLE_Y) & (ny + 1 >= PADDLE_Y) & (nx + 1 >= px)
           & (nx <= px + PADDLE_W - 1))
    d = nx + 1 - (px + PADDLE_W // 2)
    ny = np.where(pad, PADDLE_Y - BALL, ny)
    vy2 = np.where(pad, -2, vy2)
    vx2 = np.where(pad, np.where(d < -3, -2, np.where(d < 0, -1, np.where(d < 3, 1, 2))), vx2)
    lost = playing & (ny > 82)

    bx = np.where(playing, nx, np.where(serve, 8 + ((rng >> 16) % 68), bx))
    by = np.where(playing, ny, np.where(serve, 40, by))
    vx = np.where(playing, vx2, np.where(serve, np.where((rng >> 8) & 1, 1, -1), vx))
    vy = np.where(playing, vy2, np.where(serve, 2, vy))
    inp = np.where(lost, 0, np.where(serve, 1, inp))
    lives = lives - lost
    score = score + reward
    t = t + 1
    over = (lives == 0) | (b == 0).all(axis=1) | (t >= int(limit))
    ep_score = np.where(over, score, 0).astype(np.int32)

    z = np.zeros_like(px)
    px = np.where(over, PX_START, px)
    bx, by, vx, vy, inp, score, t = (np.where(over, z, v) for v in (bx, by, vx, vy, inp, score, t))
    lives = np.where(over, LIVES, lives)
    b = np.where(over[:, None], FULL_ROW, b)
    for i, v in enumerate((px, bx, by, vx, vy, inp, lives, score, t)):
        game[:, i] = v.astype(np.int32)
    game[:, RNG] = rng.astype(np.uint32).view(np.int32)
    game[:, B0:B0 + ROWS] = b.astype(np.int32)
    return reward.astype(np.float64), over, ep_score


def render_numpy(game):
    """[E,84,84] uint8 frames of the rows of `game`, painted in reverse priority order:
    lives bar, bricks, paddle, ball."""
    g = np.asarray(game).astype(np.int64)
    E = g.shape[0]
    x = np.arange(W).reshape(1, W)
    col = lambda i: g[:, i].reshape(E, 1)
    frame = np.zeros((E, H, W), np.uint8)
    bar = (x % 4 < 2) & (x // 4 < col(N_LIVES))                                   # [E,W]
    frame[:, LIVES_Y:LIVES_Y + 2, :] = np.where(bar, LIVES_SHADE, 0)[:, None, :]
    alive = (g[:, B0:B0 + ROWS, None] >> np.arange(COLS)) & 1                     # [E,6,14]
    shade = (alive * np.asarray(SHADE).reshape(1, ROWS, 1)).astype(np.uint8)
    band = frame[:, BRICK_Y0:BRICK_Y0 + ROWS * BRICK_H, :]
    band[...] = np.repeat(np.repeat(shade, BRICK_H, axis=1), BRICK_W, axis=2)
    paddle = (x >= col(PX)) & (x < col(PX) + PADDLE_W)
    rows = frame[:, PADDLE_Y:PADDLE_Y + PADDLE_H, :]
    rows[...] = np.where(paddle[:, None, :], 255, rows)
    bxm = (col(IN_PLAY) != 0) & (x >= col(BX)) & (x < col(BX) + BALL)             # x = column
    bym = (x >= col(BY)) & (x < col(BY) + BALL)                                   # x = row (H == W)
    frame[bym[:, :, None] & bxm[:, None, :]] = 255
    return frame


class BreakoutVec(GameVec):
    """E GridBreakout simulators in HBM (ba3c_amd.gamevec.GameVec): every step is one HIP launch
    (ba3c_breakout_step).  A non-default `frame_skip` (K or an inclusive (lo, hi)) / `sticky` (a
    probability) makes every step one DECISION of ba3c_amd.frameskip (ba3c_breakout_step_skip)."""

    A = NUM_ACTIONS
    PALETTE = PALETTE
    STEP, DECIDE = "ba3c_breakout_step", "ba3c_breakout_step_skip"
    RENDER, VIEW = "ba3c_breakout_render", "ba3c_breakout_view"
    initial_game = staticmethod(initial_game)
