// ba3c_breakout.h — GridBreakout: a small integer-only Breakout for a vector of simulators,
// stepped, rendered and pushed into the frame history in ONE launch.  It stands where the
// reference has GymEnv + the 84x84 resize + HistoryFramePlayer (RL/gymenv.py, RL/history.py:
// 12-55, OpenAIGym/train.py:113-128).  The rules are stated once in ba3c_amd/breakout.py
// (constants, step_numpy, render_numpy: the oracle of this kernel); this file restates them.
//
// game[e] = [px, bx, by, vx, vy, in_play, lives, score, t, rng, b0..b5], 16 int32 = 64 bytes.
//
// The launch is sim_kernel<SoloSim<BreakoutRules>, .> (ba3c_envkernel.h: one 256-thread workgroup per
// simulator, the skeleton GridBoxing shares); this file holds the game's step and pixel rules.
#pragma once
#include "ba3c_envkernel.h"

namespace ba3c {

constexpr int BK_ROWS = 6, BK_COLS = 14, BK_BRICK_W = 6, BK_BRICK_H = 3, BK_BRICK_Y0 = 18;
constexpr int BK_PADDLE_Y = 78, BK_PADDLE_W = 12, BK_PX_MAX = 72, BK_LIVES = 5;
constexpr int32_t BK_FULL_ROW = 0x3FFF;

struct BreakoutGame {
  int32_t px, bx, by, vx, vy, in_play, lives, score, t;
  uint32_t rng;
  int32_t b0, b1, b2, b3, b4, b5;   // named, not an array: r is never a compile-time constant
};

__device__ __forceinline__ int32_t bk_row_value(int r) { return r < 2 ? 7 : (r < 4 ? 4 : 1); }

// b_r by selects: a dynamically indexed private array would be placed in LDS or scratch
__device__ __forceinline__ int32_t bk_row_mask(const BreakoutGame& g, int r) {
  return r == 0 ? g.b0 : r == 1 ? g.b1 : r == 2 ? g.b2 : r == 3 ? g.b3 : r == 4 ? g.b4 : g.b5;
}

__device__ __forceinline__ void bk_clear_brick(BreakoutGame& g, int r, int c) {
  const int32_t keep = ~(1 << c);
  g.b0 &= r == 0 ? keep : -1;
  g.b1 &= r == 1 ? keep : -1;
  g.b2 &= r == 2 ? keep : -1;
  g.b3 &= r == 3 ? keep : -1;
  g.b4 &= r == 4 ? keep : -1;
  g.b5 &= r == 5 ? keep : -1;
}

// One step of the rules (breakout.py: step_numpy).  Returns the reward; *over_out / *ep_out as
// the entry point documents them.  `a` is compared, never used as an index.
__device__ __forceinline__ int32_t bk_step(BreakoutGame& g, int64_t a, int32_t limit, bool* over_out,
                                           int32_t* ep_out) {
  int32_t reward = 0;
  if (a == 2) g.px = min(g.px + 3, BK_PX_MAX);
  else if (a == 3) g.px = max(g.px - 3, 0);
  if (!g.in_play) {
    if (a == 1) {
      g.rng = g.rng * 1664525u + 1013904223u;
      g.bx = 8 + (int32_t)((g.rng >> 16) % 68u);
      g.by = 40;
      g.vx = ((g.rng >> 8) & 1u) ? 1 : -1;
      g.vy = 2;
      g.in_play = 1;
    }
  } else {
    int nx = g.bx + g.vx, ny = g.by + g.vy;
    if (nx < 0) { nx = -nx; g.vx = -g.vx; }
    else if (nx > 82) { nx = 164 - nx; g.vx = -g.vx; }
    if (ny < 0) { ny = -ny; g.vy = -g.vy; }
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cx = nx + (k & 1), cy = ny + (k >> 1);
      if (!hit && cy >= BK_BRICK_Y0 && cy < BK_BRICK_Y0 + BK_ROWS * BK_BRICK_H) {
        const int r = (cy - BK_BRICK_Y0) / BK_BRICK_H;
        const int c = (cx / BK_BRICK_W) & 31;
        if ((bk_row_mask(g, r) >> c) & 1) {
          bk_clear_brick(g, r, c);
          reward += bk_row_value(r);
          hit = true;
        }
      }
    }
    if (hit) { g.vy = -g.vy; ny = g.by; }
    if (g.vy > 0 && g.by + 1 < BK_PADDLE_Y && ny + 1 >= BK_PADDLE_Y && nx + 1 >= g.px &&
        nx <= g.px + BK_PADDLE_W - 1) {
      ny = BK_PADDLE_Y - 2;
      g.vy = -2;
      const int d = nx + 1 - (g.px + BK_PADDLE_W / 2);
      g.vx = d < -3 ? -2 : (d < 0 ? -1 : (d < 3 ? 1 : 2));
    }
    g.bx = nx;
    g.by = ny;
    if (g.by > 82) { g.in_play = 0; g.lives -= 1; }
  }
  g.score += reward;
  g.t += 1;
  const int32_t any = g.b0 | g.b1 | g.b2 | g.b3 | g.b4 | g.b5;
  const bool over = g.lives == 0 || any == 0 || g.t >= limit;
  *over_out = over;
  *ep_out = g.score;
  if (over) {
    g.px = 36;
    g.bx = g.by = g.vx = g.vy = g.in_play = 0;
    g.lives = BK_LIVES;
    g.score = 0;
    g.t = 0;
    g.b0 = g.b1 = g.b2 = g.b3 = g.b4 = g.b5 = BK_FULL_ROW;
  }
  return reward;
}

// breakout.py: render_numpy, for pixel (y, x); `bricks` / `shade` are row y's brick mask and
// shade (0 outside the brick band), hoisted by the caller because a group shares its row.
__device__ __forceinline__ uint32_t bk_pixel(const BreakoutGame& g, int y, int x, int32_t bricks,
                                             uint32_t shade) {
  if (g.in_play && (unsigned)(x - g.bx) < 2u && (unsigned)(y - g.by) < 2u) return 255u;
  if ((unsigned)(y - BK_PADDLE_Y) < 2u && (unsigned)(x - g.px) < (unsigned)BK_PADDLE_W) return 255u;
  if ((bricks >> (x / BK_BRICK_W)) & 1) return shade;
  if ((unsigned)(y - 2) < 2u && (x & 3) < 2 && (x >> 2) < g.lives) return 128u;
  return 0u;
}

// The game as ba3c_envkernel.h's sim_kernel takes it.
struct BreakoutRules {
  using Game = BreakoutGame;
  struct Row {
    int32_t bricks;   // row y's brick mask, 0 outside the brick band
    uint32_t shade;
  };
  static __device__ __forceinline__ void load(Game& g, int4 r0, int4 r1, int4 r2, int4 r3) {
    g.px = r0.x; g.bx = r0.y; g.by = r0.z; g.vx = r0.w;
    g.vy = r1.x; g.in_play = r1.y; g.lives = r1.z; g.score = r1.w;
    g.t = r2.x; g.rng = (uint32_t)r2.y; g.b0 = r2.z; g.b1 = r2.w;
    g.b2 = r3.x; g.b3 = r3.y; g.b4 = r3.z; g.b5 = r3.w;
  }
  static __device__ __forceinline__ void store(const Game& g, int4* out) {
    out[0] = make_int4(g.px, g.bx, g.by, g.vx);
    out[1] = make_int4(g.vy, g.in_play, g.lives, g.score);
    out[2] = make_int4(g.t, (int32_t)g.rng, g.b0, g.b1);
    out[3] = make_int4(g.b2, g.b3, g.b4, g.b5);
  }
  static __device__ __forceinline__ int32_t step(Game& g, int64_t a, int32_t limit, bool* over_out,
                                                 int32_t* ep_out) {
    return bk_step(g, a, limit, over_out, ep_out);
  }
  static __device__ __forceinline__ Row row(const Game& g, int y) {
    Row rw{0, 0u};
    if ((unsigned)(y - BK_BRICK_Y0) < (unsigned)(BK_ROWS * BK_BRICK_H)) {
      const int r = (y - BK_BRICK_Y0) / BK_BRICK_H;
      rw.bricks = bk_row_mask(g, r);
      rw.shade = 230u - 30u * (uint32_t)r;
    }
    return rw;
  }
  static __device__ __forceinline__ uint32_t pixel(const Game& g, int y, int x, const Row& rw) {
    return bk_pixel(g, y, x, rw.bricks, rw.shade);
  }
};

}  // namespace ba3c
