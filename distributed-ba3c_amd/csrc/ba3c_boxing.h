// ba3c_boxing.h — GridBoxing: a small integer-only Boxing for a vector of simulators: ALE's 18
// actions, a scripted opponent, rewards of both signs.  The rules are stated once in
// ba3c_amd/boxing.py (constants, step_numpy, render_numpy: the oracle of this kernel); this
// file restates them.
//
// game[e] = [ax, ay, ox, oy, a_cd, o_cd, a_score, o_score, t, rng, 0, 0, 0, 0, 0, 0],
// 16 int32 = 64 bytes; a* is the agent, o* the opponent.
//
// The launch is sim_kernel<SoloSim<BoxingRules>, .> (ba3c_envkernel.h: one 256-thread workgroup per
// simulator, the skeleton GridBreakout shares); this file holds the game's step and pixel rules.
#pragma once
#include "ba3c_envkernel.h"

namespace ba3c {

constexpr int BX_X_MIN = 4, BX_X_MAX = 74, BX_Y_MIN = 14, BX_Y_MAX = 70;
constexpr int BX_BODY_W = 6, BX_BODY_H = 8, BX_ARM_W = 4, BX_ARM_H = 2, BX_ARM_ROW = 3;
constexpr int BX_AX0 = 20, BX_AY0 = 42, BX_OX0 = 58, BX_OY0 = 42;
constexpr int BX_COOLDOWN = 8, BX_ARM_CD = 6, BX_KNOCK = 3, BX_KO = 100, BX_CLOCK = 1680;
// bit a of a mask: action a has that component (boxing.py: UP_SET .. FIRE_SET)
constexpr uint32_t BX_UP = 0x0C4C4u, BX_DOWN = 0x32320u, BX_RIGHT = 0x14948u, BX_LEFT = 0x29290u,
                   BX_FIRE = 0x3FC02u;

struct BoxingGame {
  int32_t ax, ay, ox, oy, a_cd, o_cd, a_score, o_score, t;
  uint32_t rng;
};

__device__ __forceinline__ int32_t bx_clamp(int32_t v, int32_t lo, int32_t hi) {
  return min(max(v, lo), hi);
}

__device__ __forceinline__ int32_t bx_sign(int32_t v) { return (v > 0) - (v < 0); }

__device__ __forceinline__ int32_t bx_pts(const BoxingGame& g) {
  const int32_t gx = abs(g.ax - g.ox), gy = abs(g.ay - g.oy);
  return (gy > 4 || gx > 14) ? 0 : (gx <= 9 ? 2 : 1);
}

// One step of the rules (boxing.py: step_numpy).  Returns the reward; *over_out / *ep_out as
// the entry point documents them.  `a` is range-checked and shifts the masks, never an index.
__device__ __forceinline__ int32_t bx_step(BoxingGame& g, int64_t a, int32_t limit, bool* over_out,
                                           int32_t* ep_out) {
  int32_t reward = 0;
  const uint32_t sh = (uint64_t)a < 18u ? (uint32_t)a : 0u;      // NOOP has no bit in any mask
  const int32_t dx = (int32_t)((BX_RIGHT >> sh) & 1u) - (int32_t)((BX_LEFT >> sh) & 1u);
  const int32_t dy = (int32_t)((BX_DOWN >> sh) & 1u) - (int32_t)((BX_UP >> sh) & 1u);
  const bool fire = (BX_FIRE >> sh) & 1u;
  g.a_cd = max(g.a_cd - 1, 0);
  g.o_cd = max(g.o_cd - 1, 0);
  g.rng = g.rng * 1664525u + 1013904223u;
  const uint32_t r = g.rng >> 16;
  g.ax = bx_clamp(g.ax + 2 * dx, BX_X_MIN, BX_X_MAX);
  g.ay = bx_clamp(g.ay + 2 * dy, BX_Y_MIN, BX_Y_MAX);
  int32_t odx, ody;
  if (r & 3u) {
    const int32_t s = bx_sign(g.ax - g.ox), gap = abs(g.ax - g.ox);
    ody = bx_sign(g.ay - g.oy);
    odx = gap > 11 ? s : (gap < 8 ? (s != 0 ? -s : 1) : 0);
  } else {
    odx = (int32_t)((r >> 2) % 3u) - 1;
    ody = (int32_t)((r >> 4) % 3u) - 1;
  }
  g.ox = bx_clamp(g.ox + odx, BX_X_MIN, BX_X_MAX);
  g.oy = bx_clamp(g.oy + ody, BX_Y_MIN, BX_Y_MAX);
  if (fire && g.a_cd == 0) {
    g.a_cd = BX_COOLDOWN;
    const int32_t p = bx_pts(g);
    if (p) {
      reward += p;
      g.a_score += p;
      g.ox = bx_clamp(g.ox + (g.ox >= g.ax ? BX_KNOCK : -BX_KNOCK), BX_X_MIN, BX_X_MAX);
    }
  }
  const int32_t p = bx_pts(g);                                    // after the knock-back above
  if (g.o_cd == 0 && ((r >> 8) & 1u) == 0u && p > 0) {
    g.o_cd = BX_COOLDOWN;
    reward -= p;
    g.o_score += p;
    g.ax = bx_clamp(g.ax + (g.ax > g.ox ? BX_KNOCK : -BX_KNOCK), BX_X_MIN, BX_X_MAX);
  }
  g.t += 1;
  const bool over = g.a_score >= BX_KO || g.o_score >= BX_KO || g.t >= BX_CLOCK || g.t >= limit;
  *over_out = over;
  *ep_out = g.a_score - g.o_score;
  if (over) {
    g.ax = BX_AX0; g.ay = BX_AY0; g.ox = BX_OX0; g.oy = BX_OY0;
    g.a_cd = g.o_cd = g.a_score = g.o_score = g.t = 0;
  }
  return reward;
}

// The game as ba3c_envkernel.h's sim_kernel takes it.
struct BoxingRules {
  using Game = BoxingGame;
  // boxing.py: render_numpy, for the pixels of one frame row.  A boxer's body and arm are
  // adjacent and share a shade, and both of the agent's come before both of the opponent's, so
  // each boxer is ONE span [lo, lo + w) per row (w = 0: not in this row).  The score bars, the
  // clock and the ring's horizontal edges lie in rows no boxer reaches and fold into a third
  // span; `side` marks the rows that carry the ring's two vertical edges.
  struct Row {
    int32_t a_lo, o_lo, b_lo;
    uint32_t a_w, o_w, b_w, b_shade;
    bool side;
  };
  static __device__ __forceinline__ void load(Game& g, int4 r0, int4 r1, int4 r2, int4) {
    g.ax = r0.x; g.ay = r0.y; g.ox = r0.z; g.oy = r0.w;
    g.a_cd = r1.x; g.o_cd = r1.y; g.a_score = r1.z; g.o_score = r1.w;
    g.t = r2.x; g.rng = (uint32_t)r2.y;
  }
  static __device__ __forceinline__ void store(const Game& g, int4* out) {
    out[0] = make_int4(g.ax, g.ay, g.ox, g.oy);
    out[1] = make_int4(g.a_cd, g.o_cd, g.a_score, g.o_score);
    out[2] = make_int4(g.t, (int32_t)g.rng, 0, 0);
    out[3] = make_int4(0, 0, 0, 0);
  }
  static __device__ __forceinline__ int32_t step(Game& g, int64_t a, int32_t limit, bool* over_out,
                                                 int32_t* ep_out) {
    return bx_step(g, a, limit, over_out, ep_out);
  }
  // the span of the boxer at (x, y) in frame row `fy`; its arm (cd >= 6) leaves its left side
  // when arm_left
  static __device__ __forceinline__ void span(int fy, int32_t x, int32_t y, int32_t cd, bool arm_left,
                                              int32_t* lo, uint32_t* w) {
    const bool body = (unsigned)(fy - y) < (unsigned)BX_BODY_H;
    const bool arm = cd >= BX_ARM_CD && (unsigned)(fy - y - BX_ARM_ROW) < (unsigned)BX_ARM_H;
    *lo = x - ((arm && arm_left) ? BX_ARM_W : 0);
    *w = body ? (uint32_t)(BX_BODY_W + (arm ? BX_ARM_W : 0)) : 0u;
  }
  static __device__ __forceinline__ Row row(const Game& g, int y) {
    Row rw;
    span(y, g.ax, g.ay, g.a_cd, !(g.ax <= g.ox), &rw.a_lo, &rw.a_w);   // the agent faces right
    span(y, g.ox, g.oy, g.o_cd, g.ox >= g.ax, &rw.o_lo, &rw.o_w);      // the opponent faces left
    rw.b_lo = 0;
    rw.b_w = 0u;
    rw.b_shade = 60u;
    if ((unsigned)(y - 2) < 2u) {                       // agent score bar
      rw.b_w = (uint32_t)(g.a_score / 2);
      rw.b_shade = 255u;
    } else if ((unsigned)(y - 5) < 2u) {                // opponent score bar, from the right
      rw.b_w = (uint32_t)(g.o_score / 2);
      rw.b_lo = ENV_W - (int32_t)rw.b_w;
      rw.b_shade = 130u;
    } else if (y == 8) {                                // clock
      rw.b_w = (uint32_t)max(ENV_W - g.t / 20, 0);
    } else if (y == 12 || y == 79) {                    // ring, top and bottom
      rw.b_lo = 2;
      rw.b_w = 80u;
    }
    rw.side = (unsigned)(y - 12) < 68u;                 // ring, left and right: y in [12, 79]
    return rw;
  }
  static __device__ __forceinline__ uint32_t pixel(const Game&, int, int x, const Row& rw) {
    if ((unsigned)(x - rw.a_lo) < rw.a_w) return 255u;
    if ((unsigned)(x - rw.o_lo) < rw.o_w) return 130u;
    if ((unsigned)(x - rw.b_lo) < rw.b_w) return rw.b_shade;
    if (rw.side && (x == 2 || x == 81)) return 60u;
    return 0u;
  }
};

}  // namespace ba3c
