// ba3c_duel.h — two-player GridBoxing: both boxers of a game row are driven by actions and each
// side receives its own observation.  The rules are stated once in ba3c_amd/duel.py (step_numpy,
// render_numpy, mirror_rows: the oracle of this kernel); this file restates them over
// ba3c_boxing.h's row, masks, bx_clamp / bx_pts and BoxingRules' pixels.
//
// game[e] = [ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t, rng, 0, ...]: GridBoxing's row,
// side B in the o* fields; rng is carried unchanged (the duel draws nothing).
// G games have 2G players: player e is side A of game e, player G + e is side B.  Side B acts
// and sees in the mirror x -> 78 - x, in which it is the white boxer that starts on the left.
//
// One 256-thread workgroup per GAME (not per player): both sides replace the same row, so one
// workgroup steps it once and then renders twice, side A from g and side B from mirror(g).
#pragma once
#include "ba3c_boxing.h"

namespace ba3c {

struct DuelArgs {
  int32_t* game;            // [G][16]
  const int64_t* action;    // [2G] (null: render only)
  int32_t n_games;
  int32_t limit;
  double* reward;           // [2G]
  uint8_t* over;            // [2G]
  int32_t* ep_score;        // [2G], written where over
  uint8_t* frame;           // [2G][84*84] or null
  uint8_t* state;           // [2G][84*84][4] or null
};

// (dx, dy, fire) of an action in its side's own frame; out of range: NOOP.
__device__ __forceinline__ void duel_decode(int64_t a, int32_t* dx, int32_t* dy, bool* fire) {
  const uint32_t sh = (uint64_t)a < 18u ? (uint32_t)a : 0u;      // NOOP has no bit in any mask
  *dx = (int32_t)((BX_RIGHT >> sh) & 1u) - (int32_t)((BX_LEFT >> sh) & 1u);
  *dy = (int32_t)((BX_DOWN >> sh) & 1u) - (int32_t)((BX_UP >> sh) & 1u);
  *fire = (BX_FIRE >> sh) & 1u;
}

// duel.py: mirror_rows.  The world as side B sees it: x -> 78 - x and the sides exchanged.
__device__ __forceinline__ BoxingGame duel_mirror(const BoxingGame& g) {
  BoxingGame m;
  m.ax = 78 - g.ox; m.ay = g.oy; m.ox = 78 - g.ax; m.oy = g.ay;
  m.a_cd = g.o_cd; m.o_cd = g.a_cd; m.a_score = g.o_score; m.o_score = g.a_score;
  m.t = g.t; m.rng = g.rng;
  return m;
}

// One step of the rules (duel.py: step_numpy).  Returns side A's reward (side B's is its
// negative); *ep_out is side A's episode score.
__device__ __forceinline__ int32_t duel_step(BoxingGame& g, int64_t a, int64_t b, int32_t limit,
                                             bool* over_out, int32_t* ep_out) {
  int32_t dx_a, dy_a, dx_b, dy_b;
  bool fire_a, fire_b;
  duel_decode(a, &dx_a, &dy_a, &fire_a);
  duel_decode(b, &dx_b, &dy_b, &fire_b);
  g.a_cd = max(g.a_cd - 1, 0);
  g.o_cd = max(g.o_cd - 1, 0);
  g.ax = bx_clamp(g.ax + 2 * dx_a, BX_X_MIN, BX_X_MAX);
  g.ay = bx_clamp(g.ay + 2 * dy_a, BX_Y_MIN, BX_Y_MAX);
  g.ox = bx_clamp(g.ox - 2 * dx_b, BX_X_MIN, BX_X_MAX);           // B's RIGHT is the world's left
  g.oy = bx_clamp(g.oy + 2 * dy_b, BX_Y_MIN, BX_Y_MAX);
  const int32_t p = bx_pts(g);                                    // ONE judgement, after both moves
  const bool b_right = g.ox >= g.ax;
  int32_t pa = 0, pb = 0;
  if (fire_a && g.a_cd == 0) { g.a_cd = BX_COOLDOWN; pa = p; }
  if (fire_b && g.o_cd == 0) { g.o_cd = BX_COOLDOWN; pb = p; }
  g.a_score += pa;
  g.o_score += pb;
  if (pa) g.ox = bx_clamp(g.ox + (b_right ? BX_KNOCK : -BX_KNOCK), BX_X_MIN, BX_X_MAX);
  if (pb) g.ax = bx_clamp(g.ax + (b_right ? -BX_KNOCK : BX_KNOCK), BX_X_MIN, BX_X_MAX);
  g.t += 1;
  const bool over = g.a_score >= BX_KO || g.o_score >= BX_KO || g.t >= BX_CLOCK || g.t >= limit;
  *over_out = over;
  *ep_out = g.a_score - g.o_score;
  if (over) {
    g.ax = BX_AX0; g.ay = BX_AY0; g.ox = BX_OX0; g.oy = BX_OY0;
    g.a_cd = g.o_cd = g.a_score = g.o_score = g.t = 0;
  }
  return pa - pb;
}

__global__ void __launch_bounds__(256) duel_kernel(const DuelArgs a) {
  const int e = blockIdx.x;
  const int tid = threadIdx.x;
  const int4* row = reinterpret_cast<const int4*>(a.game + (size_t)e * 16);
  const int4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
  BoxingGame g;
  BoxingRules::load(g, r0, r1, r2, r3);
  bool over = a.action == nullptr;      // render only: both histories start (zeros + frame)
  if (a.action != nullptr) {
    int32_t ep = 0;
    const int32_t reward = duel_step(g, a.action[e], a.action[a.n_games + e], a.limit, &over, &ep);
    __syncthreads();                    // every thread has read the row before it is replaced
    if (tid == 0) {
      BoxingRules::store(g, reinterpret_cast<int4*>(a.game + (size_t)e * 16));
      a.reward[e] = (double)reward;
      a.reward[a.n_games + e] = (double)-reward;
      a.over[e] = a.over[a.n_games + e] = over ? 1 : 0;
      if (over) {
        a.ep_score[e] = ep;
        a.ep_score[a.n_games + e] = -ep;
      }
    }
  }
  env_render_push<BoxingRules>(g, over, a.frame, a.state, e, tid);
  env_render_push<BoxingRules>(duel_mirror(g), over, a.frame, a.state, a.n_games + e, tid);
}

}  // namespace ba3c
