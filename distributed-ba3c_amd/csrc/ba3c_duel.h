// ba3c_duel.h — two-player GridBoxing: both boxers of a game row are driven by actions and each
// side receives its own observation.  The rules are stated once in ba3c_amd/duel.py (step_numpy,
// render_numpy, mirror_rows: the oracle of this kernel); this file restates them over
// ba3c_boxing.h's row, masks, bx_clamp / bx_pts and BoxingRules' pixels.
//
// game[e] = [ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t, rng, 0, ...]: GridBoxing's row,
// side B in the o* fields; rng is carried unchanged by a step (only a drawn start draws from it).
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
// negative); *ep_out is side A's episode score.  kFresh: on `over` the row restarts from the fixed
// start here; duel_decide_kernel passes false and starts the episode itself (a drawn start).
template <bool kFresh = true>
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
  if (kFresh && over) {
    g.ax = BX_AX0; g.ay = BX_AY0; g.ox = BX_OX0; g.oy = BX_OY0;
    g.a_cd = g.o_cd = g.a_score = g.o_score = g.t = 0;
  }
  return pa - pb;
}

// The fresh episode of a drawn start (duel.py: "Drawn starts"), or of the fixed start when
// h_lo == 19 (no draw: rng is kept).  ONE draw from the row's own rng gives the half-gap h in
// [h_lo, h_lo + h_span) and the shared y; the row (39 - h, y, 39 + h, y) is its own mirror image.
__device__ __forceinline__ void duel_fresh(BoxingGame& g, int32_t h_lo, uint32_t h_span) {
  int32_t h = 19, y = BX_AY0;
  if (h_lo != 19) {
    g.rng = env_lcg(g.rng);
    const uint32_t r = g.rng >> 16;
    h = h_lo + (int32_t)(r % h_span);
    y = BX_Y_MIN + 2 * (int32_t)((r >> 8) % 29u);
  }
  g.ax = 39 - h; g.ay = y; g.ox = 39 + h; g.oy = y;
  g.a_cd = g.o_cd = g.a_score = g.o_score = g.t = 0;
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

// What a decision adds to a step (duel.py: decide_numpy): the aux rows, the frame-skip and sticky
// parameters of ba3c_amd/frameskip.py and the range of the drawn start.
struct DuelDecideArgs {
  int32_t* aux;             // [G][8] = [rng_k, rng_a, rng_b, prev_a, prev_b, 0, 0, 0]
  int32_t skip_lo;          // k = skip_lo + draw % skip_span, skip_span = hi - lo + 1
  uint32_t skip_span;
  uint32_t sticky_q16;      // a side's sub-step repeats its prev when its 16-bit draw is below this
  int32_t start_lo;         // half-gap h = start_lo + draw % start_span; start_lo == 19: the fixed
  uint32_t start_span;      // start, which draws nothing
};

// One DECISION of every game per launch (a.action is never null here): k drawn from rng_k, each
// side's sticky draws from its own generator, k steps of the rules in registers, then one store
// and two renders, as duel_kernel.  k, every draw and both rows are wave-uniform, so the whole
// loop runs on the scalar unit; the sub-steps after an episode's end are dropped and the fresh
// row is drawn once.  One barrier.
__global__ void __launch_bounds__(256) duel_decide_kernel(const DuelArgs a, const DuelDecideArgs k) {
  const int e = blockIdx.x;
  const int tid = threadIdx.x;
  const int4* row = reinterpret_cast<const int4*>(a.game + (size_t)e * 16);
  const int4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
  const int4* aux = reinterpret_cast<const int4*>(k.aux + (size_t)e * 8);
  const int4 x0 = aux[0], x1 = aux[1];
  BoxingGame g;
  BoxingRules::load(g, r0, r1, r2, r3);
  const int64_t act_a = a.action[e], act_b = a.action[a.n_games + e];
  const int32_t chosen_a = (uint64_t)act_a < 32u ? (int32_t)act_a : 0;   // out of range: NOOP, before
  const int32_t chosen_b = (uint64_t)act_b < 32u ? (int32_t)act_b : 0;   // it can be remembered
  const uint32_t rng_k = env_lcg((uint32_t)x0.x);
  uint32_t rng_a = (uint32_t)x0.y, rng_b = (uint32_t)x0.z;
  int32_t prev_a = x0.w, prev_b = x1.x;
  const int32_t n = k.skip_lo + (int32_t)((rng_k >> 16) % k.skip_span);
  int32_t reward = 0, ep = 0;
  bool over = false;
  for (int32_t j = 0; j < n && !over; ++j) {
    rng_a = env_lcg(rng_a);
    prev_a = ((rng_a >> 8) & 0xFFFFu) < k.sticky_q16 ? prev_a : chosen_a;
    rng_b = env_lcg(rng_b);
    prev_b = ((rng_b >> 8) & 0xFFFFu) < k.sticky_q16 ? prev_b : chosen_b;
    reward += duel_step<false>(g, (int64_t)prev_a, (int64_t)prev_b, a.limit, &over, &ep);
  }
  if (over) {
    prev_a = prev_b = 0;
    duel_fresh(g, k.start_lo, k.start_span);
  }
  __syncthreads();                      // every thread has read both rows before they are replaced
  if (tid == 0) {
    BoxingRules::store(g, reinterpret_cast<int4*>(a.game + (size_t)e * 16));
    int4* aux_out = reinterpret_cast<int4*>(k.aux + (size_t)e * 8);
    aux_out[0] = make_int4((int32_t)rng_k, (int32_t)rng_a, (int32_t)rng_b, prev_a);
    aux_out[1] = make_int4(prev_b, 0, 0, 0);
    a.reward[e] = (double)reward;
    a.reward[a.n_games + e] = (double)-reward;
    a.over[e] = a.over[a.n_games + e] = over ? 1 : 0;
    if (over) {
      a.ep_score[e] = ep;
      a.ep_score[a.n_games + e] = -ep;
    }
  }
  env_render_push<BoxingRules>(g, over, a.frame, a.state, e, tid);
  env_render_push<BoxingRules>(duel_mirror(g), over, a.frame, a.state, a.n_games + e, tid);
}

}  // namespace ba3c
