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
// workgroup steps it once and then renders twice, side A from g and side B from mirror(g):
// sim_kernel<DuelSim, .> (ba3c_envkernel.h) with DuelSim below.
#pragma once
#include "ba3c_boxing.h"

namespace ba3c {

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
// start here; DuelSim::decide passes false and starts the episode itself (a drawn start).
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

// What a decision adds to a step (duel.py: decide_numpy): the aux rows, the frame-skip and sticky
// parameters of ba3c_amd/frameskip.py (EnvSkipArgs, the sticky draw per side) and the range of the
// drawn start.  aux is [G][8] = [rng_k, rng_a, rng_b, prev_a, prev_b, 0, 0, 0] here.
struct DuelDecideArgs : EnvSkipArgs {
  int32_t start_lo;        // half-gap h = start_lo + draw % start_span; start_lo == 19: the fixed
  uint32_t start_span;      // start, which draws nothing
};

// Two players per row (ba3c_envkernel.h: Sim): player 0 is side A, player 1 side B, who acts on
// and sees the mirrored row.  The step is made once and both sides are rendered from it.
struct DuelSim {
  using Rules = BoxingRules;
  using DecideArgs = DuelDecideArgs;
  struct Aux { int4 lo, hi; };
  static constexpr int PLAYERS = 2;
  static __device__ __forceinline__ BoxingGame view(const BoxingGame& g, int p) {
    return p ? duel_mirror(g) : g;
  }
  static __device__ __forceinline__ int32_t step(BoxingGame& g, const int64_t* action, int e, int G,
                                                 int32_t limit, bool* over, int32_t* ep) {
    return duel_step(g, action[e], action[G + e], limit, over, ep);
  }
  static __device__ __forceinline__ Aux load_aux(const DecideArgs& k, int e) {
    const int4* aux = reinterpret_cast<const int4*>(k.aux + (size_t)e * 8);
    return Aux{aux[0], aux[1]};
  }
  static __device__ __forceinline__ void store_aux(const DecideArgs& k, int e, const Aux& x) {
    int4* aux = reinterpret_cast<int4*>(k.aux + (size_t)e * 8);
    aux[0] = x.lo;
    aux[1] = x.hi;
  }
  // duel.py: decide_numpy.  k drawn from rng_k, each side's sticky draws from its own generator,
  // k steps of the rules in registers; the sub-steps after an episode's end are dropped and the
  // fresh row is drawn once.
  static __device__ __forceinline__ int32_t decide(BoxingGame& g, Aux& x, const int64_t* action, int e, int G,
                                                   int32_t limit, const DecideArgs& k, bool* over_out,
                                                   int32_t* ep) {
    const int64_t act_a = action[e], act_b = action[G + e];
    const int32_t chosen_a = (uint64_t)act_a < 32u ? (int32_t)act_a : 0;   // out of range: NOOP, before
    const int32_t chosen_b = (uint64_t)act_b < 32u ? (int32_t)act_b : 0;   // it can be remembered
    const uint32_t rng_k = env_lcg((uint32_t)x.lo.x);
    uint32_t rng_a = (uint32_t)x.lo.y, rng_b = (uint32_t)x.lo.z;
    int32_t prev_a = x.lo.w, prev_b = x.hi.x;
    const int32_t n = k.skip_lo + (int32_t)((rng_k >> 16) % k.skip_span);
    int32_t reward = 0;
    bool over = false;
    for (int32_t j = 0; j < n && !over; ++j) {
      rng_a = env_lcg(rng_a);
      prev_a = ((rng_a >> 8) & 0xFFFFu) < k.sticky_q16 ? prev_a : chosen_a;
      rng_b = env_lcg(rng_b);
      prev_b = ((rng_b >> 8) & 0xFFFFu) < k.sticky_q16 ? prev_b : chosen_b;
      reward += duel_step<false>(g, (int64_t)prev_a, (int64_t)prev_b, limit, &over, ep);
    }
    if (over) {
      prev_a = prev_b = 0;
      duel_fresh(g, k.start_lo, k.start_span);
    }
    x.lo = make_int4((int32_t)rng_k, (int32_t)rng_a, (int32_t)rng_b, prev_a);
    x.hi = make_int4(prev_b, 0, 0, 0);
    *over_out = over;
    return reward;
  }
};

}  // namespace ba3c
