// ba3c_envkernel.h — the per-workgroup skeleton the on-device games share (ba3c_breakout.h,
// ba3c_boxing.h, ba3c_duel.h): load the 64-byte game row, step it, store it, render the 84x84
// frame of every player of the row and push it into the H=4, c=1 frame history, all in ONE launch.
//
// One 256-thread workgroup per row.  Every thread loads the row and computes the (wave-uniform)
// step redundantly, a barrier separates those loads from thread 0's store of the new row, then
// the workgroup renders the frames, 4 pixels (one 16-byte group of the history) per thread per
// iteration.  HBM-bound: 2 * 28224 bytes of state per player.
//
// sim_kernel<Sim, true> is the same launch for ONE DECISION (ba3c_amd/frameskip.py, duel.py:
// decide_numpy, its oracles): a frame skip k drawn from [lo, hi] and sticky actions, k game
// steps in registers, then one store, one render and one push per player.  Its draws come from a
// per-row aux row.
//
// A game is a `Rules` type with
//   Game                                   the row as named fields
//   Row                                    what the pixels of one frame row share
//   load(Game&, int4, int4, int4, int4)    the four 16-byte quarters of the row -> fields
//   store(const Game&, int4*)              fields -> the row
//   step(Game&, int64_t a, int32_t limit, bool* over, int32_t* ep_score) -> int32_t reward
//   row(const Game&, int y) -> Row         hoisted by the kernel: a 4-pixel group shares its row
//   pixel(const Game&, int y, int x, const Row&) -> uint32_t shade
// and a `Sim` says how rows map to players (SoloSim<Rules> below, DuelSim in ba3c_duel.h):
//   Rules, PLAYERS                         player p of row e of G is index p * G + e everywhere
//   view(const Game&, int p) -> Game       the row as player p sees it
//   step(Game&, const int64_t* action, int e, int G, int32_t limit, bool* over, int32_t* ep)
//                                          one step; -> player 0's reward (player 1's is its
//                                          negative, as its ep_score; `over` is shared)
//   DecideArgs, Aux, load_aux, store_aux   the aux rows of a decision and its draw parameters
//   decide(Game&, Aux&, action, e, G, limit, const DecideArgs&, over, ep)     one decision
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ba3c {

constexpr int ENV_W = 84, ENV_PIXELS = 84 * 84, ENV_GROUPS = ENV_PIXELS / 4;   // 1764 groups of 4 px

struct EnvArgs {
  int32_t* game;            // [G][16], G rows of PLAYERS players each: E = PLAYERS * G
  const int64_t* action;    // [E] (null: render only)
  int32_t limit;
  int32_t rows;             // G, the grid's size (gridDim.x would cost the launch its hidden arguments)
  double* reward;           // [E]
  uint8_t* over;            // [E]
  int32_t* ep_score;        // [E], written where over
  uint8_t* frame;           // [E][84*84] or null
  uint8_t* state;           // [E][84*84][4] or null
};

// Render the frame of `g` and push it into the frame history: 4 pixels (one 16-byte group of the
// history) per thread per iteration; `over` starts the history (zeros + frame).
template <class Rules>
__device__ __forceinline__ void env_render_push(const typename Rules::Game& g, bool over, uint8_t* frame,
                                                uint8_t* state, int e, int tid) {
  uint4* st = state ? reinterpret_cast<uint4*>(state + (size_t)e * ENV_PIXELS * 4) : nullptr;
  uint32_t* fr = frame ? reinterpret_cast<uint32_t*>(frame + (size_t)e * ENV_PIXELS) : nullptr;
  for (int q = tid; q < ENV_GROUPS; q += 256) {
    const int y = q / (ENV_W / 4), x0 = 4 * (q - y * (ENV_W / 4));
    const typename Rules::Row rw = Rules::row(g, y);
    const uint32_t p0 = Rules::pixel(g, y, x0, rw), p1 = Rules::pixel(g, y, x0 + 1, rw),
                   p2 = Rules::pixel(g, y, x0 + 2, rw), p3 = Rules::pixel(g, y, x0 + 3, rw);
    if (fr) fr[q] = p0 | (p1 << 8) | (p2 << 16) | (p3 << 24);
    if (st) {
      uint4 v = over ? make_uint4(0, 0, 0, 0) : st[q];
      v.x = (v.x >> 8) | (p0 << 24);
      v.y = (v.y >> 8) | (p1 << 24);
      v.z = (v.z >> 8) | (p2 << 24);
      v.w = (v.w >> 8) | (p3 << 24);
      st[q] = v;
    }
  }
}

// `a.action == nullptr` is the render-only launch: no step, no store, and the histories start.
// The step depends on blockIdx.x and the kernel arguments only, never on threadIdx.x, so it (and
// a decision's whole loop) runs on the scalar unit.  A decision's action is never null.
template <class Sim, bool kDecide>
__global__ void __launch_bounds__(256) sim_kernel(const EnvArgs a, const typename Sim::DecideArgs k) {
  using Rules = typename Sim::Rules;
  const int e = blockIdx.x, G = a.rows;
  const int tid = threadIdx.x;
  int4* row = reinterpret_cast<int4*>(a.game + (size_t)e * 16);
  const int4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
  typename Rules::Game g;
  Rules::load(g, r0, r1, r2, r3);
  bool over = true;                     // render only: the histories start (zeros + frame)
  if (kDecide || a.action != nullptr) {
    typename Sim::Aux x;
    int32_t reward, ep = 0;
    if constexpr (kDecide) {
      x = Sim::load_aux(k, e);
      reward = Sim::decide(g, x, a.action, e, G, a.limit, k, &over, &ep);
    } else {
      reward = Sim::step(g, a.action, e, G, a.limit, &over, &ep);
    }
    __syncthreads();                    // every thread has read the rows before they are replaced
    if (tid == 0) {
      Rules::store(g, row);
      if constexpr (kDecide) Sim::store_aux(k, e, x);
#pragma unroll
      for (int p = 0; p < Sim::PLAYERS; ++p) {
        a.reward[p * G + e] = (double)(p ? -reward : reward);
        a.over[p * G + e] = over ? 1 : 0;
        if (over) a.ep_score[p * G + e] = p ? -ep : ep;
      }
    }
  }
  // `over` is wave-uniform, but past thread 0's branch the compiler no longer sees it: said here,
  // the history's restart stays a scalar branch of the render loop, not an exec-masked one
  over = __builtin_amdgcn_readfirstlane(over);
#pragma unroll
  for (int p = 0; p < Sim::PLAYERS; ++p)
    env_render_push<Rules>(Sim::view(g, p), over, a.frame, a.state, p * G + e, tid);
}

// What a decision adds to a step: the aux rows and the draw parameters (frameskip.py).
struct EnvSkipArgs {
  int32_t* aux;             // [E][2] = [rng2, prev]
  int32_t skip_lo;          // k = skip_lo + draw % skip_span, skip_span = hi - lo + 1
  uint32_t skip_span;
  uint32_t sticky_q16;      // a sub-step repeats prev when its 16-bit draw is below this
};

__device__ __forceinline__ uint32_t env_lcg(uint32_t x) { return x * 1664525u + 1013904223u; }

// One player per row: Breakout and Boxing.
template <class R>
struct SoloSim {
  using Rules = R;
  using Game = typename R::Game;
  using DecideArgs = EnvSkipArgs;
  using Aux = int2;
  static constexpr int PLAYERS = 1;
  static __device__ __forceinline__ const Game& view(const Game& g, int) { return g; }
  static __device__ __forceinline__ int32_t step(Game& g, const int64_t* action, int e, int, int32_t limit,
                                                 bool* over, int32_t* ep) {
    return R::step(g, action[e], limit, over, ep);
  }
  static __device__ __forceinline__ Aux load_aux(const DecideArgs& k, int e) {
    return *reinterpret_cast<const int2*>(k.aux + (size_t)e * 2);
  }
  static __device__ __forceinline__ void store_aux(const DecideArgs& k, int e, const Aux& x) {
    *reinterpret_cast<int2*>(k.aux + (size_t)e * 2) = x;
  }
  // frameskip.py: step_numpy.  k and every draw come from the one generator of the aux row; the
  // sub-steps after an episode's end are dropped (the row has auto-reset).
  static __device__ __forceinline__ int32_t decide(Game& g, Aux& x, const int64_t* action, int e, int,
                                                   int32_t limit, const DecideArgs& k, bool* over_out,
                                                   int32_t* ep) {
    const int64_t act = action[e];
    const int32_t chosen = (uint64_t)act < 32u ? (int32_t)act : 0;   // out of range: NOOP, before it
    uint32_t rng2 = env_lcg((uint32_t)x.x);                           // can be remembered
    int32_t prev = x.y;
    const int32_t n = k.skip_lo + (int32_t)((rng2 >> 16) % k.skip_span);
    int32_t reward = 0;
    bool over = false;
    for (int32_t j = 0; j < n && !over; ++j) {
      rng2 = env_lcg(rng2);
      prev = ((rng2 >> 8) & 0xFFFFu) < k.sticky_q16 ? prev : chosen;
      reward += R::step(g, (int64_t)prev, limit, &over, ep);
    }
    if (over) prev = 0;
    x = make_int2((int32_t)rng2, prev);
    *over_out = over;
    return reward;
  }
};

}  // namespace ba3c
