// ba3c_envkernel.h — the per-workgroup skeleton the on-device games share (ba3c_breakout.h,
// ba3c_boxing.h): load the 64-byte game row, step it, store it, render the 84x84 frame and push
// it into the H=4, c=1 frame history, all in ONE launch.
//
// One 256-thread workgroup per simulator.  Every thread loads the game row and computes the
// (wave-uniform) step redundantly, a barrier separates those loads from thread 0's store of
// the new row, then the workgroup renders the frame, 4 pixels (one 16-byte group of the
// history) per thread per iteration.  HBM-bound: 2 * 28224 bytes of state per env.
//
// env_skip_kernel is the same launch for ONE DECISION of ba3c_amd/frameskip.py (its oracle): a
// frame skip k drawn from [lo, hi] and sticky actions, k game steps in registers, then one
// render and one push.  Its draws come from a per-simulator aux row [rng2, prev], 8 bytes.
//
// A game is a `Rules` type with
//   Game                                   the row as named fields
//   Row                                    what the pixels of one frame row share
//   load(Game&, int4, int4, int4, int4)    the four 16-byte quarters of the row -> fields
//   store(const Game&, int4*)              fields -> the row
//   step(Game&, int64_t a, int32_t limit, bool* over, int32_t* ep_score) -> int32_t reward
//   row(const Game&, int y) -> Row         hoisted by the kernel: a 4-pixel group shares its row
//   pixel(const Game&, int y, int x, const Row&) -> uint32_t shade
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ba3c {

constexpr int ENV_W = 84, ENV_PIXELS = 84 * 84, ENV_GROUPS = ENV_PIXELS / 4;   // 1764 groups of 4 px

struct EnvArgs {
  int32_t* game;            // [E][16]
  const int64_t* action;    // [E] (null: render only)
  int32_t limit;
  double* reward;           // [E]
  uint8_t* over;            // [E]
  int32_t* ep_score;        // [E], written where over
  uint8_t* frame;           // [E][84*84] or null
  uint8_t* state;           // [E][84*84][4] or null
};

// Render the frame of `g` and push it into the frame history: 4 pixels (one 16-byte group of the
// history) per thread per iteration; `over` starts the history (zeros + frame).  Shared by both
// kernels below.
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

template <class Rules>
__global__ void __launch_bounds__(256) env_kernel(const EnvArgs a) {
  const int e = blockIdx.x;
  const int tid = threadIdx.x;
  const int4* row = reinterpret_cast<const int4*>(a.game + (size_t)e * 16);
  const int4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
  typename Rules::Game g;
  Rules::load(g, r0, r1, r2, r3);
  bool over = a.action == nullptr;      // render only: the history starts (zeros + frame)
  if (a.action != nullptr) {
    int32_t ep = 0;
    const int32_t reward = Rules::step(g, a.action[e], a.limit, &over, &ep);
    __syncthreads();                    // every thread has read the row before it is replaced
    if (tid == 0) {
      Rules::store(g, reinterpret_cast<int4*>(a.game + (size_t)e * 16));
      a.reward[e] = (double)reward;
      a.over[e] = over ? 1 : 0;
      if (over) a.ep_score[e] = ep;
    }
  }
  env_render_push<Rules>(g, over, a.frame, a.state, e, tid);
}

// What a decision adds to a step: the aux rows and the draw parameters (frameskip.py).
struct EnvSkipArgs {
  int32_t* aux;             // [E][2] = [rng2, prev]
  int32_t skip_lo;          // k = skip_lo + draw % skip_span, skip_span = hi - lo + 1
  uint32_t skip_span;
  uint32_t sticky_q16;      // a sub-step repeats prev when its 16-bit draw is below this
};

__device__ __forceinline__ uint32_t env_lcg(uint32_t x) { return x * 1664525u + 1013904223u; }

// One decision per launch (a.action is never null here).  k, every draw and the game row are
// wave-uniform, so the whole loop runs on the scalar unit; the sub-steps after an episode's end
// are dropped (the row has auto-reset).  One barrier, as in env_kernel.
template <class Rules>
__global__ void __launch_bounds__(256) env_skip_kernel(const EnvArgs a, const EnvSkipArgs k) {
  const int e = blockIdx.x;
  const int tid = threadIdx.x;
  const int4* row = reinterpret_cast<const int4*>(a.game + (size_t)e * 16);
  const int4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
  const int2 aux = *reinterpret_cast<const int2*>(k.aux + (size_t)e * 2);
  typename Rules::Game g;
  Rules::load(g, r0, r1, r2, r3);
  const int64_t act = a.action[e];
  const int32_t chosen = (uint64_t)act < 32u ? (int32_t)act : 0;   // out of range: NOOP, before it
  uint32_t rng2 = env_lcg((uint32_t)aux.x);                         // can be remembered
  int32_t prev = aux.y;
  const int32_t n = k.skip_lo + (int32_t)((rng2 >> 16) % k.skip_span);
  int32_t reward = 0, ep = 0;
  bool over = false;
  for (int32_t j = 0; j < n && !over; ++j) {
    rng2 = env_lcg(rng2);
    prev = ((rng2 >> 8) & 0xFFFFu) < k.sticky_q16 ? prev : chosen;
    reward += Rules::step(g, (int64_t)prev, a.limit, &over, &ep);
  }
  if (over) prev = 0;
  __syncthreads();                      // every thread has read both rows before they are replaced
  if (tid == 0) {
    Rules::store(g, reinterpret_cast<int4*>(a.game + (size_t)e * 16));
    *reinterpret_cast<int2*>(k.aux + (size_t)e * 2) = make_int2((int32_t)rng2, prev);
    a.reward[e] = (double)reward;
    a.over[e] = over ? 1 : 0;
    if (over) a.ep_score[e] = ep;
  }
  env_render_push<Rules>(g, over, a.frame, a.state, e, tid);
}

}  // namespace ba3c
