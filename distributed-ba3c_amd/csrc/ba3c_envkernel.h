// ba3c_envkernel.h — the per-workgroup skeleton the on-device games share (ba3c_breakout.h,
// ba3c_boxing.h): load the 64-byte game row, step it, store it, render the 84x84 frame and push
// it into the H=4, c=1 frame history, all in ONE launch.
//
// One 256-thread workgroup per simulator.  Every thread loads the game row and computes the
// (wave-uniform) step redundantly, a barrier separates those loads from thread 0's store of
// the new row, then the workgroup renders the frame, 4 pixels (one 16-byte group of the
// history) per thread per iteration.  HBM-bound: 2 * 28224 bytes of state per env.
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
  uint4* st = a.state ? reinterpret_cast<uint4*>(a.state + (size_t)e * ENV_PIXELS * 4) : nullptr;
  uint32_t* fr = a.frame ? reinterpret_cast<uint32_t*>(a.frame + (size_t)e * ENV_PIXELS) : nullptr;
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

}  // namespace ba3c
