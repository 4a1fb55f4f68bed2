// ba3c_episodes.h — the episodes the training simulators finish, logged on the GPU:
// MySimulatorMaster's reward sum per simulator (self.stats[ident], OpenAIGym/train.py:394-412),
// fed to self.games at every episode end, for every simulator at once and without a host read.
// ba3c_amd/episodes.py (update_numpy) states the rules and is this kernel's bit-exact oracle.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ba3c {

// One launch, for every simulator e:
//   ret[e] += reward[e] (float64, one rounding; the raw reward);  len[e] += 1
//   over[e]:  ring slot (head + k) % cap, k = the flags set below e in this launch, receives
//             {ret[e], len[e], e};  ret[e] = +0.0, len[e] = 0
//   head += the flags set
// The order of one launch's entries (increasing e) comes from a scan over the flags: a wave
// ballot + popcount, and one LDS pass over the wave totals.  No atomics: two runs log identical
// rings.
//
// One workgroup of 1024 threads walks the simulators in passes of kEpisodeChunk with a carry (the
// ring position), as nstep_returns_kernel does.  A single workgroup, because `head` is read and
// written by the same launch: across workgroups the write of the new head would race the reads of
// the old one.  Each thread takes kEpisodeUnroll simulators per pass (e = first + j * 1024 + tid),
// so their loads are in flight together and a pass costs one barrier: 16 passes at E = 65536.
// The wave totals are double-buffered: a wave two passes ahead cannot exist, as the barrier in
// between needs every wave to have left the pass before.
struct EpisodeArgs {
  const double* reward;     // [E] as the environments return it (unclipped)
  const uint8_t* over;      // [E] the step ended the simulator's episode
  int E;
  double* ret;              // [E] running reward sum of the episode in progress
  int32_t* len;             // [E] its decisions so far
  double* log_score;        // [cap] ring: finished episodes' sums
  int32_t* log_len;         // [cap]       ... lengths
  int32_t* log_env;         // [cap]       ... simulators
  int cap;                  // >= E: one launch never overwrites its own entries
  int64_t* head;            // [1] episodes ever logged
};

constexpr int kEpisodeThreads = 1024;
constexpr int kEpisodeUnroll = 4;
constexpr int kEpisodeChunk = kEpisodeThreads * kEpisodeUnroll;
constexpr int kEpisodeWaves = kEpisodeThreads / 64;

__global__ void __launch_bounds__(kEpisodeThreads) episode_stats_kernel(const EpisodeArgs a) {
  __shared__ int32_t wave_total[2][kEpisodeUnroll][kEpisodeWaves];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int64_t head = *a.head;
  const uint32_t cap = (uint32_t)a.cap;
  uint32_t base = (uint32_t)(head % a.cap);     // ring slot of the next entry
  int64_t logged = 0;
  int buf = 0;
  for (int64_t first = 0; first < a.E; first += kEpisodeChunk, buf ^= 1) {
    double r[kEpisodeUnroll];
    int32_t l[kEpisodeUnroll];
    bool o[kEpisodeUnroll];
    int below[kEpisodeUnroll];                  // flags set in lower lanes of the same wave
#pragma unroll
    for (int j = 0; j < kEpisodeUnroll; ++j) {
      const int64_t e = first + j * kEpisodeThreads + tid;
      o[j] = false;
      r[j] = 0.0;
      l[j] = 0;
      if (e < a.E) {
        r[j] = a.ret[e] + a.reward[e];
        l[j] = a.len[e] + 1;
        o[j] = a.over[e] != 0;
      }
      const unsigned long long m = __ballot(o[j]);
      below[j] = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wave_total[buf][j][wave] = __popcll(m);
    }
    __syncthreads();
    uint32_t run = 0;                           // flags set in the pass so far
#pragma unroll
    for (int j = 0; j < kEpisodeUnroll; ++j) {
      uint32_t k = run;
#pragma unroll
      for (int w = 0; w < kEpisodeWaves; ++w) {
        const uint32_t t = (uint32_t)wave_total[buf][j][w];
        if (w < wave) k += t;
        run += t;
      }
      const int64_t e = first + j * kEpisodeThreads + tid;
      if (e < a.E) {
        if (o[j]) {
          uint32_t slot = base + k + (uint32_t)below[j];     // < 2 * cap <= 2^32 - 2
          if (slot >= cap) slot -= cap;
          a.log_score[slot] = r[j];
          a.log_len[slot] = l[j];
          a.log_env[slot] = (int32_t)e;
          r[j] = 0.0;
          l[j] = 0;
        }
        a.ret[e] = r[j];
        a.len[e] = l[j];
      }
    }
    base += run;                                // run <= E <= cap
    if (base >= cap) base -= cap;
    logged += run;
  }
  if (tid == 0) *a.head = head + logged;
}

}  // namespace ba3c
