// ba3c_perturb.h — perturbation saliency on the device: the kernel that
// makes the 289 blurred-patch copies of a state and the kernel that turns the network's outputs on
// them into an 84 x 84 score map.  ba3c_amd/perturb.py states the rule and is the oracle of both;
// the first kernel is held to it bit for bit.
//
// perturb_states_kernel: one workgroup per (state, centre row i).  It stages the state's four
// planes in LDS once (a pixel is a dword of four history bytes, four pixels a 16-byte group),
// blurs only what its 17 centres (5i, 5j) can touch — the horizontal pass over source rows
// 5i-24 .. 5i+24, the vertical pass over the 31 rows 5i-15 .. 5i+15, both exact, reflected at
// the edges — keeps that Q24 band in LDS, and writes its 17 perturbed states with 16-byte stores:
// copies of the LDS image outside the centre's 31 x 31 window, the fixed-point blend inside.
// The launch is store-bound by construction (289 x 28 224 bytes out for 28 224 in).  WEIGHTS and
// MASK_Q are compile-time tables: the blur's taps are unrolled immediates, the mask's 16 entries
// are packed into two 64-bit immediates and selected by a shift, so no runtime value indexes
// memory other than pixel addresses.  No atomics; plain vector C++.
//
// perturb_scores_kernel: one workgroup per source state forms the 17 x 17 grid of the requested
// score in float64 in LDS (lane k, then k + 256, owns centre k; actions are summed in order) and
// writes the bilinear 84 x 84 float32 map, and the raw grid where asked.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ba3c {

struct Perturb {
  static constexpr int H = 84, W = 84;
  static constexpr int GROUPS = 21;             // 16-byte groups of four pixels per row
  static constexpr int VEC = H * GROUPS;        // 1764 groups = 28 224 bytes per state
  static constexpr int GRID = 17, NC = GRID * GRID, STRIDE = 5;
  static constexpr int R = 9;                   // blur radius: 19 taps
  static constexpr int MR = 15;                 // the mask is zero beyond
  static constexpr int HROWS = 2 * (MR + R) + 1;   // 49 rows of the horizontal pass
  static constexpr int BROWS = 2 * MR + 1;         // 31 rows of the blurred band
  static constexpr int THREADS = 256;
  // perturb.WEIGHTS (Q12, sum 4096) and perturb.MASK_Q (peak 256)
  static constexpr unsigned WEIGHTS[2 * R + 1] = {6,   16,  36,  74,  136, 224, 331, 437, 516, 544,
                                                  516, 437, 331, 224, 136, 74,  36,  16,  6};
  static constexpr unsigned MASK_Q[MR + 1] = {256, 251, 236, 214, 186, 155, 125, 96, 71, 51, 35, 23, 14, 9, 5, 3};
};

struct PerturbStatesArgs {
  const uint4* state;      // [n][84][21] groups
  uint4* out;              // [count][84][21]
  long long first, count;  // the perturbed states first .. first + count of the n * 289
  int wg0;                 // (state, centre row) of workgroup 0: first / 17
};

struct PerturbScoresArgs {
  const float *probs0, *value0;   // the source states' outputs [n][A], [n]
  const float *probs, *value;     // the perturbed states' [n * 289][A], [n * 289]
  float* map;                     // [n][84][84]
  double* grid;                   // [n][17][17], or null
  int num_actions, which;         // which: 0 S_v, 1 S_pi
};

hipError_t launch_perturb_states(hipStream_t s, const PerturbStatesArgs& a, bool newest);
hipError_t launch_perturb_scores(hipStream_t s, const PerturbScoresArgs& a, int n);

#ifdef BA3C_PERTURB_KERNELS   // the device code: ba3c_perturb.hip only

constexpr unsigned long long perturb_mask_word(int k0) {
  unsigned long long v = 0;
  for (int k = 0; k < 8; ++k) v |= (unsigned long long)(Perturb::MASK_Q[k0 + k] & 255u) << (8 * k);
  return v;
}
constexpr bool perturb_tables_ok() {
  unsigned sum = 0;
  for (unsigned w : Perturb::WEIGHTS) sum += w;
  bool ok = sum == 4096 && Perturb::MASK_Q[0] == 256;
  for (int k = 1; k <= Perturb::MR; ++k) ok = ok && Perturb::MASK_Q[k] < 256;
  return ok;
}
static_assert(perturb_tables_ok(), "WEIGHTS sum to 4096; MASK_Q[1..15] fit a byte under a peak of 256");

// MASK_Q[t] for t = |d| >= 0 (0 beyond 15): a shift of one of two immediates
__device__ __forceinline__ unsigned perturb_mask_q(int t) {
  constexpr unsigned long long LO = perturb_mask_word(0), HI = perturb_mask_word(8);
  const unsigned v = (unsigned)((t < 8 ? LO : HI) >> (8 * (t & 7))) & 255u;
  return t == 0 ? 256u : (t > Perturb::MR ? 0u : v);
}

__device__ __forceinline__ int perturb_reflect(int i) {   // d c b a | a b c d, |overhang| <= 84
  return i < 0 ? -1 - i : (i >= Perturb::H ? 2 * Perturb::H - 1 - i : i);
}

// One pixel: (p 2^24 (2^16 - m) + blur m + 2^39) >> 40 per plane, planes P0..3 (the others copied)
template <int P0>
__device__ __forceinline__ unsigned perturb_blend(unsigned p, const uint4& b, unsigned m) {
  const unsigned blur[4] = {b.x, b.y, b.z, b.w};
  unsigned out = P0 ? p & 0x00FFFFFFu : 0u;
#pragma unroll
  for (int c = P0; c < 4; ++c) {
    const unsigned pc = (p >> (8 * c)) & 255u;
    const unsigned long long v = (unsigned long long)(pc << 24) * (65536u - m) +
                                 (unsigned long long)blur[c] * m + (1ull << 39);
    out |= (unsigned)(v >> 40) << (8 * c);
  }
  return out;
}

template <bool NEWEST>
__global__ __launch_bounds__(Perturb::THREADS) void perturb_states_kernel(PerturbStatesArgs a) {
  using P = Perturb;
  constexpr int P0 = NEWEST ? 3 : 0;                 // first plane that is blurred
  __shared__ uint4 s_state[P::VEC];                  // 28 224 bytes: the state
  __shared__ uint4 s_h[P::HROWS * P::W];             // 65 856: the horizontal pass, Q12 per plane
  __shared__ uint4 s_b[P::BROWS * P::W];             // 41 664: the blurred band, Q24 per plane
  const int tid = threadIdx.x;
  const int bs = a.wg0 + (int)blockIdx.x;
  const int n = bs / P::GRID, i = bs - P::GRID * n;
  const int cy = P::STRIDE * i;
  const int h0 = max(0, cy - (P::MR + P::R)), h1 = min(P::H - 1, cy + P::MR + P::R);
  const int b0 = max(0, cy - P::MR), b1 = min(P::H - 1, cy + P::MR);

  const uint4* src = a.state + (size_t)n * P::VEC;
  for (int v = tid; v < P::VEC; v += P::THREADS) s_state[v] = src[v];
  __syncthreads();

  // horizontal pass: an item is a group of four pixels of one row; it reads the 7 groups
  // g-3 .. g+3 (a group past an edge is the mirrored group, its pixels reversed)
  for (int it = tid; it < (h1 - h0 + 1) * P::GROUPS; it += P::THREADS) {
    const int r = it / P::GROUPS, g = it - P::GROUPS * r;
    const uint4* row = s_state + (h0 + r) * P::GROUPS;
    unsigned px[28];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const int gg = g - 3 + k;
      const bool mirrored = gg < 0 || gg >= P::GROUPS;
      const uint4 q = row[gg < 0 ? -1 - gg : (gg >= P::GROUPS ? 2 * P::GROUPS - 1 - gg : gg)];
      px[4 * k + 0] = mirrored ? q.w : q.x;
      px[4 * k + 1] = mirrored ? q.z : q.y;
      px[4 * k + 2] = mirrored ? q.y : q.z;
      px[4 * k + 3] = mirrored ? q.x : q.w;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      unsigned acc[4] = {0, 0, 0, 0};
#pragma unroll
      for (int t = -P::R; t <= P::R; ++t)
#pragma unroll
        for (int c = P0; c < 4; ++c) acc[c] += P::WEIGHTS[t + P::R] * ((px[12 + d + t] >> (8 * c)) & 255u);
      s_h[r * P::W + 4 * g + d] = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    }
  }
  __syncthreads();

  // vertical pass: an item is one pixel of the band; its 19 rows lie in h0 .. h1 after reflection
  for (int it = tid; it < (b1 - b0 + 1) * P::W; it += P::THREADS) {
    const int r = it / P::W, x = it - P::W * r;
    unsigned acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int t = -P::R; t <= P::R; ++t) {
      const uint4 q = s_h[(perturb_reflect(b0 + r + t) - h0) * P::W + x];
      const unsigned hq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int c = P0; c < 4; ++c) acc[c] += P::WEIGHTS[t + P::R] * hq[c];
    }
    s_b[it] = make_uint4(acc[0], acc[1], acc[2], acc[3]);
  }
  __syncthreads();

  // the 17 perturbed states of this centre row, those inside the chunk
  for (int j = 0; j < P::GRID; ++j) {
    const long long idx = (long long)bs * P::GRID + j;
    if (idx < a.first || idx >= a.first + a.count) continue;
    uint4* dst = a.out + (size_t)(idx - a.first) * P::VEC;
    const int cx = P::STRIDE * j;
    for (int v = tid; v < P::VEC; v += P::THREADS) {
      const int y = v / P::GROUPS, x0 = 4 * (v - P::GROUPS * y);
      uint4 q = s_state[v];
      if (abs(y - cy) <= P::MR && x0 + 3 >= cx - P::MR && x0 <= cx + P::MR) {
        const unsigned my = perturb_mask_q(abs(y - cy));
        const uint4* band = s_b + (y - b0) * P::W + x0;
        q.x = perturb_blend<P0>(q.x, band[0], my * perturb_mask_q(abs(x0 - cx)));
        q.y = perturb_blend<P0>(q.y, band[1], my * perturb_mask_q(abs(x0 + 1 - cx)));
        q.z = perturb_blend<P0>(q.z, band[2], my * perturb_mask_q(abs(x0 + 2 - cx)));
        q.w = perturb_blend<P0>(q.w, band[3], my * perturb_mask_q(abs(x0 + 3 - cx)));
      }
      dst[v] = q;
    }
  }
}

__global__ __launch_bounds__(Perturb::THREADS) void perturb_scores_kernel(PerturbScoresArgs a) {
  using P = Perturb;
  __shared__ double s_g[P::NC];
  const int n = blockIdx.x, tid = threadIdx.x, A = a.num_actions;
  for (int k = tid; k < P::NC; k += P::THREADS) {
    const size_t row = (size_t)n * P::NC + k;
    double s = 0.0;
    if (a.which == 0) {
      const double d = (double)a.value0[n] - (double)a.value[row];
      s = d * d;
    } else {
      for (int c = 0; c < A; ++c) {
        const double d = (double)a.probs0[(size_t)n * A + c] - (double)a.probs[row * A + c];
        s += d * d;
      }
    }
    s *= 0.5;
    s_g[k] = s;
    if (a.grid) a.grid[row] = s;
  }
  __syncthreads();
  float* map = a.map + (size_t)n * P::H * P::W;
  for (int v = tid; v < P::H * P::W; v += P::THREADS) {
    const int y = v / P::W, x = v - P::W * y;
    const int y0 = min(y / P::STRIDE, P::GRID - 1), y1 = min(y0 + 1, P::GRID - 1);
    const int x0 = min(x / P::STRIDE, P::GRID - 1), x1 = min(x0 + 1, P::GRID - 1);
    const double ty = y < P::STRIDE * (P::GRID - 1) ? (y % P::STRIDE) / (double)P::STRIDE : 0.0;
    const double tx = x < P::STRIDE * (P::GRID - 1) ? (x % P::STRIDE) / (double)P::STRIDE : 0.0;
    const double top = (1.0 - tx) * s_g[y0 * P::GRID + x0] + tx * s_g[y0 * P::GRID + x1];
    const double bot = (1.0 - tx) * s_g[y1 * P::GRID + x0] + tx * s_g[y1 * P::GRID + x1];
    map[v] = (float)((1.0 - ty) * top + ty * bot);
  }
}

#endif  // BA3C_PERTURB_KERNELS

}  // namespace ba3c
