// ba3c_intgrad.h — integrated-gradients saliency on the device: the kernel
// that makes the K uint8 path states between a baseline and a state, and the kernel that sums the
// K input-gradient images of a state in float64 and scales them by x - x0.  ba3c_amd/intgrad.py
// states the rule and is the oracle of both; the first kernel is held to it bit for bit.
//
// Both kernels split the work the same way: a workgroup owns one (state, band of 12 rows) pair,
// and thread t < 252 owns one 16-byte group of the band (four pixels of four history bytes), so
// x and x0 of the group live in registers for the whole launch.  A chunk [first, first + count)
// of the n * K path states touches the states first / K .. (first + count - 1) / K; a workgroup
// walks the j of its state that fall inside the chunk, [j0, j1), which is where a seam in the
// middle of a state's K points is handled.
//
// The "blur" baseline is perturb.py's blur A of the whole frame, rounded half up to a byte.  A
// workgroup stages its band plus the 9-row halo (30 rows, reflected at the edges) in LDS, runs the
// horizontal pass over those rows into LDS (Q12 per plane, a uint4 per pixel) and the vertical pass
// straight into the owning thread's registers: 50 400 bytes of LDS, no third buffer, and no
// baseline image in HBM.  The "zero" baseline uses no LDS at all.
//
// ig_states_kernel: per j one uint4 store per thread.  Per byte, with d = x - x0 and D = 2K,
//   p = x0 + floor(((2j+1) d + K) / D) = x0 - 256 + floor(((2j+1) d + K + 256 D) / D):
// the shifted numerator is in [0, 2^18), and a division of such a value by D <= 512 is exact as
// the high word of a product with M = floor(2^32 / D) + 1 (M D - 2^32 <= D, and 2^18 D < 2^32).
// The launch is store-bound: count * 28 224 bytes out for at most n * 28 224 in.
//
// ig_accumulate_kernel: the thread's 16 float64 sums come from acc (two double2 per pixel), the
// chunk's gradients of its state are added in ascending j (a float4 per pixel and j), and go back
// to acc; no atomics, so the sums do not depend on where the seams fall.  Where the state's last
// point is in the chunk, attr = (float)((d / 255) (sum / K)) with d recomputed from the state.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba3c_perturb.h"   // Perturb: the frame's geometry and the blur's WEIGHTS

namespace ba3c {

struct IntGrad {
  static constexpr int BAND = 12;                            // rows of a workgroup
  static constexpr int BANDS = Perturb::H / BAND;            // 7 per state
  static constexpr int ITEMS = BAND * Perturb::GROUPS;       // 252 groups: one per thread
  static constexpr int HROWS = BAND + 2 * Perturb::R;        // 30 rows of the horizontal pass
  static constexpr int THREADS = 256;
  static constexpr int MAX_STEPS = 256;
};
static_assert(IntGrad::BANDS * IntGrad::BAND == Perturb::H && IntGrad::ITEMS <= IntGrad::THREADS,
              "the bands tile the frame, and a thread owns at most one group");

struct IgChunk {
  const uint4* state;      // [n][84][21] groups
  long long first, count;  // the path states first .. first + count of the n * steps
  int steps;               // K
  int s0;                  // the state of workgroups 0 .. 6: first / K
};

struct IgStatesArgs {
  IgChunk c;
  uint4* out;              // [count][84][21]
  unsigned magic;          // floor(2^32 / 2K) + 1
};

struct IgAccumulateArgs {
  IgChunk c;
  const float4* grads;     // [count][84][84] pixels of four channels
  double2* acc;            // [n][84][84][2]
  float4* attr;            // [n][84][84], or null
};

hipError_t launch_ig_states(hipStream_t s, const IgStatesArgs& a, bool blur);
hipError_t launch_ig_accumulate(hipStream_t s, const IgAccumulateArgs& a, bool blur);

// the workgroups of a chunk: seven per state it touches
inline int ig_grid(const IgChunk& c) {
  return (int)((c.first + c.count - 1) / c.steps - c.s0 + 1) * IntGrad::BANDS;
}

#ifdef BA3C_INTGRAD_KERNELS   // the device code: ba3c_intgrad.hip only

__device__ __forceinline__ int ig_reflect(int i) {   // d c b a | a b c d, |overhang| <= 9
  return i < 0 ? -1 - i : (i >= Perturb::H ? 2 * Perturb::H - 1 - i : i);
}

// The blurred baseline of the group that thread `tid` owns in `band` of the state at `src`: every
// thread of the workgroup calls it (two barriers); threads past ITEMS get zeros.
__device__ __forceinline__ uint4 ig_blur_group(const uint4* src, int band, int tid) {
  using P = Perturb;
  using I = IntGrad;
  __shared__ uint4 s_rows[I::HROWS * P::GROUPS];     // 10 080 bytes: the band and its halo
  __shared__ uint4 s_h[I::HROWS * P::W];             // 40 320: the horizontal pass, Q12 per plane
  const int top = band * I::BAND - P::R;             // the frame row of LDS row 0, before reflection
  for (int v = tid; v < I::HROWS * P::GROUPS; v += I::THREADS) {
    const int r = v / P::GROUPS, g = v - P::GROUPS * r;
    s_rows[v] = src[ig_reflect(top + r) * P::GROUPS + g];
  }
  __syncthreads();

  // horizontal pass: an item is a group of four pixels of one row; it reads the 7 groups
  // g-3 .. g+3 (a group past an edge is the mirrored group, its pixels reversed)
  for (int it = tid; it < I::HROWS * P::GROUPS; it += I::THREADS) {
    const int r = it / P::GROUPS, g = it - P::GROUPS * r;
    const uint4* row = s_rows + r * P::GROUPS;
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
        for (int c = 0; c < 4; ++c) acc[c] += P::WEIGHTS[t + P::R] * ((px[12 + d + t] >> (8 * c)) & 255u);
      s_h[r * P::W + 4 * g + d] = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    }
  }
  __syncthreads();

  // vertical pass: the thread's own four pixels; band row r is LDS row r + R, so its 19 taps are
  // LDS rows r .. r + 18.  Q24 <= 255 * 2^24, and + 2^23 still fits 32 bits.
  unsigned out[4] = {0, 0, 0, 0};
  if (tid < I::ITEMS) {
    const int r = tid / P::GROUPS, g = tid - P::GROUPS * r;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      unsigned acc[4] = {0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t <= 2 * P::R; ++t) {
        const uint4 q = s_h[(r + t) * P::W + 4 * g + d];
        acc[0] += P::WEIGHTS[t] * q.x;
        acc[1] += P::WEIGHTS[t] * q.y;
        acc[2] += P::WEIGHTS[t] * q.z;
        acc[3] += P::WEIGHTS[t] * q.w;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) out[d] |= ((acc[c] + (1u << 23)) >> 24) << (8 * c);
    }
  }
  return make_uint4(out[0], out[1], out[2], out[3]);
}

// What a workgroup owns: its state, its band, and the j of that state inside the chunk
struct IgOwn {
  int s, band, j0, j1;
  long long row0;          // the chunk row of path state j0
};
__device__ __forceinline__ IgOwn ig_own(const IgChunk& c) {
  IgOwn o;
  o.s = c.s0 + (int)blockIdx.x / IntGrad::BANDS;
  o.band = (int)blockIdx.x % IntGrad::BANDS;
  const long long base = (long long)o.s * c.steps;
  o.j0 = (int)max(0ll, c.first - base);
  o.j1 = (int)min((long long)c.steps, c.first + c.count - base);
  o.row0 = base + o.j0 - c.first;
  return o;
}

template <bool BLUR>
__global__ __launch_bounds__(IntGrad::THREADS) void ig_states_kernel(IgStatesArgs a) {
  using P = Perturb;
  using I = IntGrad;
  const int tid = threadIdx.x;
  const IgOwn o = ig_own(a.c);
  const uint4* src = a.c.state + (size_t)o.s * P::VEC;
  uint4 x0 = make_uint4(0, 0, 0, 0);
  if (BLUR) x0 = ig_blur_group(src, o.band, tid);
  if (tid >= I::ITEMS) return;
  const size_t e = (size_t)o.band * I::ITEMS + tid;           // the group within a state
  const uint4 x = src[e];
  const unsigned xw[4] = {x.x, x.y, x.z, x.w}, bw[4] = {x0.x, x0.y, x0.z, x0.w};
  int d[16], lo[16];                                          // x - x0 and x0 - 256, per byte
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int xb = (int)((xw[k >> 2] >> (8 * (k & 3))) & 255u), bb = (int)((bw[k >> 2] >> (8 * (k & 3))) & 255u);
    d[k] = xb - bb;
    lo[k] = bb - 256;
  }
  const int K = a.c.steps, shift = K + 512 * K;               // K + 256 D
  uint4* dst = a.out + (size_t)o.row0 * P::VEC + e;
  for (int j = o.j0; j < o.j1; ++j, dst += P::VEC) {
    const int t = 2 * j + 1;
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const unsigned q = __umulhi((unsigned)(t * d[k] + shift), a.magic);
      w[k >> 2] |= (unsigned)((int)q + lo[k]) << (8 * (k & 3));     // a byte: the rule never overshoots
    }
    *dst = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

template <bool BLUR>
__global__ __launch_bounds__(IntGrad::THREADS) void ig_accumulate_kernel(IgAccumulateArgs a) {
  using P = Perturb;
  using I = IntGrad;
  const int tid = threadIdx.x;
  const IgOwn o = ig_own(a.c);
  const uint4* src = a.c.state + (size_t)o.s * P::VEC;
  const bool last = a.attr && o.j1 == a.c.steps;              // the same for the whole workgroup
  uint4 x0 = make_uint4(0, 0, 0, 0);
  if (BLUR && last) x0 = ig_blur_group(src, o.band, tid);
  if (tid >= I::ITEMS) return;
  const size_t e = (size_t)o.band * I::ITEMS + tid;
  double2* acc = a.acc + ((size_t)o.s * P::VEC + e) * 8;      // 16 sums: 8 double2
  double sum[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double2 v = acc[k];
    sum[2 * k] = v.x;
    sum[2 * k + 1] = v.y;
  }
  const float4* g = a.grads + ((size_t)o.row0 * P::VEC + e) * 4;
  for (int j = o.j0; j < o.j1; ++j, g += (size_t)P::VEC * 4) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float4 v = g[p];
      sum[4 * p + 0] += (double)v.x;
      sum[4 * p + 1] += (double)v.y;
      sum[4 * p + 2] += (double)v.z;
      sum[4 * p + 3] += (double)v.w;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = make_double2(sum[2 * k], sum[2 * k + 1]);
  if (!last) return;
  const uint4 x = src[e];
  const unsigned xw[4] = {x.x, x.y, x.z, x.w}, bw[4] = {x0.x, x0.y, x0.z, x0.w};
  const double K = (double)a.c.steps;
  float4* attr = a.attr + ((size_t)o.s * P::VEC + e) * 4;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int d = (int)((xw[p] >> (8 * c)) & 255u) - (int)((bw[p] >> (8 * c)) & 255u);
      r[c] = (float)(((double)d / 255.0) * (sum[4 * p + c] / K));
    }
    attr[p] = make_float4(r[0], r[1], r[2], r[3]);
  }
}

#endif  // BA3C_INTGRAD_KERNELS

}  // namespace ba3c
