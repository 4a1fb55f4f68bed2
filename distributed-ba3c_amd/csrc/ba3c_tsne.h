// ba3c_tsne.h — exact t-SNE of a set of feature vectors on the device.
// ba3c_amd/tsne.py states the rule in float64 and is the oracle of every kernel here.
//
// Three launches make the joint affinities P from X [N, D], then an iteration is two launches.
//
// Distances.  tsne_means_kernel (float64 column means, rounded once to float32) and
// tsne_center_kernel (a wave per row: Xc = X - mean, the row's |xc|^2 summed in float64 and rounded
// to float32, and the row's max |xc|) are the pre-pass.  tsne_sqdist_kernel computes the Gram matrix
// Xc Xc^T with v_mfma_f32_16x16x32_f16 on the scaled fp16 hi/lo split of ba3c_split.h: a workgroup
// owns one 64 x 64 tile on or above the diagonal, its four waves a 32 x 32 quarter each (2 x 2 MFMA
// tiles).  Per K-step of 32 the 64 rows of both operands are read once (8 floats per thread, zero
// past D and past N: the padding is the loader's), scaled by 2^k (k from the largest |xc|, which
// every workgroup reduces from the per-row maxima: no atomics), split ONCE into an fp16 hi and lo
// plane and staged in LDS at a pitch of 80 bytes per row, so a lane's fragment is one 16-byte LDS
// read; the three products hi hi, hi lo, lo hi accumulate in fp32.  The epilogue forms
// d = max(0, (n_i + n_j) - 2 g) in an LDS tile of pitch 65; the tile on the diagonal is made
// symmetric there (the lower half copies the upper: g_ij and g_ji add their products in different
// orders), and the tile goes out twice, row-wise and, read column-wise from LDS, as the transposed
// tile: both stores are coalesced, and d_ij == d_ji bit for bit by construction.
// 64 x 64 and not 128 x 128: N = 1024 then gives 136 workgroups instead of 36 on 256 CUs, and the
// launch runs once per embedding.
//
// Affinities.  tsne_affinity_kernel: a workgroup per row i.  The row goes to LDS once (N floats);
// every bisection step is one pass over it with exp in float64, sum e and sum d'e reduced per wave
// by cross-lane moves and across the four waves through one double-buffered LDS exchange (one
// barrier per step).  Every thread reads the same four partials in the same order, so the branch
// on H is uniform.  It writes beta_i and the conditional row as float32 into p.
// tsne_symmetrize_kernel then works IN PLACE on p: a workgroup owns the tile pair (a, b), (b, a),
// a <= b, reads both row-wise into LDS, and writes both row-wise as ((double)t + t') / 2N; no
// other workgroup touches the pair, so there is no second N^2 buffer.
//
// The iteration.  tsne_pairs_kernel stages the whole Y in LDS as two planes (x, then y: a lane's
// four neighbours are one 16-byte read per plane, conflict-free), at most 64 KB.  A wave owns
// `rows` consecutive rows i, y_i in registers; its lanes stride j in groups of four, so a row of P
// is read in full contiguous 16-byte lane loads (N a multiple of 4; other N take the scalar
// instantiation).  The terms of a pair are fp32 (1 / (1 + |dy|^2) by v_rcp_f32), the four terms of
// a lane load are added in fp32 and folded into the lane's float64 sums, which the wave reduces by
// cross-lane moves: part[i] = (a_x, a_y, r_x, r_y, z_i, kl_i).  tsne_update_kernel sums z (and kl)
// over all rows in one fixed order in every workgroup, so all of them hold the same bits of Z, and
// a thread applies the gains / velocity / position rule to its row; workgroup 0 writes
// KL = sum kl_i + log Z where the caller asks for it.  No atomics, no waits, no host reads.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ba3c_split.h"   // split2x2, amax_exp, SplitP<2>

namespace ba3c {

struct Tsne {
  static constexpr int MIN_N = 8, MAX_N = 8192, MAX_D = 2048;
  static constexpr int THREADS = 256, WAVES = 4;
  static constexpr int TILE = 64, KSTEP = 32;
  static constexpr int PITCH = 5;          // uint4 per staged row of a plane: 64 bytes of fp16 + 16 of padding
  static constexpr int TP = TILE + 1;      // float pitch of the transposition tile
  static constexpr int MAX_BISECT = 100;
  static constexpr int PART = 6;           // doubles per row: a_x, a_y, r_x, r_y, z, kl
  static constexpr int MEAN_COLS = 64;     // columns of a tsne_means_kernel workgroup
};

// The workspace: the regions that depend on n alone come first, so a caller that knows no d
// (affinities, step) addresses the same `part`
struct TsneWork {
  float* norm;      // [n] |xc_i|^2
  float* rowmax;    // [n] max_k |xc_ik|
  double* part;     // [n][PART]
  float* mean;      // [d]
  float* xc;        // [n][d]
};
inline size_t tsne_work_layout(int n, int d, void* base, TsneWork* w) {
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  char* b = static_cast<char*>(base);
  size_t o = 0;
  TsneWork t;
  t.norm = reinterpret_cast<float*>(b + o), o += al((size_t)n * 4);
  t.rowmax = reinterpret_cast<float*>(b + o), o += al((size_t)n * 4);
  t.part = reinterpret_cast<double*>(b + o), o += al((size_t)n * Tsne::PART * 8);
  t.mean = reinterpret_cast<float*>(b + o), o += al((size_t)d * 4);
  t.xc = reinterpret_cast<float*>(b + o), o += al((size_t)n * d * 4);
  if (w) *w = t;
  return o;
}

struct TsneStepArgs {
  const float* p;
  float2* y;
  float2* vel;
  float2* gains;
  double* part;
  double* kl_out;   // may be null
  int n, rows;      // rows per wave of tsne_pairs_kernel
  double exag, momentum, lr;
};

// rows a wave of tsne_pairs_kernel owns: enough workgroups for the 256 CUs first
inline int tsne_rows_per_wave(int n) { return n >= 4096 ? 4 : (n >= 2048 ? 2 : 1); }

hipError_t launch_tsne_sqdist(hipStream_t s, const float* x, int n, int d, void* work, float* dist);
hipError_t launch_tsne_affinities(hipStream_t s, const float* dist, int n, double log_u, double* beta, float* p);
hipError_t launch_tsne_step(hipStream_t s, const TsneStepArgs& a);

#ifdef BA3C_TSNE_KERNELS   // the device code: ba3c_tsne.hip only

__device__ __forceinline__ double tsne_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float tsne_wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float tsne_wave_min(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- the pre-pass -----------------------------------------------------------------------------

// grid ceil(d / 64): thread (c, g) sums rows g, g + 4, ... of column 64 b + c, the four g in order
__global__ __launch_bounds__(Tsne::THREADS) void tsne_means_kernel(const float* __restrict__ x, int n, int d,
                                                                   float* __restrict__ mean) {
  __shared__ double s_sum[Tsne::WAVES][Tsne::MEAN_COLS];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6, col = blockIdx.x * Tsne::MEAN_COLS + c;
  double acc = 0.0;
  if (col < d)
    for (int r = g; r < n; r += Tsne::WAVES) acc += (double)x[(size_t)r * d + col];
  s_sum[g][c] = acc;
  __syncthreads();
  if (g == 0 && col < d)
    mean[col] = (float)((((s_sum[0][c] + s_sum[1][c]) + s_sum[2][c]) + s_sum[3][c]) / (double)n);
}

// grid ceil(n / 4): a wave per row
__global__ __launch_bounds__(Tsne::THREADS) void tsne_center_kernel(const float* __restrict__ x, int n, int d,
                                                                    const float* __restrict__ mean,
                                                                    float* __restrict__ xc, float* __restrict__ norm,
                                                                    float* __restrict__ rowmax) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * Tsne::WAVES + (threadIdx.x >> 6);
  if (i >= n) return;
  double acc = 0.0;
  float m = 0.f;
  for (int k = lane; k < d; k += 64) {
    const float v = x[(size_t)i * d + k] - mean[k];
    xc[(size_t)i * d + k] = v;
    acc += (double)v * (double)v;
    m = fmaxf(m, fabsf(v));
  }
  acc = tsne_wave_sum(acc);
  m = tsne_wave_max(m);
  if (lane == 0) {
    norm[i] = (float)acc;
    rowmax[i] = m;
  }
}

// ---- the Gram matrix and the distances ----------------------------------------------------------

// grid (T, T), T = ceil(n / 64): workgroup (bx, by) owns rows 64 by .., columns 64 bx .., bx >= by
__global__ __launch_bounds__(Tsne::THREADS) void tsne_sqdist_kernel(const float* __restrict__ xc,
                                                                    const float* __restrict__ norm,
                                                                    const float* __restrict__ rowmax, int n, int d,
                                                                    float* __restrict__ dist) {
  using T = Tsne;
  using SP = SplitP<2>;
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx < by) return;
  __shared__ uint4 s_a[2][T::TILE * T::PITCH];     // [plane][row][k quarter]: 10 240 bytes
  __shared__ uint4 s_b[2][T::TILE * T::PITCH];
  __shared__ float s_t[T::TILE * T::TP];           // 16 640 bytes
  __shared__ float s_max[T::WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;

  float m = 0.f;
  for (int r = tid; r < n; r += T::THREADS) m = fmaxf(m, rowmax[r]);
  m = tsne_wave_max(m);
  if (lane == 0) s_max[wave] = m;
  __syncthreads();
  const int kexp = amax_exp(__float_as_uint(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]))));
  const float sc = exp2i(kexp), unsc = exp2i(-kexp);

  // the loader: thread t stages 8 consecutive k of row t / 4 of both operands
  const int srow = tid >> 2, sq = tid & 3;
  const int arow = by * T::TILE + srow, brow = bx * T::TILE + srow;
  auto stage = [&](int grow, int k0, uint4 (&dst)[2][T::TILE * T::PITCH]) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = k0 + sq * 8 + e;
      v[e] = (grow < n && k < d) ? xc[(size_t)grow * d + k] : 0.f;
    }
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) split2x2(v[2 * e] * sc, v[2 * e + 1] * sc, hi[e], lo[e]);
    dst[0][srow * T::PITCH + sq] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    dst[1][srow * T::PITCH + sq] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  };

  const int wr = wave >> 1, wc = wave & 1;
  f32x4 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) acc[mt][0] = acc[mt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < d; k0 += T::KSTEP) {
    __syncthreads();                               // the previous step's fragments are read
    stage(arow, k0, s_a);
    stage(brow, k0, s_b);
    __syncthreads();
    u32x4 af[2][2], bf[2][2];                      // [plane][m or n tile]
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const uint4 ua = s_a[pl][(wr * 32 + t * 16 + li) * T::PITCH + lq];
        const uint4 ub = s_b[pl][(wc * 32 + t * 16 + li) * T::PITCH + lq];
        af[pl][t] = u32x4{ua.x, ua.y, ua.z, ua.w};
        bf[pl][t] = u32x4{ub.x, ub.y, ub.z, ub.w};
      }
#pragma unroll
    for (int pr = 0; pr < SP::NPROD; ++pr)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          acc[mt][nt] = SP::mfma(af[SP::pa(pr)][mt], bf[SP::pb(pr)][nt], acc[mt][nt]);
  }

  // epilogue: a lane holds rows 4 lq + r, column li of each 16 x 16 tile
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wr * 32 + mt * 16 + 4 * lq + r, col = wc * 32 + nt * 16 + li;
        const int gi = by * T::TILE + row, gj = bx * T::TILE + col;
        const float ni = gi < n ? norm[gi] : 0.f, nj = gj < n ? norm[gj] : 0.f;
        const float g = (acc[mt][nt][r] * unsc) * unsc;
        s_t[row * T::TP + col] = gi == gj ? 0.f : fmaxf(0.f, (ni + nj) - 2.f * g);
      }
  __syncthreads();
  if (bx == by) {
    for (int e = tid; e < T::TILE * T::TILE; e += T::THREADS) {
      const int r = e >> 6, c = e & 63;
      if (r > c) s_t[r * T::TP + c] = s_t[c * T::TP + r];
    }
    __syncthreads();
  }
  for (int e = tid; e < T::TILE * T::TILE; e += T::THREADS) {
    const int r = e >> 6, c = e & 63;
    const int gi = by * T::TILE + r, gj = bx * T::TILE + c;
    if (gi < n && gj < n) dist[(size_t)gi * n + gj] = s_t[r * T::TP + c];
    const int ti = bx * T::TILE + r, tj = by * T::TILE + c;          // the transposed tile
    if (bx != by && ti < n && tj < n) dist[(size_t)ti * n + tj] = s_t[c * T::TP + r];
  }
}

// ---- the affinities ---------------------------------------------------------------------------

// grid n, dynamic LDS n floats
__global__ __launch_bounds__(Tsne::THREADS) void tsne_affinity_kernel(const float* __restrict__ dist, int n,
                                                                      double log_u, double* __restrict__ beta_out,
                                                                      float* __restrict__ pc) {
  using T = Tsne;
  extern __shared__ float s_row[];
  __shared__ double s_red[2][T::WAVES][2];
  __shared__ float s_min[T::WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x;
  float mn = __builtin_inff();
  for (int j = tid; j < n; j += T::THREADS) {
    const float v = dist[(size_t)i * n + j];
    s_row[j] = v;
    if (j != i) mn = fminf(mn, v);
  }
  mn = tsne_wave_min(mn);
  if (lane == 0) s_min[wave] = mn;
  __syncthreads();
  const double dmin = (double)fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));

  double beta = 1.0, lo = -__builtin_inf(), hi = __builtin_inf(), sum = 1.0;
  for (int it = 0; it <= T::MAX_BISECT; ++it) {
    double se = 0.0, sde = 0.0;
    for (int j = tid; j < n; j += T::THREADS) {
      if (j == i) continue;
      const double dm = (double)s_row[j] - dmin, e = exp(-beta * dm);
      se += e;
      sde += dm * e;
    }
    se = tsne_wave_sum(se);
    sde = tsne_wave_sum(sde);
    double(*slot)[2] = s_red[it & 1];              // two slots: one barrier per step
    if (lane == 0) slot[wave][0] = se, slot[wave][1] = sde;
    __syncthreads();
    sum = ((slot[0][0] + slot[1][0]) + slot[2][0]) + slot[3][0];
    const double sd = ((slot[0][1] + slot[1][1]) + slot[2][1]) + slot[3][1];
    const double h = log(sum) + beta * sd / sum;
    if (fabs(h - log_u) <= 1e-5 || it == T::MAX_BISECT) break;   // uniform: every thread holds the same h
    if (h > log_u) {
      lo = beta;
      beta = hi == __builtin_inf() ? beta * 2.0 : 0.5 * (beta + hi);
    } else {
      hi = beta;
      beta = lo == -__builtin_inf() ? beta * 0.5 : 0.5 * (beta + lo);
    }
  }
  for (int j = tid; j < n; j += T::THREADS)
    pc[(size_t)i * n + j] = j == i ? 0.f : (float)(exp(-beta * ((double)s_row[j] - dmin)) / sum);
  if (tid == 0) beta_out[i] = beta;
}

// grid (T, T): workgroup (bx, by), bx >= by, owns tiles (by, bx) and (bx, by) of p, in place
__global__ __launch_bounds__(Tsne::THREADS) void tsne_symmetrize_kernel(float* __restrict__ p, int n) {
  using T = Tsne;
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx < by) return;
  __shared__ float s_u[T::TILE * T::TP], s_l[T::TILE * T::TP];   // tile (by, bx) and tile (bx, by)
  const int tid = threadIdx.x;
  for (int e = tid; e < T::TILE * T::TILE; e += T::THREADS) {
    const int r = e >> 6, c = e & 63;
    const int ui = by * T::TILE + r, uj = bx * T::TILE + c, li = bx * T::TILE + r, lj = by * T::TILE + c;
    s_u[r * T::TP + c] = (ui < n && uj < n) ? p[(size_t)ui * n + uj] : 0.f;
    s_l[r * T::TP + c] = (li < n && lj < n) ? p[(size_t)li * n + lj] : 0.f;
  }
  __syncthreads();                                 // both tiles are read before either is written
  const double two_n = 2.0 * (double)n;
  for (int e = tid; e < T::TILE * T::TILE; e += T::THREADS) {
    const int r = e >> 6, c = e & 63;
    const int ui = by * T::TILE + r, uj = bx * T::TILE + c, li = bx * T::TILE + r, lj = by * T::TILE + c;
    if (ui < n && uj < n)
      p[(size_t)ui * n + uj] = (float)(((double)s_u[r * T::TP + c] + (double)s_l[c * T::TP + r]) / two_n);
    if (bx != by && li < n && lj < n)
      p[(size_t)li * n + lj] = (float)(((double)s_u[c * T::TP + r] + (double)s_l[r * T::TP + c]) / two_n);
  }
}

// ---- the iteration ----------------------------------------------------------------------------

// the fp32 terms of the pair (i, j): own = (j == i)
template <bool KL>
__device__ __forceinline__ void tsne_pair(float p, float xi, float yi, float xj, float yj, bool own, float& ax,
                                          float& ay, float& rx, float& ry, float& z, float& kl) {
  const float dx = xi - xj, dy = yi - yj, t = 1.f + (dx * dx + dy * dy);
  const float q = own ? 0.f : __builtin_amdgcn_rcpf(t), pq = p * q, qq = q * q;
  ax += pq * dx;
  ay += pq * dy;
  rx += qq * dx;
  ry += qq * dy;
  z += q;
  if (KL) kl += p * logf(fmaxf(p, 1e-12f) * t);    // p_ii = 0
}

// grid ceil(n / (4 rows)), dynamic LDS 2 n floats: x plane, y plane
template <bool VEC, bool KL>
__global__ __launch_bounds__(Tsne::THREADS) void tsne_pairs_kernel(TsneStepArgs a) {
  using T = Tsne;
  extern __shared__ float4 s_y4[];
  float* sx = reinterpret_cast<float*>(s_y4);
  float* sy = sx + a.n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n;
  for (int j = tid; j < n; j += T::THREADS) {
    const float2 v = a.y[j];
    sx[j] = v.x;
    sy[j] = v.y;
  }
  __syncthreads();
  const int row0 = ((int)blockIdx.x * T::WAVES + wave) * a.rows;
  for (int r = 0; r < a.rows; ++r) {
    const int i = row0 + r;
    if (i >= n) break;                             // uniform in the wave
    const float xi = sx[i], yi = sy[i];
    const float* prow = a.p + (size_t)i * n;
    double acc[T::PART] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (VEC) {
      for (int j = 4 * lane; j < n; j += 256) {
        const float4 pv = *reinterpret_cast<const float4*>(prow + j);
        const float4 xj = *reinterpret_cast<const float4*>(sx + j), yj = *reinterpret_cast<const float4*>(sy + j);
        float f[T::PART] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        tsne_pair<KL>(pv.x, xi, yi, xj.x, yj.x, j == i, f[0], f[1], f[2], f[3], f[4], f[5]);
        tsne_pair<KL>(pv.y, xi, yi, xj.y, yj.y, j + 1 == i, f[0], f[1], f[2], f[3], f[4], f[5]);
        tsne_pair<KL>(pv.z, xi, yi, xj.z, yj.z, j + 2 == i, f[0], f[1], f[2], f[3], f[4], f[5]);
        tsne_pair<KL>(pv.w, xi, yi, xj.w, yj.w, j + 3 == i, f[0], f[1], f[2], f[3], f[4], f[5]);
#pragma unroll
        for (int k = 0; k < T::PART; ++k) acc[k] += (double)f[k];
      }
    } else {
      for (int j = lane; j < n; j += 64) {
        float f[T::PART] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        tsne_pair<KL>(prow[j], xi, yi, sx[j], sy[j], j == i, f[0], f[1], f[2], f[3], f[4], f[5]);
#pragma unroll
        for (int k = 0; k < T::PART; ++k) acc[k] += (double)f[k];
      }
    }
#pragma unroll
    for (int k = 0; k < T::PART; ++k) acc[k] = tsne_wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < T::PART; ++k) a.part[(size_t)i * T::PART + k] = acc[k];
    }
  }
}

// grid ceil(n / 256): a thread per row, after every workgroup has summed Z in the same order
__global__ __launch_bounds__(Tsne::THREADS) void tsne_update_kernel(TsneStepArgs a) {
#pragma clang fp contract(off)
  using T = Tsne;
  __shared__ double s_red[T::WAVES][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n;
  double z = 0.0, kl = 0.0;
  for (int j = tid; j < n; j += T::THREADS) {
    z += a.part[(size_t)j * T::PART + 4];
    kl += a.part[(size_t)j * T::PART + 5];
  }
  z = tsne_wave_sum(z);
  kl = tsne_wave_sum(kl);
  if (lane == 0) s_red[wave][0] = z, s_red[wave][1] = kl;
  __syncthreads();
  const double Z = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
  if (a.kl_out && blockIdx.x == 0 && tid == 0)
    *a.kl_out = (((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1]) + log(Z);
  const int i = (int)blockIdx.x * T::THREADS + tid;
  if (i >= n) return;
  const double* pt = a.part + (size_t)i * T::PART;
  const float2 y = a.y[i], u = a.vel[i], g = a.gains[i];
  const float yv[2] = {y.x, y.y}, uv[2] = {u.x, u.y}, gv[2] = {g.x, g.y};
  float yo[2], uo[2], go[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double grad = 4.0 * (a.exag * pt[c] - pt[2 + c] / Z);
    const bool flip = (grad > 0.0) != (uv[c] > 0.f);
    go[c] = fmaxf(flip ? gv[c] + 0.2f : gv[c] * 0.8f, 0.01f);
    uo[c] = (float)(a.momentum * (double)uv[c] - a.lr * (double)go[c] * grad);
    yo[c] = yv[c] + uo[c];
  }
  a.y[i] = make_float2(yo[0], yo[1]);
  a.vel[i] = make_float2(uo[0], uo[1]);
  a.gains[i] = make_float2(go[0], go[1]);
}

#endif  // BA3C_TSNE_KERNELS

}  // namespace ba3c
