// ba3c_pca.h — the leading principal components of a feature matrix on the device (DESIGN.md
// section 25).  ba3c_amd/pca.py states the rule in float64 and is the oracle of every kernel here.
// The kernels live in ba3c_tsne.hip's translation unit: the same flags, no further code object.
//
// Scatter.  C = Xc^T Xc is D x D with the long reduction over the rows n, read down the columns of
// Xc [N][D] (tsne_means_kernel and tsne_center_kernel make Xc and the per-row maxima, as for the
// distances).  pca_scatter_kernel: a workgroup owns one 64 x 64 tile of C on or above the diagonal
// over one chunk of rows, its four waves a 32 x 32 quarter each (2 x 2 v_mfma_f32_16x16x32_f16
// tiles), the three products hi hi, hi lo, lo hi of the scaled fp16 split accumulating in fp32.
// The MFMA wants a lane's eight K values contiguous, and K is the row n, so the loader transposes
// for free: in a K-step of 32 rows thread (c = tid & 63, g = tid >> 6) loads column 64 b + c of rows
// 8 g .. 8 g + 7 (each of the eight loads is one coalesced 256-byte row segment per wave), then
// holds eight n-consecutive values of one column, scales and splits them once and writes ONE
// 16-byte LDS entry per plane at [c][g], the 80-byte-pitch layout whose fragment reads
// tsne_sqdist_kernel already uses.  Zeros past the chunk, past N and past D are the loader's.  A
// tile on the diagonal stages one operand only.  The row chunks are multiples of 32 rows chosen so
// that the launch has at least 256 workgroups where N and D allow (pca_chunks); a workgroup stores
// its raw fp32 accumulators (still scaled by 2^2k) as a partial tile: no atomics.  The partials
// take (chunks x tile pairs) x 16 KiB, and pca_chunks caps chunks x pairs at 528 (D = 2048, one
// chunk; below 256 pairs it stays under 256 + pairs): 8.25 MiB at the most.
// pca_scatter_reduce_kernel sums a tile's partials in chunk order in float64, removes the scale
// (a power of two: exact) and writes C float64 [D][D]; the tile below the diagonal is the
// transposed copy of the same sums (and the lower half of a diagonal tile copies its upper half),
// so C is symmetric bit for bit.
//
// Block iteration.  Q and Z are float64 [D][8]: columns past m = min(8, D) are zero, stay zero
// under the zero-column rule and touch no other column, so no kernel branches on m.
// pca_multiply_kernel (Z = C Q): a wave owns two rows of C, its lanes stride the columns in
// contiguous loads, each with eight float64 accumulators per row and Q's row as four 16-byte loads;
// a cross-lane float64 sum ends it.  C is read once per sweep.  pca_orth_kernel: ONE workgroup,
// modified Gram-Schmidt with the projection pass applied twice.  A thread owns rows tid, tid + 256,
// ... of every column, the current column in registers, and is the only reader and writer of its
// rows of Q; a dot product is the thread's rows in order, a cross-lane sum and the four waves'
// partials added in order through a double-buffered LDS slot (one barrier per dot product).
// A sweep is these two launches.
//
// Rayleigh-Ritz.  pca_ritz_kernel, one workgroup: G = Q^T Z (wave w the rows 2 w, 2 w + 1 of G),
// H = (G + G^T) / 2, thread 0 runs the cyclic Jacobi on H in LDS (Pca::JACOBI_SWEEPS sweeps over
// the pairs (p, q), p < q, row by row) and sorts; then per kept component all threads form
// v = Q w and C v = Z w for their rows, reduce the residual and the first entry of largest
// magnitude, and write the float32 component with that entry positive.
//
// Projection.  pca_project_kernel: a wave per row of Xc, float64 sums, float32 scores, and where
// asked Y0 from the first two scores and l_1, read on the device.
#pragma once

#include "ba3c_tsne.h"

namespace ba3c {

struct Pca {
  static constexpr int M = 8;                       // columns of Q, Z, H
  static constexpr int MAX_SWEEPS = 256, JACOBI_SWEEPS = 12;
  static constexpr int THREADS = 256, WAVES = 4;
  static constexpr int TILE = Tsne::TILE, KSTEP = Tsne::KSTEP, PITCH = Tsne::PITCH;
  static constexpr int TILE_EL = TILE * TILE;
  static constexpr int DP = TILE + 1;               // double pitch of the reduce kernel's tile
  static constexpr int TARGET_WGS = 256;            // workgroups the scatter launch aims for
  static constexpr int OWN = Tsne::MAX_D / THREADS; // rows of a column a thread of the one-workgroup kernels owns
  static constexpr int MUL_ROWS = 2;                // rows of C per wave of pca_multiply_kernel
};

inline int pca_tiles(int d) { return (d + Pca::TILE - 1) / Pca::TILE; }
inline int pca_pairs(int d) { return pca_tiles(d) * (pca_tiles(d) + 1) / 2; }
// rows per chunk (a multiple of 32) and the number of chunks; every chunk holds a row
inline void pca_chunks(int n, int d, int* rows, int* chunks) {
  const int steps = (n + Pca::KSTEP - 1) / Pca::KSTEP, pairs = pca_pairs(d);
  const int want = (Pca::TARGET_WGS + pairs - 1) / pairs;
  const int c = steps < want ? steps : want, per = (steps + c - 1) / c;
  *rows = per * Pca::KSTEP;
  *chunks = (steps + per - 1) / per;
}

// The workspace.  The scatter and the projection use the t-SNE pre-pass regions and, after them,
// the exponent and the partial tiles.  ba3c_pca_components knows no n: its Q and Z lie at the base
// and overlay the pre-pass regions, which nothing reads once a call that filled them has returned.
struct PcaWork {
  int* kexp;        // the scale exponent of the scatter launch
  float* part;      // [chunks][pairs][64][64]
  double* q;        // [d][8]
  double* z;        // [d][8]
};
inline size_t pca_work_layout(int n, int d, void* base, TsneWork* tw, PcaWork* w) {
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  char* b = static_cast<char*>(base);
  size_t o = tsne_work_layout(n, d, base, tw);
  int rows, chunks;
  pca_chunks(n, d, &rows, &chunks);
  PcaWork p;
  p.kexp = reinterpret_cast<int*>(b + o), o += 256;
  p.part = reinterpret_cast<float*>(b + o), o += al((size_t)chunks * pca_pairs(d) * Pca::TILE_EL * 4);
  const size_t qz = al((size_t)d * Pca::M * 8);
  p.q = reinterpret_cast<double*>(b);
  p.z = reinterpret_cast<double*>(b + qz);
  if (w) *w = p;
  return o > 2 * qz ? o : 2 * qz;
}

hipError_t launch_pca_scatter(hipStream_t s, const float* x, int n, int d, void* work, double* c);
hipError_t launch_pca_components(hipStream_t s, const double* c, int d, const double* trace, const double* q0, int k,
                                 int sweeps, void* work, float* components, double* eigvals, double* ratio,
                                 double* resid);
hipError_t launch_pca_project(hipStream_t s, const float* x, int n, int d, const float* components, int k,
                              const double* eigvals, void* work, float* scores, float* y0);

#ifdef BA3C_TSNE_KERNELS   // the device code: ba3c_tsne.hip only

// ---- the scatter matrix ------------------------------------------------------------------------

// grid (T, T, chunks), T = ceil(d / 64): workgroup (bx, by, ch), bx >= by, owns rows 64 by .. and
// columns 64 bx .. of C over the rows [ch chunk_rows, (ch + 1) chunk_rows) of xc
__global__ __launch_bounds__(Pca::THREADS) void pca_scatter_kernel(const float* __restrict__ xc,
                                                                   const float* __restrict__ rowmax, int n, int d,
                                                                   int chunk_rows, float* __restrict__ part,
                                                                   int* __restrict__ kexp_out) {
  using P = Pca;
  using SP = SplitP<2>;
  const int bx = blockIdx.x, by = blockIdx.y, ch = blockIdx.z;
  if (bx < by) return;
  __shared__ uint4 s_a[2][P::TILE * P::PITCH];     // [plane][column of xc][row quarter]: 10 240 bytes
  __shared__ uint4 s_b[2][P::TILE * P::PITCH];
  __shared__ float s_max[P::WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;

  float m = 0.f;
  for (int r = tid; r < n; r += P::THREADS) m = fmaxf(m, rowmax[r]);
  m = tsne_wave_max(m);
  if (lane == 0) s_max[wave] = m;
  __syncthreads();
  const int kexp = amax_exp(__float_as_uint(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]))));
  if (bx == 0 && by == 0 && ch == 0 && tid == 0) *kexp_out = kexp;
  const float sc = exp2i(kexp);
  const int r0 = ch * chunk_rows, r1 = min(n, r0 + chunk_rows);
  const bool diag = bx == by;

  // the loader: thread (c, g) stages rows k0 + 8 g .. + 7 of column `col`; a wave's load e is the
  // 64 consecutive floats of row k0 + 8 g + e
  const int c = lane, g = wave;
  auto stage = [&](int col, int k0, uint4 (&dst)[2][P::TILE * P::PITCH]) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = k0 + g * 8 + e;
      v[e] = (row < r1 && col < d) ? xc[(size_t)row * d + col] : 0.f;
    }
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) split2x2(v[2 * e] * sc, v[2 * e + 1] * sc, hi[e], lo[e]);
    dst[0][c * P::PITCH + g] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    dst[1][c * P::PITCH + g] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  };
  const uint4(*sb)[P::TILE * P::PITCH] = diag ? s_a : s_b;

  const int wr = wave >> 1, wc = wave & 1;
  f32x4 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) acc[mt][0] = acc[mt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = r0; k0 < r1; k0 += P::KSTEP) {
    __syncthreads();                               // the previous step's fragments are read
    stage(by * P::TILE + c, k0, s_a);
    if (!diag) stage(bx * P::TILE + c, k0, s_b);
    __syncthreads();
    u32x4 af[2][2], bf[2][2];                      // [plane][m or n tile]
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const uint4 ua = s_a[pl][(wr * 32 + t * 16 + li) * P::PITCH + lq];
        const uint4 ub = sb[pl][(wc * 32 + t * 16 + li) * P::PITCH + lq];
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

  // the partial tile, still scaled: a lane holds rows 4 lq + r, column li of each 16 x 16 tile
  const int tiles = gridDim.x, pair = by * tiles - by * (by - 1) / 2 + (bx - by);
  float* out = part + ((size_t)ch * (tiles * (tiles + 1) / 2) + pair) * P::TILE_EL;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(wr * 32 + mt * 16 + 4 * lq + r) * P::TILE + wc * 32 + nt * 16 + li] = acc[mt][nt][r];
}

// grid (T, T): workgroup (bx, by), bx >= by, writes tiles (by, bx) and (bx, by) of C
__global__ __launch_bounds__(Pca::THREADS) void pca_scatter_reduce_kernel(const float* __restrict__ part,
                                                                          const int* __restrict__ kexp, int d,
                                                                          int chunks, double* __restrict__ cmat) {
  using P = Pca;
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx < by) return;
  __shared__ double s_t[P::TILE * P::DP];          // 33 280 bytes
  const int tid = threadIdx.x, tiles = gridDim.x, pairs = tiles * (tiles + 1) / 2;
  const int pair = by * tiles - by * (by - 1) / 2 + (bx - by);
  const double unsc2 = __hiloint2double((1023 - 2 * kexp[0]) << 20, 0);   // 2^(-2 k), |k| <= 100
  for (int e = tid; e < P::TILE_EL; e += P::THREADS) {
    double sum = 0.0;
    for (int ch = 0; ch < chunks; ++ch) sum += (double)part[((size_t)ch * pairs + pair) * P::TILE_EL + e];
    s_t[(e >> 6) * P::DP + (e & 63)] = sum * unsc2;
  }
  __syncthreads();
  if (bx == by) {                                   // c_ij and c_ji added their products in different orders
    for (int e = tid; e < P::TILE_EL; e += P::THREADS) {
      const int r = e >> 6, c = e & 63;
      if (r > c) s_t[r * P::DP + c] = s_t[c * P::DP + r];
    }
    __syncthreads();
  }
  for (int e = tid; e < P::TILE_EL; e += P::THREADS) {
    const int r = e >> 6, c = e & 63;
    const int gi = by * P::TILE + r, gj = bx * P::TILE + c;
    if (gi < d && gj < d) cmat[(size_t)gi * d + gj] = s_t[r * P::DP + c];
    const int ti = bx * P::TILE + r, tj = by * P::TILE + c;          // the transposed tile
    if (bx != by && ti < d && tj < d) cmat[(size_t)ti * d + tj] = s_t[c * P::DP + r];
  }
}

// ---- the block iteration -----------------------------------------------------------------------

// a row of Q or Z: eight doubles, 64-byte aligned
__device__ __forceinline__ void pca_row8(const double* __restrict__ p, double (&v)[Pca::M]) {
#pragma unroll
  for (int j = 0; j < Pca::M; j += 2) {
    const double2 t = *reinterpret_cast<const double2*>(p + j);
    v[j] = t.x;
    v[j + 1] = t.y;
  }
}

// grid ceil(d / 8): wave w of workgroup b owns rows 2 (4 b + w), + 1 of C
__global__ __launch_bounds__(Pca::THREADS) void pca_multiply_kernel(const double* __restrict__ cmat,
                                                                    const double* __restrict__ q, int d,
                                                                    double* __restrict__ z) {
  using P = Pca;
  const int lane = threadIdx.x & 63, row0 = ((int)blockIdx.x * P::WAVES + (threadIdx.x >> 6)) * P::MUL_ROWS;
  if (row0 >= d) return;
  const bool two = row0 + 1 < d;
  const double* c0 = cmat + (size_t)row0 * d;
  const double* c1 = c0 + (two ? d : 0);
  double acc[P::MUL_ROWS][P::M];
#pragma unroll
  for (int j = 0; j < P::M; ++j) acc[0][j] = acc[1][j] = 0.0;
  for (int col = lane; col < d; col += 64) {
    double qv[P::M];
    pca_row8(q + (size_t)col * P::M, qv);
    const double a = c0[col], b = c1[col];
#pragma unroll
    for (int j = 0; j < P::M; ++j) {
      acc[0][j] += a * qv[j];
      acc[1][j] += b * qv[j];
    }
  }
#pragma unroll
  for (int r = 0; r < P::MUL_ROWS; ++r)
#pragma unroll
    for (int j = 0; j < P::M; ++j) acc[r][j] = tsne_wave_sum(acc[r][j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < P::M; ++j) {
      z[(size_t)row0 * P::M + j] = acc[0][j];
      if (two) z[(size_t)(row0 + 1) * P::M + j] = acc[1][j];
    }
  }
}

// the workgroup's sum of v in one fixed order: the lanes, then the four waves in order.  `slot`
// alternates between two LDS slots, so a sum costs one barrier
__device__ __forceinline__ double pca_block_sum(double v, double (*s_red)[Pca::WAVES], int& slot) {
  v = tsne_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_red[slot][threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((s_red[slot][0] + s_red[slot][1]) + s_red[slot][2]) + s_red[slot][3];
  slot ^= 1;
  return r;
}

// one workgroup: q [d][8] = orth(src), src [d][pitch] with `cols` columns (the others are zero).
// q may be read only by the thread that wrote the row: a thread owns rows tid + 256 r
__global__ __launch_bounds__(Pca::THREADS) void pca_orth_kernel(const double* __restrict__ src, int pitch, int cols,
                                                                int d, double* q) {
#pragma clang fp contract(off)
  using P = Pca;
  __shared__ double s_red[2][P::WAVES];
  const int tid = threadIdx.x;
  int slot = 0;
  for (int j = 0; j < P::M; ++j) {
    double zc[P::OWN], ss = 0.0;
#pragma unroll
    for (int r = 0; r < P::OWN; ++r) {
      const int row = tid + P::THREADS * r;
      zc[r] = (row < d && j < cols) ? src[(size_t)row * pitch + j] : 0.0;
      ss += zc[r] * zc[r];
    }
    const double before = sqrt(pca_block_sum(ss, s_red, slot));
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < j; ++i) {
        double qi[P::OWN], dot = 0.0;
#pragma unroll
        for (int r = 0; r < P::OWN; ++r) {
          const int row = tid + P::THREADS * r;
          qi[r] = row < d ? q[(size_t)row * P::M + i] : 0.0;
          dot += qi[r] * zc[r];
        }
        dot = pca_block_sum(dot, s_red, slot);
#pragma unroll
        for (int r = 0; r < P::OWN; ++r) zc[r] -= dot * qi[r];
      }
    ss = 0.0;
#pragma unroll
    for (int r = 0; r < P::OWN; ++r) ss += zc[r] * zc[r];
    const double after = sqrt(pca_block_sum(ss, s_red, slot));
    const bool zero = after == 0.0 || after <= 0x1p-40 * before;
#pragma unroll
    for (int r = 0; r < P::OWN; ++r) {
      const int row = tid + P::THREADS * r;
      if (row < d) q[(size_t)row * P::M + j] = zero ? 0.0 : zc[r] / after;
    }
  }
}

// ---- Rayleigh-Ritz -----------------------------------------------------------------------------

struct PcaRitzArgs {
  const double* q;        // [d][8] orthonormal (or zero) columns
  const double* z;        // [d][8] C q
  const double* cmat;     // [d][d], read on its diagonal where trace is null
  const double* trace;    // may be null
  int d, m, k;
  float* components;      // [k][d]
  double* eigvals;        // [k]
  double* ratio;          // [k]
  double* resid;          // [k]
};

// one workgroup
__global__ __launch_bounds__(Pca::THREADS) void pca_ritz_kernel(PcaRitzArgs a) {
#pragma clang fp contract(off)
  using P = Pca;
  __shared__ double s_red[2][P::WAVES];
  __shared__ double s_h[P::M][P::M], s_w[P::M][P::M], s_eig[P::M], s_trace;
  __shared__ int s_ord[P::M];
  __shared__ double s_bv[P::WAVES];
  __shared__ int s_bi[P::WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = a.d, m = a.m;
  int slot = 0;

  // G = Q^T Z: wave w the rows 2 w and 2 w + 1, lanes stride the rows of Q and Z
  {
    double g[2][P::M];
#pragma unroll
    for (int j = 0; j < P::M; ++j) g[0][j] = g[1][j] = 0.0;
    for (int row = lane; row < d; row += 64) {
      double zv[P::M];
      pca_row8(a.z + (size_t)row * P::M, zv);
      const double2 qv = *reinterpret_cast<const double2*>(a.q + (size_t)row * P::M + 2 * wave);
#pragma unroll
      for (int j = 0; j < P::M; ++j) {
        g[0][j] += qv.x * zv[j];
        g[1][j] += qv.y * zv[j];
      }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int j = 0; j < P::M; ++j) {
        const double v = tsne_wave_sum(g[p][j]);
        if (lane == 0) s_w[2 * wave + p][j] = v;   // G, until thread 0 has formed H
      }
  }
  double tr = 0.0;
  if (!a.trace)
    for (int i = tid; i < d; i += P::THREADS) tr += a.cmat[(size_t)i * d + i];
  tr = pca_block_sum(tr, s_red, slot);             // its barrier also publishes G

  if (tid == 0) {
    s_trace = a.trace ? a.trace[0] : tr;
    for (int p = 0; p < P::M; ++p)
      for (int q = p; q < P::M; ++q) s_h[p][q] = s_h[q][p] = (s_w[p][q] + s_w[q][p]) / 2.0;
    for (int p = 0; p < P::M; ++p)
      for (int q = 0; q < P::M; ++q) s_w[p][q] = p == q ? 1.0 : 0.0;
    for (int sweep = 0; sweep < P::JACOBI_SWEEPS; ++sweep)
      for (int p = 0; p + 1 < m; ++p)
        for (int q = p + 1; q < m; ++q) {
          const double hpq = s_h[p][q];
          if (hpq == 0.0) continue;
          const double theta = (s_h[q][q] - s_h[p][p]) / (2.0 * hpq);
          const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          for (int i = 0; i < m; ++i) {            // columns p and q of H and of W
            const double hp = s_h[i][p], hq = s_h[i][q], wp = s_w[i][p], wq = s_w[i][q];
            s_h[i][p] = c * hp - s * hq;
            s_h[i][q] = s * hp + c * hq;
            s_w[i][p] = c * wp - s * wq;
            s_w[i][q] = s * wp + c * wq;
          }
          for (int i = 0; i < m; ++i) {            // rows p and q of H
            const double hp = s_h[p][i], hq = s_h[q][i];
            s_h[p][i] = c * hp - s * hq;
            s_h[q][i] = s * hp + c * hq;
          }
        }
    // descending, stable: an insertion sort of the indices
    for (int i = 0; i < m; ++i) {
      int at = i;
      while (at > 0 && s_h[s_ord[at - 1]][s_ord[at - 1]] < s_h[i][i]) {
        s_ord[at] = s_ord[at - 1];
        --at;
      }
      s_ord[at] = i;
    }
    for (int i = 0; i < m; ++i) s_eig[i] = s_h[s_ord[i]][s_ord[i]];
  }
  __syncthreads();

  const double l1 = s_eig[0], trace = s_trace;
  for (int j = 0; j < a.k; ++j) {
    const int col = s_ord[j];
    const double lj = s_eig[j];
    double v[P::OWN], ss = 0.0, best = 0.0;
    int besti = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < P::OWN; ++r) {
      const int row = tid + P::THREADS * r;
      double qv[P::M], zv[P::M], cv = 0.0;
      v[r] = 0.0;
      if (row < d) {
        pca_row8(a.q + (size_t)row * P::M, qv);
        pca_row8(a.z + (size_t)row * P::M, zv);
#pragma unroll
        for (int i = 0; i < P::M; ++i) {           // past m: a zero column of Q and Z times W's identity
          v[r] += qv[i] * s_w[i][col];
          cv += zv[i] * s_w[i][col];
        }
        const double e = cv - lj * v[r];
        ss += e * e;
        if (fabs(v[r]) > fabs(best) || besti == 0x7fffffff) best = v[r], besti = row;   // rows ascend: the first stays
      }
    }
    ss = pca_block_sum(ss, s_red, slot);
    // the first entry of largest magnitude: lanes, then waves
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(besti, o, 64);
      if (fabs(ob) > fabs(best) || (fabs(ob) == fabs(best) && oi < besti)) best = ob, besti = oi;
    }
    if (lane == 0) s_bv[wave] = best, s_bi[wave] = besti;
    __syncthreads();
    best = s_bv[0], besti = s_bi[0];
    for (int w = 1; w < P::WAVES; ++w)
      if (fabs(s_bv[w]) > fabs(best) || (fabs(s_bv[w]) == fabs(best) && s_bi[w] < besti)) best = s_bv[w], besti = s_bi[w];
    const bool neg = best < 0.0;
#pragma unroll
    for (int r = 0; r < P::OWN; ++r) {
      const int row = tid + P::THREADS * r;
      if (row < d) a.components[(size_t)j * d + row] = (float)(neg ? -v[r] : v[r]);
    }
    if (tid == 0) {
      a.eigvals[j] = lj;
      a.ratio[j] = trace > 0.0 ? lj / trace : 0.0;
      a.resid[j] = l1 > 0.0 ? sqrt(ss) / l1 : 0.0;
    }
    __syncthreads();                               // s_bv and s_bi are read before the next component
  }
}

// ---- the projection ----------------------------------------------------------------------------

// grid ceil(n / 4): a wave per row of xc
__global__ __launch_bounds__(Pca::THREADS) void pca_project_kernel(const float* __restrict__ xc, int n, int d,
                                                                   const float* __restrict__ components, int k,
                                                                   const double* __restrict__ eigvals,
                                                                   float* __restrict__ scores, float2* __restrict__ y0) {
#pragma clang fp contract(off)
  using P = Pca;
  const int lane = threadIdx.x & 63, i = (int)blockIdx.x * P::WAVES + (threadIdx.x >> 6);
  if (i >= n) return;
  double acc[P::M];
#pragma unroll
  for (int j = 0; j < P::M; ++j) acc[j] = 0.0;
  for (int col = lane; col < d; col += 64) {
    const double xv = (double)xc[(size_t)i * d + col];
#pragma unroll
    for (int j = 0; j < P::M; ++j)
      if (j < k) acc[j] += xv * (double)components[(size_t)j * d + col];
  }
  float sc[P::M];
#pragma unroll
  for (int j = 0; j < P::M; ++j) sc[j] = (float)tsne_wave_sum(acc[j]);
  if (lane != 0) return;
#pragma unroll
  for (int j = 0; j < P::M; ++j)
    if (j < k) scores[(size_t)i * k + j] = sc[j];
  const double l1 = eigvals[0];
  if (y0 && l1 > 0.0) {                            // l_1 = 0: y0 keeps what the caller drew
    const double sd = sqrt(l1 / (double)n);
    y0[i] = make_float2((float)(1e-4 * (double)sc[0] / sd), k > 1 ? (float)(1e-4 * (double)sc[1] / sd) : 0.f);
  }
}

#endif  // BA3C_TSNE_KERNELS

}  // namespace ba3c
