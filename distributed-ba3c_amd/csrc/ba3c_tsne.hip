// ba3c_tsne.hip — the t-SNE kernels (ba3c_tsne.h) and the PCA kernels (ba3c_pca.h) in a translation
// unit of their own, compiled without packed fp32 VALU operations (Makefile).  ba3c_capi.hip
// launches them through the host functions below.
#include <hip/hip_runtime.h>

#define BA3C_TSNE_KERNELS 1
#include "ba3c_tsne.h"
#include "ba3c_pca.h"

namespace ba3c {

#define TSNE_LAUNCHED()                                    \
  do {                                                     \
    const hipError_t _e = hipGetLastError();               \
    if (_e != hipSuccess) return _e;                       \
  } while (0)

hipError_t launch_tsne_sqdist(hipStream_t s, const float* x, int n, int d, void* work, float* dist) {
  using T = Tsne;
  TsneWork w;
  tsne_work_layout(n, d, work, &w);
  const dim3 block(T::THREADS);
  const int tiles = (n + T::TILE - 1) / T::TILE;
  hipLaunchKernelGGL(tsne_means_kernel, dim3((d + T::MEAN_COLS - 1) / T::MEAN_COLS), block, 0, s, x, n, d, w.mean);
  TSNE_LAUNCHED();
  hipLaunchKernelGGL(tsne_center_kernel, dim3((n + T::WAVES - 1) / T::WAVES), block, 0, s, x, n, d, w.mean, w.xc,
                     w.norm, w.rowmax);
  TSNE_LAUNCHED();
  hipLaunchKernelGGL(tsne_sqdist_kernel, dim3(tiles, tiles), block, 0, s, w.xc, w.norm, w.rowmax, n, d, dist);
  return hipGetLastError();
}

hipError_t launch_tsne_affinities(hipStream_t s, const float* dist, int n, double log_u, double* beta, float* p) {
  using T = Tsne;
  const int tiles = (n + T::TILE - 1) / T::TILE;
  hipLaunchKernelGGL(tsne_affinity_kernel, dim3(n), dim3(T::THREADS), (size_t)n * sizeof(float), s, dist, n, log_u,
                     beta, p);
  TSNE_LAUNCHED();
  hipLaunchKernelGGL(tsne_symmetrize_kernel, dim3(tiles, tiles), dim3(T::THREADS), 0, s, p, n);
  return hipGetLastError();
}

hipError_t launch_tsne_step(hipStream_t s, const TsneStepArgs& a) {
  using T = Tsne;
  const int per_wg = T::WAVES * a.rows;
  const dim3 grid((a.n + per_wg - 1) / per_wg), block(T::THREADS);
  const size_t lds = (size_t)a.n * 2 * sizeof(float);   // at most 64 KB
  const bool vec = a.n % 4 == 0, kl = a.kl_out != nullptr;
  if (vec && kl)
    hipLaunchKernelGGL((tsne_pairs_kernel<true, true>), grid, block, lds, s, a);
  else if (vec)
    hipLaunchKernelGGL((tsne_pairs_kernel<true, false>), grid, block, lds, s, a);
  else if (kl)
    hipLaunchKernelGGL((tsne_pairs_kernel<false, true>), grid, block, lds, s, a);
  else
    hipLaunchKernelGGL((tsne_pairs_kernel<false, false>), grid, block, lds, s, a);
  TSNE_LAUNCHED();
  hipLaunchKernelGGL(tsne_update_kernel, dim3((a.n + T::THREADS - 1) / T::THREADS), block, 0, s, a);
  return hipGetLastError();
}

// the pre-pass both PCA entry points that see x share with the distances
static hipError_t pca_center(hipStream_t s, const float* x, int n, int d, const TsneWork& w) {
  using T = Tsne;
  hipLaunchKernelGGL(tsne_means_kernel, dim3((d + T::MEAN_COLS - 1) / T::MEAN_COLS), dim3(T::THREADS), 0, s, x, n, d,
                     w.mean);
  TSNE_LAUNCHED();
  hipLaunchKernelGGL(tsne_center_kernel, dim3((n + T::WAVES - 1) / T::WAVES), dim3(T::THREADS), 0, s, x, n, d, w.mean,
                     w.xc, w.norm, w.rowmax);
  return hipGetLastError();
}

hipError_t launch_pca_scatter(hipStream_t s, const float* x, int n, int d, void* work, double* c) {
  using P = Pca;
  TsneWork tw;
  PcaWork w;
  pca_work_layout(n, d, work, &tw, &w);
  int rows, chunks;
  pca_chunks(n, d, &rows, &chunks);
  const int tiles = pca_tiles(d);
  const hipError_t e = pca_center(s, x, n, d, tw);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pca_scatter_kernel, dim3(tiles, tiles, chunks), dim3(P::THREADS), 0, s, tw.xc, tw.rowmax, n, d,
                     rows, w.part, w.kexp);
  TSNE_LAUNCHED();
  hipLaunchKernelGGL(pca_scatter_reduce_kernel, dim3(tiles, tiles), dim3(P::THREADS), 0, s, w.part, w.kexp, d, chunks,
                     c);
  return hipGetLastError();
}

hipError_t launch_pca_components(hipStream_t s, const double* c, int d, const double* trace, const double* q0, int k,
                                 int sweeps, void* work, float* components, double* eigvals, double* ratio,
                                 double* resid) {
  using P = Pca;
  PcaWork w;
  pca_work_layout(Tsne::MIN_N, d, work, nullptr, &w);   // q and z do not depend on n
  const int m = d < P::M ? d : P::M;
  const dim3 block(P::THREADS), mul((d + P::WAVES * P::MUL_ROWS - 1) / (P::WAVES * P::MUL_ROWS));
  hipLaunchKernelGGL(pca_orth_kernel, dim3(1), block, 0, s, q0, m, m, d, w.q);
  TSNE_LAUNCHED();
  for (int t = 0; t < sweeps; ++t) {
    hipLaunchKernelGGL(pca_multiply_kernel, mul, block, 0, s, c, w.q, d, w.z);
    TSNE_LAUNCHED();
    hipLaunchKernelGGL(pca_orth_kernel, dim3(1), block, 0, s, w.z, P::M, P::M, d, w.q);
    TSNE_LAUNCHED();
  }
  hipLaunchKernelGGL(pca_multiply_kernel, mul, block, 0, s, c, w.q, d, w.z);
  TSNE_LAUNCHED();
  hipLaunchKernelGGL(pca_ritz_kernel, dim3(1), block, 0, s,
                     PcaRitzArgs{w.q, w.z, c, trace, d, m, k, components, eigvals, ratio, resid});
  return hipGetLastError();
}

hipError_t launch_pca_project(hipStream_t s, const float* x, int n, int d, const float* components, int k,
                              const double* eigvals, void* work, float* scores, float* y0) {
  using P = Pca;
  TsneWork tw;
  tsne_work_layout(n, d, work, &tw);
  const hipError_t e = pca_center(s, x, n, d, tw);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pca_project_kernel, dim3((n + P::WAVES - 1) / P::WAVES), dim3(P::THREADS), 0, s, tw.xc, n, d,
                     components, k, eigvals, scores, reinterpret_cast<float2*>(y0));
  return hipGetLastError();
}

}  // namespace ba3c
