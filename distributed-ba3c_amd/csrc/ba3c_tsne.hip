// ba3c_tsne.hip — the t-SNE kernels (ba3c_tsne.h) in a translation unit of their own, compiled
// without packed fp32 VALU operations (Makefile).  ba3c_capi.hip launches them through the three
// host functions.
#include <hip/hip_runtime.h>

#define BA3C_TSNE_KERNELS 1
#include "ba3c_tsne.h"

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

}  // namespace ba3c
