// ba3c_perturb.hip — the perturbation-saliency kernels (ba3c_perturb.h) in a translation unit of
// their own, compiled without packed fp32 VALU operations (Makefile).  ba3c_capi.hip launches them
// through the two host functions.
#include <hip/hip_runtime.h>

#define BA3C_PERTURB_KERNELS 1
#include "ba3c_perturb.h"

namespace ba3c {

hipError_t launch_perturb_states(hipStream_t s, const PerturbStatesArgs& a, bool newest) {
  // the (state, centre row) workgroups that own a perturbed state of the chunk
  const int grid = (int)((a.first + a.count - 1) / Perturb::GRID) - a.wg0 + 1;
  if (newest)
    hipLaunchKernelGGL(perturb_states_kernel<true>, dim3(grid), dim3(Perturb::THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(perturb_states_kernel<false>, dim3(grid), dim3(Perturb::THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_perturb_scores(hipStream_t s, const PerturbScoresArgs& a, int n) {
  hipLaunchKernelGGL(perturb_scores_kernel, dim3(n), dim3(Perturb::THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace ba3c
