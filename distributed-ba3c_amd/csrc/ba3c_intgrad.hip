// ba3c_intgrad.hip — the integrated-gradients kernels (ba3c_intgrad.h) in a translation unit of
// their own, compiled without packed fp32 VALU operations (Makefile).  ba3c_capi.hip launches them
// through the two host functions.
#include <hip/hip_runtime.h>

#define BA3C_INTGRAD_KERNELS 1
#include "ba3c_intgrad.h"

namespace ba3c {

hipError_t launch_ig_states(hipStream_t s, const IgStatesArgs& a, bool blur) {
  const dim3 grid(ig_grid(a.c)), block(IntGrad::THREADS);
  if (blur)
    hipLaunchKernelGGL(ig_states_kernel<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(ig_states_kernel<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ig_accumulate(hipStream_t s, const IgAccumulateArgs& a, bool blur) {
  const dim3 grid(ig_grid(a.c)), block(IntGrad::THREADS);
  if (blur)
    hipLaunchKernelGGL(ig_accumulate_kernel<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(ig_accumulate_kernel<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace ba3c
