// ba3c_conv0d.hip — conv0's input-gradient kernel and its prep launch (ba3c_conv0d.h) in a
// translation unit of their own: like conv0's other kernels it keeps the MFMA accumulators in
// architectural VGPRs (its epilogue moves every one of them to LDS with VALU / DS instructions),
// and it is compiled without packed fp32 VALU operations (Makefile).  ba3c_capi.hip launches
// them through the two host functions.
#include <hip/hip_runtime.h>

#define BA3C_CONV0D_KERNELS 1
#include "ba3c_conv0d.h"

namespace ba3c {

hipError_t launch_conv0d_prep(hipStream_t s, const Conv0DPrepArgs& a) {
  hipLaunchKernelGGL(conv0d_prep_kernel, dim3(Conv0D::TBLK + a.batch * Conv0D::NCH), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_conv0d(int grid, hipStream_t s, const Conv0DArgs& a) {
  hipLaunchKernelGGL(conv0d_kernel, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace ba3c
