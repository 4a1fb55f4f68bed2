// ba3c_conv0.hip — the conv0 forward / weight-gradient kernels (ba3c_split.h), and the launches
// that pair them with conv1's kernels, in a translation unit of their own, compiled with MFMA
// results in architectural VGPRs (-mllvm --amdgpu-mfma-vgpr-form, Makefile): their pool / un-pool epilogues read every accumulator
// with VALU instructions, which costs a v_accvgpr_read per value when the compiler places the
// accumulators in AGPRs.  ba3c_capi.hip launches them through these host functions.
#include <hip/hip_runtime.h>

#define BA3C_SHARED_KERNELS 0

#include "ba3c_launch.h"
#include "ba3c_split.h"
#include "ba3c_band6.h"
#include "ba3c_wgrad6.h"

namespace ba3c {

hipError_t launch_conv0s_fwd(dim3 grid, hipStream_t s, const Conv0SArgs& a) {
  hipLaunchKernelGGL(conv0s_fwd_kernel, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

// conv1's whole-channel weight gradient (wgrad6w_body, MFMA-bound) beside conv0's weight
// gradient (VALU-bound un-pooling) in one launch: blocks [0, g1) walk conv1's images, blocks
// [g1, g1 + g0) conv0's bands, one workgroup of each per CU.  Both read only the finished
// output gradients dP1 / dP0 and write their own partial slabs; each body runs exactly as in
// its plain kernel with (bx, gx) = (block - first block of its job, job grid).
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
wgrad01_pair_kernel(const Wg6Args a1, const Conv0WArgs a0, int g1, int g0) {
  constexpr int B1 = wgrad6w_lds_bytes<Conv1W6W>(), B0 = Conv0W<2>::ALLOC_U4 * 16;
  __shared__ uint4 lds[(B1 > B0 ? B1 : B0) / 16];
  __shared__ uint32_t red4[4];
  const int b = blockIdx.x;
  if (b < g1) {
    wgrad6w_body<Conv1W6W>(a1, b, g1, reinterpret_cast<char*>(lds), red4);
  } else {
    conv0s_wgrad_body<2>(a0, b - g1, g0, lds, red4);
  }
}

hipError_t launch_wgrad01_pair(hipStream_t s, const Wg6Args& a1, int g1, const Conv0WArgs& a0, int g0) {
  hipLaunchKernelGGL(wgrad01_pair_kernel, dim3(g1 + g0), dim3(256), 0, s, a1, a0, g1, g0);
  return hipGetLastError();
}

// conv0's forward (HBM-store and VALU bound) and conv1's forward ring walk (LDS-read bound) as
// one persistent launch: workgroup bx of gx takes its contiguous images [bx ipw, (bx + 1) ipw)
// through both layers, image by image — conv0(img), conv1(img), next image — and waits for no
// other workgroup: conv1 needs only the image's own p0 rows and its own maximum.  Each body
// runs as in its plain kernel over a range of one image (pointers offset to the image, batch
// = 1, (bx, gx) = (0, 1)), so the arithmetic per image is unchanged.  One launch boundary and
// one launch tail go away, and conv1 stages p0 rows its own CU wrote a moment earlier.
//
// Of the three orders measured the image-major one won; layer-major
// (conv0 for all of the workgroup's images, then conv1) and image-major with one workgroup of
// each CU running conv0 one image ahead were slower.  conv0 runs at wave priority 2, above
// conv1's main loop (1): where the two workgroups of a CU drift into different layers, the
// store-bound layer issues first.
//
// Visibility inside the workgroup: p0 / c0 are written through to L2 and this CU reads none of
// their lines before they are written, so a workgroup-scope release / acquire around the
// barrier is enough for the map; the image's maximum arrives in L2 by atomicMax and is read
// with an agent-scope load (band6r_body FRESH).  The barrier on the way back keeps conv0's
// restaging behind conv1's last LDS reads.
constexpr int FWD01_CONV0_PRIO = 2;

__device__ __forceinline__ void fwd01_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool TRAIN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
fwd01_kernel(const Conv0SArgs a0, const Band6Args a1) {
  using L1 = Conv1FLay;
  constexpr int B0 = conv0s_fwd_lds_bytes(), B1 = L1::LDS_BYTES;
  __shared__ uint4 lds4[(B0 > B1 ? B0 : B1) / 16];
  char* lds = reinterpret_cast<char*>(lds4);
  const int gx = gridDim.x, ipw = (a0.batch + gx - 1) / gx;
  const int img0 = min(a0.batch, (int)blockIdx.x * ipw), img1 = min(a0.batch, img0 + ipw);
  constexpr size_t X_IMG = (size_t)Conv0S::HS * Conv0S::WS * Conv0S::C;
  constexpr size_t P0_IMG = (size_t)(Conv0S::HO / 2) * (Conv0S::WO / 2) * Conv0S::COUT;
  constexpr size_t P1_IMG = (size_t)(L1::G::HO / 2) * (L1::G::WO / 2) * L1::G::COUT;
  for (int img = img0; img < img1; ++img) {
    {
      Conv0SArgs s = a0;
      s.x += img * X_IMG;
      s.out += img * P0_IMG;
      if (TRAIN) s.out_code += img * P0_IMG;
      s.amax_out += img;
      s.batch = 1;
      // (the weight fragments are reloaded per image, not kept in 64 registers through conv1)
      int z = 0;
      asm volatile("" : "+v"(z));
      s.wb += __builtin_amdgcn_readfirstlane(z);
      __builtin_amdgcn_s_setprio(FWD01_CONV0_PRIO);
      conv0s_fwd_body_t<TRAIN, true>(s, 0, 1, lds);
      __builtin_amdgcn_s_setprio(0);
    }
    fwd01_handoff();
    {
      Band6Args s = a1;
      s.src += img * P0_IMG;
      s.out += img * P1_IMG;
      if (TRAIN) s.out_code += img * P1_IMG;
      s.amax_in += img;
      s.amax_out += img;
      s.batch = 1;
      band6r_body<L1, false, true>(s, 0, 1, lds);
    }
    fwd01_handoff();
  }
}

hipError_t launch_fwd01(int grid, hipStream_t s, const Conv0SArgs& a0, const Band6Args& a1) {
  if (a0.out_code) hipLaunchKernelGGL(fwd01_kernel<true>, dim3(grid), dim3(256), 0, s, a0, a1);
  else hipLaunchKernelGGL(fwd01_kernel<false>, dim3(grid), dim3(256), 0, s, a0, a1);
  return hipGetLastError();
}

hipError_t launch_conv0s_wgrad(dim3 grid, hipStream_t s, const Conv0WArgs& a) {
  hipLaunchKernelGGL(conv0s_wgrad_kernel<2>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace ba3c
