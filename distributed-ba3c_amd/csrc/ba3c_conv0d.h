// ba3c_conv0d.h — conv0's INPUT gradient (Conv2DBackpropInput of conv0): the derivative with
// respect to the float frames the network sees (state / 255), for saliency maps.  Training never
// needs it; ba3c_conv0_input_grad / ba3c_input_grads run it after the ordinary backward pass.
//
//   dX[b, y, x, c] = sum_{ky, kx in 0..4, o in 0..31} dY[b, y - ky, x - kx, o] W0[ky, kx, c, o]
//
// with dY the un-pooled 80 x 80 x 32 output gradient (dP0 routed to each window's argmax code,
// 0 elsewhere and outside the map), 0 <= y, x < 84, c < 4 (only conv0/W's real channels are read).
//
// The GEMM.  N = 4 channels would waste 3/4 of a 16-column MFMA, so the weights are expanded
// Toeplitz-wise: a GEMM row is a GROUP of four adjacent output pixels x = 4g + dx (21 groups per
// row) and a column is (dx, c), N = 16.  A group reads the 8 dY columns 4g - 4 + j, j = 0..7, so
// K = 5 ky x 8 j x 32 o = 1280 and
//   T[(ky, j, o), (dx, c)] = W0[ky, dx + 4 - j, c, o]   where 0 <= dx + 4 - j <= 4, else 0:
// 800 of the 1280 k of a column are real taps (62.5 % dense, against 25 % for C padded to 16).
// A k-step of 32 is one (ky, j) over all 32 o, and the 8 columns j are exactly the four POOLED
// columns 2g - 2 .. 2g + 1, so the A operand is read from a pooled, channel-last LDS image and
// un-pooled in registers: the fragment of (ky, j) is the pooled element's 8 values ANDed with the
// mask of `code == 2 (row parity) + (j & 1)`.
//
// Arithmetic: the fp32-class family of ba3c_split.h — fp16 hi/lo planes of dP0 2^kd (kd per
// IMAGE, from the image's own max) and of T 2^kw (per tensor), a1b1 + a1b2 + a2b1 on
// v_mfma_f32_16x16x32_f16 with fp32 accumulation, both scales removed exactly in the epilogue.
// An all-zero image has kd = 0, zero planes and an exactly zero result.
//
// Work split: a workgroup (4 waves) takes one image's band of RB = 4 output rows: 84 GEMM rows
// as (row r, m-tile of 16 groups) = 8 m-tiles.  The band needs dY rows 4 band - 4 .. 4 band + 3
// = 4 pooled rows, staged ONCE per workgroup as split planes + codes (35 KB).  K is split over
// the waves by pooled column: wave w owns j in {2w, 2w + 1} for every ky, so its 20 B fragments
// (5 ky x 2 j x 2 planes, 80 registers) stay in registers for the workgroup's life, every pooled
// element a wave reads feeds all four codes, and the four partial accumulators meet in LDS, summed
// in wave order (an image's result is a function of the image alone).  Persistent workgroups walk
// (image, band) pairs; the next band's dP0 / codes are loaded into registers before the current
// band's MFMAs.
//
// The per-image maxima and T come from conv0d_prep_kernel (one small launch): the kernel depends
// on no producer of dP0.
#pragma once
#include "ba3c_split.h"

namespace ba3c {

struct Conv0D {
  static constexpr int HS = 84, WS = 84, C = 4, CPAD = 16, COUT = 32, KT = 5;
  static constexpr int PH = 40, PW = 40, P_IMG = PH * PW * COUT;
  static constexpr int RB = 4, NBANDS = HS / RB, NG = WS / 4;          // 21 bands, 21 groups per row
  static constexpr int PROWS = (RB + KT - 1) / 2;                       // pooled rows per band (4)
  static constexpr int PCOLS = PW + 4;                                  // pooled columns -2 .. 41
  static constexpr int NJ = 8, KSTEPS = KT * NJ;                        // 40 k-steps of 32
  // plane pitch 80 B per pooled pixel: a 16-lane group's b128 reads (2 pixels = 160 B apart,
  // lane groups 16 B apart) cover all 8 16-byte bank groups evenly; codes 40 B per pixel
  static constexpr int PPITCH = 80, CPITCH = 40;
  static constexpr int PLANE_BYTES = PROWS * PCOLS * PPITCH, CODE_BYTES = PROWS * PCOLS * CPITCH;
  static constexpr int BAND_F = RB * WS * C;                            // 1344 outputs per band
  static constexpr int RED_OFF = 2 * PLANE_BYTES + CODE_BYTES;
  static constexpr int LDS_BYTES = RED_OFF + 4 * BAND_F * 4;            // 56704
  static constexpr int TB_U4 = 2 * KSTEPS * 64;                         // T: [plane][k-step][lane] x 16 B
  static constexpr int TBLK = KSTEPS * 64 / 256;                        // prep workgroups that build T
  static constexpr int NCH = 10, CH_F = P_IMG / NCH;                    // max partials per image
  static constexpr int NU = PROWS * PCOLS * (COUT / 4), NPT = (NU + 255) / 256;   // staging units of 4 o
  static_assert(HS % RB == 0 && RB % 2 == 0 && WS % 4 == 0 && NG <= 32, "band geometry");
  static_assert(PLANE_BYTES % 16 == 0 && RED_OFF % 16 == 0 && CH_F % 1024 == 0, "layout");
};

struct Conv0DPrepArgs {
  const float* w0;         // conv0/W [5,5,16,32]
  const float* dp;         // dP0 [B,40,40,32]
  const uint8_t* code;     // argmax codes of dP0
  uint4* tb;               // [Conv0D::TB_U4]
  int* wexp;               // [1]: kw
  uint32_t* amaxp;         // [B][NCH]: partial max |dY| bits
  int batch;
};

struct Conv0DArgs {
  const float* dp;
  const uint8_t* code;
  const uint4* tb;
  const int* wexp;
  const uint32_t* amaxp;
  float* dx;               // [B,84,84,4]
  float* map;              // [B,84,84] = sum_c |dX| (may be null)
  int batch;
};

// host launchers (ba3c_conv0d.hip); each returns hipGetLastError() of its launch
hipError_t launch_conv0d_prep(hipStream_t s, const Conv0DPrepArgs& a);
hipError_t launch_conv0d(int grid, hipStream_t s, const Conv0DArgs& a);

#ifdef BA3C_CONV0D_KERNELS   // the device code: ba3c_conv0d.hip only

// Workgroups [0, TBLK): T, split and in B-fragment order — thread (k-step ks = (ky, j), lane):
// column n = lane & 15 = (dx, c), k values o = 8 (lane >> 4) .. + 7.  Workgroups after them:
// (image, chunk of 4 pooled rows) -> the chunk's max |dP0| over live windows (code < 4).
__global__ void __launch_bounds__(256) conv0d_prep_kernel(const Conv0DPrepArgs a) {
  using G = Conv0D;
  __shared__ float red4[4];
  const int tid = threadIdx.x, lane = tid & 63;
  if ((int)blockIdx.x < G::TBLK) {
    const int kw = amax_exp(__float_as_uint(conv0_wmax_block(a.w0, red4)));
    if (blockIdx.x == 0 && tid == 0) a.wexp[0] = kw;
    const float sc = exp2i(kw);
    const int ks = ((int)blockIdx.x * 256 + tid) >> 6, ky = ks >> 3, j = ks & 7;
    const int n = lane & 15, q = lane >> 4, dx = n >> 2, c = n & 3, kx = dx + 4 - j;
    const bool tap = kx >= 0 && kx < G::KT;
    const float* wr = a.w0 + ((size_t)(ky * G::KT + (tap ? kx : 0)) * G::CPAD + c) * G::COUT + 8 * q;
    uint32_t part[2][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) split2(tap ? wr[e] * sc : 0.f, part[0][e], part[1][e]);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
      a.tb[(pl * G::KSTEPS + ks) * 64 + lane] =
          make_uint4(part[pl][0] | (part[pl][1] << 16), part[pl][2] | (part[pl][3] << 16),
                     part[pl][4] | (part[pl][5] << 16), part[pl][6] | (part[pl][7] << 16));
    return;
  }
  const int b = (int)blockIdx.x - G::TBLK;          // (image, chunk): contiguous CH_F elements
  const size_t base = (size_t)b * G::CH_F;
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < G::CH_F / 1024; ++i) {
    const size_t e = base + 4 * (size_t)(tid + 256 * i);
    const float4 v = *reinterpret_cast<const float4*>(a.dp + e);
    const uint32_t cw = *reinterpret_cast<const uint32_t*>(a.code + e);
    m = fmaxf(m, (cw & 0xFCu) ? 0.f : fabsf(v.x));
    m = fmaxf(m, (cw & 0xFC00u) ? 0.f : fabsf(v.y));
    m = fmaxf(m, (cw & 0xFC0000u) ? 0.f : fabsf(v.z));
    m = fmaxf(m, (cw & 0xFC000000u) ? 0.f : fabsf(v.w));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) red4[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) a.amaxp[b] = __float_as_uint(fmaxf(fmaxf(red4[0], red4[1]), fmaxf(red4[2], red4[3])));
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) conv0d_kernel(const Conv0DArgs a) {
  using G = Conv0D;
  using SP = SplitP<2>;
  __shared__ uint4 lds4[G::LDS_BYTES / 16];
  char* const hi = reinterpret_cast<char*>(lds4);
  char* const lo = hi + G::PLANE_BYTES;
  char* const cd = hi + 2 * G::PLANE_BYTES;
  float* const red = reinterpret_cast<float*>(hi + G::RED_OFF);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int nbands = a.batch * G::NBANDS;

  // ---- one band's 4 pooled rows x 44 pooled columns, a unit = 4 channels of a pooled pixel:
  // loaded into registers (branch-free: a unit outside the map re-reads the image's element 0
  // and is staged as zeros / dead codes), split and stored a band later ----
  float4 pv[G::NPT];
  uint32_t pc[G::NPT];
  auto load_band = [&](int band) {
    const int img = band / G::NBANDS, br = band - img * G::NBANDS;
    const float* dpi = a.dp + (size_t)img * G::P_IMG;
    const uint8_t* cdi = a.code + (size_t)img * G::P_IMG;
#pragma unroll
    for (int i = 0; i < G::NPT; ++i) {
      const int u = tid + 256 * i, o4 = u & 7, pix = u >> 3;
      const int prr = pix / G::PCOLS, col = pix - prr * G::PCOLS;
      const int p = 2 * br - 2 + prr, q = col - 2;
      const bool in = u < G::NU && p >= 0 && p < G::PH && q >= 0 && q < G::PW;
      const int e = in ? (p * G::PW + q) * G::COUT + 4 * o4 : 0;
      const float4 v = *reinterpret_cast<const float4*>(dpi + e);
      const uint32_t c = *reinterpret_cast<const uint32_t*>(cdi + e);
      pv[i] = in ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      pc[i] = in ? c : 0xFFFFFFFFu;
    }
  };
  auto store_band = [&](float sc) {
#pragma unroll
    for (int i = 0; i < G::NPT; ++i) {
      const int u = tid + 256 * i, o4 = u & 7, pix = u >> 3;
      if (u < G::NU) {
        uint32_t h01, l01, h23, l23;
        split2x2(pv[i].x * sc, pv[i].y * sc, h01, l01);
        split2x2(pv[i].z * sc, pv[i].w * sc, h23, l23);
        *reinterpret_cast<uint2*>(hi + pix * G::PPITCH + 8 * o4) = make_uint2(h01, h23);
        *reinterpret_cast<uint2*>(lo + pix * G::PPITCH + 8 * o4) = make_uint2(l01, l23);
        *reinterpret_cast<uint32_t*>(cd + pix * G::CPITCH + 4 * o4) = pc[i];
      }
    }
  };

  int band = blockIdx.x;
  if (band < nbands) load_band(band);

  // this wave's B fragments: T's k-steps (ky, j = 2 wave + sx), both planes
  u32x4 bf[2][G::KT][2];
#pragma unroll
  for (int pl = 0; pl < 2; ++pl)
#pragma unroll
    for (int ky = 0; ky < G::KT; ++ky)
#pragma unroll
      for (int sx = 0; sx < 2; ++sx) {
        const uint4 u = a.tb[(pl * G::KSTEPS + ky * G::NJ + 2 * wave + sx) * 64 + lane];
        bf[pl][ky][sx] = u32x4{u.x, u.y, u.z, u.w};
      }
  const int kw = a.wexp[0];

  for (; band < nbands; band += gridDim.x) {
    const int img = band / G::NBANDS, br = band - img * G::NBANDS;
    uint32_t am = 0u;                                  // the image's max |dY| (bits order like floats)
#pragma unroll
    for (int ch = 0; ch < G::NCH; ++ch) am = max(am, a.amaxp[img * G::NCH + ch]);
    const int kd = amax_exp(am);
    store_band(exp2i(kd));
    __syncthreads();                                   // (also: the previous band's epilogue is done)
    if (band + (int)gridDim.x < nbands) load_band(band + gridDim.x);

    f32x4 acc[G::RB][2];
#pragma unroll
    for (int r = 0; r < G::RB; ++r) acc[r][0] = acc[r][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int prr = 0; prr < G::PROWS; ++prr)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        // group g's pooled column 2g - 2 + wave (rows past group 20 repeat it and are discarded)
        const int pix = prr * G::PCOLS + 2 * min(16 * mt + li, G::NG - 1) + wave;
        const uint4 h = *reinterpret_cast<const uint4*>(hi + pix * G::PPITCH + 16 * lq);
        const uint4 l = *reinterpret_cast<const uint4*>(lo + pix * G::PPITCH + 16 * lq);
        const uint2 cw = *reinterpret_cast<const uint2*>(cd + pix * G::CPITCH + 8 * lq);
        // the 8 codes as 16-bit halves beside their values
        const uint32_t k0 = __builtin_amdgcn_perm(cw.x, cw.x, 0x0C010C00u), k1 = __builtin_amdgcn_perm(cw.x, cw.x, 0x0C030C02u);
        const uint32_t k2 = __builtin_amdgcn_perm(cw.y, cw.y, 0x0C010C00u), k3 = __builtin_amdgcn_perm(cw.y, cw.y, 0x0C030C02u);
#pragma unroll
        for (int sy = 0; sy < 2; ++sy) {
          const int ur = 2 * prr + sy;                 // un-pooled row of the band = r - ky + 4
#pragma unroll
          for (int sx = 0; sx < 2; ++sx) {
            const uint32_t x = (uint32_t)(2 * sy + sx) * 0x00010001u;
            const uint32_t m0 = c0w_mask16_eq0(k0 ^ x), m1 = c0w_mask16_eq0(k1 ^ x);
            const uint32_t m2 = c0w_mask16_eq0(k2 ^ x), m3 = c0w_mask16_eq0(k3 ^ x);
            const u32x4 ah = {h.x & m0, h.y & m1, h.z & m2, h.w & m3};
            const u32x4 al = {l.x & m0, l.y & m1, l.z & m2, l.w & m3};
#pragma unroll
            for (int r = 0; r < G::RB; ++r) {
              const int ky = r + G::KT - 1 - ur;
              if (ky >= 0 && ky < G::KT) {
                acc[r][mt] = SP::mfma(ah, bf[0][ky][sx], acc[r][mt]);
                acc[r][mt] = SP::mfma(ah, bf[1][ky][sx], acc[r][mt]);
                acc[r][mt] = SP::mfma(al, bf[0][ky][sx], acc[r][mt]);
              }
            }
          }
        }
      }

    // the wave's partial band [r][x][c]: lane holds groups 16 mt + 4 lq + e, column li = (dx, c)
    float* rw = red + wave * G::BAND_F;
#pragma unroll
    for (int r = 0; r < G::RB; ++r)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int g = 16 * mt + 4 * lq + e;
          if (g < G::NG) rw[(r * G::NG + g) * 16 + li] = acc[r][mt][e];
        }
    __syncthreads();
    // one 16-byte store per pixel: the four waves' partials in wave order, then both scales
    const float s1 = exp2i(-kd), s2 = exp2i(-kw);
    const size_t pix0 = ((size_t)img * G::HS + G::RB * br) * G::WS;
    for (int p = tid; p < G::RB * G::WS; p += 256) {
      const float4* r4 = reinterpret_cast<const float4*>(red) + p;
      const float4 w0 = r4[0], w1 = r4[G::BAND_F / 4], w2 = r4[2 * G::BAND_F / 4], w3 = r4[3 * G::BAND_F / 4];
      float4 o;
      o.x = (((w0.x + w1.x) + w2.x) + w3.x) * s1 * s2;
      o.y = (((w0.y + w1.y) + w2.y) + w3.y) * s1 * s2;
      o.z = (((w0.z + w1.z) + w2.z) + w3.z) * s1 * s2;
      o.w = (((w0.w + w1.w) + w2.w) + w3.w) * s1 * s2;
      reinterpret_cast<float4*>(a.dx)[pix0 + p] = o;
      if (a.map) a.map[pix0 + p] = (fabsf(o.x) + fabsf(o.y)) + (fabsf(o.z) + fabsf(o.w));
    }
  }
}

#endif  // BA3C_CONV0D_KERNELS

}  // namespace ba3c
