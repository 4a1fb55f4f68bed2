// ba3c_capi.hip — C ABI (include/ba3c.h) and step orchestration of libba3c.so.
//
// One call of ba3c_train_grads runs, on the caller's stream, the whole tower of
// train.py:164-327 plus its TF autodiff (train/multigpu.py:85-86):
//   conv0..conv3 forward (ReLU, max-pool + argmax codes fused), fc1, heads+softmax+loss,
//   then backward: head/fc1/conv weight gradients (split-K MFMA + deterministic reduce)
//   and input gradients (MFMA dgrad with MaxPoolGrad/ReluGrad fused into the loaders).
// No device allocation and no synchronisation happen inside any entry point.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>   // types only: the functions are resolved from the loaded RCCL (dlsym)

#include <cmath>
#include <cstdio>
#include <cstring>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ba3c.h"
#include "ba3c_band6.h"
#include "ba3c_boxing.h"
#include "ba3c_breakout.h"
#include "ba3c_conv.h"
#include "ba3c_conv3.h"
#include "ba3c_duel.h"
#include "ba3c_envview.h"
#include "ba3c_episodes.h"
#include "ba3c_gemm6.h"
#include "ba3c_launch.h"
#include "ba3c_multi.h"
#include "ba3c_plan.h"
#include "ba3c_problems.h"
#include "ba3c_rollout.h"
#include "ba3c_small.h"
#include "ba3c_split.h"
#include "ba3c_wgrad6.h"

using namespace ba3c;

// The TfDictOp scalar reduction (scalars_block) as one workgroup of a multi-job launch: at
// large batches it rides on conv3's input-gradient launch instead of its own dependent
// launch after the heads (nothing in the step reads the scalars).
struct ScalarsJob {
  struct Args {
    const float* terms;
    int B;
    float beta;
    const unsigned long long* relu;
    double* out;
  };
  static constexpr int LDS = 0;
  __device__ static void run(const Args& a, int, int, int, int, char*, uint32_t*) {
    scalars_block(a.terms, a.B, a.beta, a.relu, a.out);
  }
};

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return fail(BA3C_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
  } while (0)

#ifndef BA3C_WGRAD_TARGET
#define BA3C_WGRAD_TARGET 1024   // split-K workgroups a GEMM-engine weight gradient aims for (A/B)
#endif
constexpr int kWgradTargetBlocks = BA3C_WGRAD_TARGET;
constexpr int kMaxBatch = 16384;

inline int64_t align64(int64_t x) { return (x + 63) & ~int64_t(63); }
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

struct TensorDesc {
  std::string name;
  int64_t offset;
  int64_t numel;
  int32_t shape[4];
  int32_t ndim;
};

constexpr int CHAIN_SITES = 1;   // chained launch sites (launch_chain)

struct ba3c_handle {
  ba3c_config cfg;
  std::vector<TensorDesc> tensors;
  int64_t flat;
  int idx_conv[4];
  int idx_fc1;        // first fc1 tensor
  int idx_piW, idx_pib, idx_vW, idx_vb;
  int per, wstride;
  TensorTable table;
  Switches sw;        // the launch-structure switches (ba3c_plan.h), fixed at create; device_errors
                      // may clear sw.chain
  // !sw.generic: split-MFMA kernels (band convolutions, conv0, weight gradients, the bf16x6 GEMM
  // engine); BA3C_GENERIC=1: every convolution and GEMM on the fp32-MFMA GEMM engine instead
  bool band = true;
  uint32_t merged[BA3C_NUM_KERNELS] = {};   // ba3c_kernel_merged, per training pass
  // the large-batch scalar reduction when run_heads deferred it (sw.scalars_ride) onto conv3's
  // input-gradient launch (also across the phase-1/phase-2 split of the N>1 step); when no
  // launch takes it, finish() launches it at the end of phase 0 or phase 2
  bool pend_scalars = false;
  ScalarsJob::Args scalars_args{};
  int cus = 256;      // compute units of the device (persistent grids)
  bool g6 = true;     // implicit-GEMM launches (conv3, fc1, heads; C=12 conv0) on bf16x6 split
                      // MFMA (ba3c_gemm6.h; off with BA3C_GENERIC=1: fp32 MFMA)
  // clip_update_kernel's tagged partials (nchunks words) + error flag: device, zeroed at create;
  // clip_range_kernel's (a generation space of their own) follow them
  unsigned long long* utag = nullptr;
  unsigned long long* ctag = nullptr;
  // chained multi-job launches (ba3c_multi.h: an in-launch dependency instead of a kernel
  // boundary): CHAIN_SITES x 4 words + an error word after the tags (null: no device memory,
  // unchained launches)
  unsigned* chain = nullptr;
  // recorded on the pass's stream after conv3's input- and weight-gradient launches of every
  // phase-2 pass (ba3c_set_phase2_event; null: none)
  hipEvent_t ev_mid = nullptr;
  hipStream_t side = nullptr;
  hipEvent_t ev_fork[4] = {}, ev_join = nullptr;
  // weight-gradient reductions of the backward pass (BackwardPass), launched together at its end
  ReduceJobs rjobs{};
  // RCCL communicator of the C-ABI gradient exchange (ba3c_comm_init; null: none)
  ncclComm_t comm = nullptr;
  int comm_ranks = 0;
  // timing probe
  int probe_kernel = -1;
  std::vector<hipEvent_t> ev_begin, ev_end;
  int probe_used = 0;
  int probe_every = 1;        // ba3c_probe_every: bracket one launch in `probe_every`
  unsigned probe_seen = 0;    // launches of probe_kernel since ba3c_probe_enable
  int probe_launches = 0;
  double probe_ms = 0.0;
};

namespace {

// ---- workspace layout -----------------------------------------------------------------
// band-conv geometries (ba3c_conv.h): forward conv1/conv2 with pooling, and the input
// gradients of conv1/conv2 as VALID convs over the 4-padded un-pooled output gradient
// (conv1's forward geometry GConv1F and its layout Conv1FLay: ba3c_band6.h)
using GConv2F = BandGeom<18, 18, 32, 64, 5, 5, 14, true, 0, 4>;
using GConv1D = BandGeom<44, 44, 32, 32, 5, 5, 4, false, 1, 8, 4, 4, 18, 18, 36, 36>;
using GConv2D = BandGeom<22, 22, 64, 32, 5, 5, 6, false, 1, 8, 4, 4, 7, 7, 14, 14>;
// split-family variants (ba3c_band6.h): pixel pitch / extra row bytes from a bank-conflict
// search (scripts/lds_bank_search.py), per family (3 bf16 planes or 2 fp16 planes per pixel)
//  C2D: conv2 input gradient, the whole 18x18 map per workgroup in two 32-channel phases
//       (r01r: 0.44 ms at 6-row bands -> 0.31 ms: no halo re-staging, 11 m-blocks per wave
//       hide the weight-fragment latency; 6 and 9-row bands and 8-row conv1 / 12-row
//       conv1-fwd bands measured slower)
//  C2FS / C2DS: small batches (B <= SMALL_B, e.g. configs[1]'s B=32): conv2 forward / input
//       gradient in 2- / 3-row bands, so the launch has 7x / 6x the workgroups of the
//       whole-map kernels — at B=32 those are 32 workgroups on 256 CUs, one latency-bound
//       wave of work.  Every output's K order (phase, tap, channel chunk, product) is the same
//       in both geometries, so results are bit-identical across the switch.
using GConv2DW = BandGeom<22, 22, 64, 32, 5, 5, 18, false, 1, 8, 4, 4, 7, 7, 14, 14>;
using GConv2FS = BandGeom<18, 18, 32, 64, 5, 5, 2, true, 0, 4>;
using GConv2DS = BandGeom<22, 22, 64, 32, 5, 5, 3, false, 1, 8, 4, 4, 7, 7, 14, 14>;
// split-kernel layouts (scaled fp16 hi/lo planes)
struct Lay {
  using C1F = Conv1FLay;
  using C2F = Band6<GConv2F, 160, 64, 7, 0, 2>;   // (double-buffered: 256 VGPRs, neutral, r04)
  using C1D = Band6<GConv1D, 160, 0, 5, 0, 2, true, true>;   // 4x4 tiles: RP = 128 mod 256 B
  using C2D = Band6<GConv2DW, 160, 128, 11, 32, 2, false, false, true>;   // padding skip, no A double buffer
  using C2FS = Band6<GConv2FS, 160, 64, 2, 0, 2, true>;
  using C2DS = Band6<GConv2DS, 160, 128, 2, 32, 2, true>;
  using W1 = Wg6Geom<40, 40, 32, 32, 4, 16, 32, 96, 160, 2>;
  using W2 = Wg6Geom<18, 18, 32, 64, 14, 16, 32, 96, 160, 2>;
  using W1W = Wg6WGeom<40, 40, 32, 32, 4, 160, 160>;   // conv1, B >= W6W_MIN_B (66.2 KB LDS)
};
// the layout numbers of the slab-count functions (ba3c_plan.h)
static_assert(Lay::W1::NBANDS == W1_NBANDS && Conv0S::NBANDS == C0F_NBANDS && Conv0W<2>::NBANDS == C0W_NBANDS,
              "ba3c_plan.h: bands per image");
constexpr int WT_C1F = 0, WT_C2F = WT_C1F + 800 * 32, WT_C3F = WT_C2F + 800 * 64,
              WT_C1D = WT_C3F + 576 * 64, WT_C2D = WT_C1D + 800 * 32, WT_C3D = WT_C2D + 1600 * 32,
              WT_C0F = WT_C3D + 576 * 64,
              WT_C0S = WT_C0F + 32 * Conv0Geom::KDIM,            // uint4 [Conv0S::WB_U4]
              WT_TOTAL = WT_C0S + 4 * Conv0S::WB_U4;
static_assert(WT_C0S % 4 == 0, "conv0's fragments are read as uint4: a 16-byte aligned offset");

// max-|x| slot arrays (ba3c_split.h, fp16 family)
enum { AM_P0 = 0, AM_P1 = 1, AM_DP0 = 2, AM_DP1 = 3, AM_DP2 = 4, AM_P2 = 5, AM_DY3 = 6, AMAX_N = 7 };
struct Workspace {
  float *p0, *p1, *p2, *a3, *h, *fcpart, *dh, *dy3, *dp2, *dp1, *dp0, *dzv, *terms, *part0, *sumsq, *wt;
  // split-K / per-workgroup partial slabs of each weight gradient (reduced in one launch at the
  // end of the backward pass, so each layer needs a region of its own)
  float *part_h, *part_f, *part_3, *part_2, *part_1;
  uint16_t* wt6;   // [3][N][K] bf16 splits of the four band-conv weight copies
  uint8_t *c0, *c1, *c2;
  unsigned long long* relu;
  uint32_t* amax;  // [AMAX_N][1 + max_batch]: max |x| of split operands (global, per image)
  int* wexp;       // [8]: weight scale exponents (wprep jobs WJ_*, conv0 = WX_CONV0)
  size_t bytes;
  uint32_t* am(int t, const ba3c_handle* h) const { return amax + (size_t)t * (1 + h->cfg.max_batch); }
};
// weight-preparation jobs (forward copies first: inference prepares only those) and the
// index of each one's scale exponent in Workspace::wexp
enum { WJ_C1F = 0, WJ_C2F = 1, WJ_C3F = 2, WJ_C1D = 3, WJ_C2D = 4, WJ_C3D = 5, WJ_N = 6, WJ_FWD = 3,
       WX_CONV0 = 7 };

struct WgradPlan {
  int M, N, K, S, kchunk, mt, nt;
};

WgradPlan plan_wgrad(int M, int N, int K, int BM, int BN, int target = kWgradTargetBlocks) {
  WgradPlan w;
  w.M = M;
  w.N = N;
  w.K = K;
  w.mt = (M + BM - 1) / BM;
  w.nt = (N + BN - 1) / BN;
  const int ktiles = (K + GEMM_BK - 1) / GEMM_BK;
  int S = (target + w.mt * w.nt - 1) / (w.mt * w.nt);
  S = std::max(1, std::min(S, (ktiles + 3) / 4));   // >= 4 k-tiles per split
  const int tiles_per = (ktiles + S - 1) / S;
  w.kchunk = tiles_per * GEMM_BK;
  w.S = (K + w.kchunk - 1) / w.kchunk;
  return w;
}

// fc1's backward at large batches (the multi-job launch): 128 x 128 tiles for the input and
// weight gradients instead of 64 x 64 / 128 x 64.  The engine splits every staged fp32 value
// into three bf16 planes (ba3c_gemm6.h), and at the small tiles that staging issued 10.8 VALU
// instructions per MFMA (PMC): four times the MFMAs per staged value.  The weight gradient
// takes fewer, longer K slabs (BA3C_FC1W_TARGET workgroups: 5 slabs at B = 2048, F = 512).
// Measured (r06v, r06w): the launch 0.0600 -> 0.0586 ms and the all-layer reduction 29.2 ->
// 28.0 us (half the fc1 slabs); not the 3x the VALU count suggested — the two workgroups per CU
// that 60 KB of LDS allows leave each k-tile's staging exposed, and 3- / 4-deep load rings
// (BA3C_FCD_DEPTH) made it 0.079 / 0.080 ms.
#ifndef BA3C_FC1W_TARGET
#define BA3C_FC1W_TARGET 256
#endif
WgradPlan fc1w_plan(int F, int B, bool legacy, bool bigtile) {
  return bigtile ? plan_wgrad(1600 + (legacy ? 1 : 0), F, B, 128, 128, BA3C_FC1W_TARGET)
                 : plan_wgrad(1600 + (legacy ? 1 : 0), F, B, 128, 64);
}

// geometry constants (train.py:92, :177-212)
constexpr int P0 = 40 * 40 * 32, P1 = 18 * 18 * 32, P2 = 7 * 7 * 64, A3 = 1600;
// FC1 fwd split-K: 5 fixed chunks of 10 k-tiles (batch-independent rounding), each the sum
// of its even and its odd k-tiles (gemm6_body PAR: two groups at B <= 64, one
// group with two accumulator sets above; the same association, so every row rounds the same
// at any batch).
// r02: 416 (4 chunks of 13 k-tiles) left B=32 with 8 workgroups walking 13 dependent k-tiles
// (17.6 us).  r06aa / r06ab: 5 chunks instead of 10 (half the partial sums written by fc1 and
// read by the heads kernel) took the B=2048 step 1.713 -> 1.685 and 1.685 -> 1.665 ms, but
// B=32 0.1565 -> 0.1612 ms with 10 k-tiles per workgroup in series: hence the two groups.
#ifndef BA3C_FC_KCHUNK
#define BA3C_FC_KCHUNK 320
#endif
constexpr int FC_KCHUNK = BA3C_FC_KCHUNK, FC_SPLIT = (A3 + FC_KCHUNK - 1) / FC_KCHUNK;
static_assert(FC_SPLIT <= FC_SPLIT_MAX, "heads kernel finishes at most FC_SPLIT_MAX chunks");
static_assert(FC_KCHUNK % GEMM_BK == 0, "k-chunk of whole k-tiles");

// conv0's weight gradient runs on the main stream while the other weight gradients run on
// the side stream, so its split-K partials get a region of their own
size_t max_partials0(const ba3c_handle* h, int B) {
  size_t mx = 0;
  const WgradPlan w = plan_wgrad(25 * h->cfg.channels, 32, B * 6400, 128, 32);
  mx = std::max(mx, (size_t)w.S * w.M * w.N);
  mx = std::max(mx, (size_t)WG_P0S * Conv0W<2>::M * 32);
  return mx;
}

// partial-slab floats of each layer's weight gradient (every kernel variant of that layer)
struct PartialSizes {
  size_t heads, fc1, conv3, conv2, conv1;
};
PartialSizes partial_sizes(const ba3c_handle* h, int B) {
  const int F = h->cfg.fc_neurons;
  auto sz = [](const WgradPlan& w) { return (size_t)w.S * w.M * w.N; };
  PartialSizes p;
  p.heads = sz(plan_wgrad(F + 1, h->cfg.num_actions + 1, B, 128, 32));
  const bool legacy = !h->cfg.replace_with_conv;
  p.fc1 = std::max(sz(fc1w_plan(F, B, legacy, false)), sz(fc1w_plan(F, B, legacy, true)));
  p.conv3 = std::max(sz(plan_wgrad(576, 64, B * 25, 128, 64)), (size_t)C3W_P * 576 * 64);
  p.conv2 = std::max(sz(plan_wgrad(800, 64, B * 196, 128, 64)), (size_t)W6_P2 * Lay::W2::M * Lay::W2::COUT);
  p.conv1 = std::max(sz(plan_wgrad(800, 32, B * 1296, 128, 32)), (size_t)WG_P1 * Lay::W1::M * Lay::W1::COUT);
  return p;
}

Workspace carve(const ba3c_handle* h, void* base, int B, bool train) {
  Workspace w;
  std::memset(&w, 0, sizeof(w));
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) -> char* {
    char* r = reinterpret_cast<char*>(reinterpret_cast<uintptr_t>(p) + off);  // p may be 0: offsets
    off += align256(bytes);
    return r;
  };
  const size_t Bz = (size_t)B;
  const int F = h->cfg.fc_neurons;
  // The clip / optimizer per-chunk sum-of-squares partials come FIRST, at a batch-independent
  // offset: ba3c_clip_grads / ba3c_apply_update receive only the workspace base.
  w.sumsq = (float*)take((size_t)h->table.nchunks * 4);
  w.amax = (uint32_t*)take((size_t)AMAX_N * (1 + h->cfg.max_batch) * 4);
  w.wexp = (int*)take(8 * 4);
  w.p0 = (float*)take(Bz * P0 * 4);
  w.p1 = (float*)take(Bz * P1 * 4);
  w.p2 = (float*)take(Bz * P2 * 4);
  w.a3 = (float*)take(Bz * A3 * 4);
  w.h = (float*)take(Bz * F * 4);
  w.fcpart = (float*)take((size_t)FC_SPLIT * Bz * F * 4);
  w.relu = (unsigned long long*)take(RELU_WORDS * 8);
  w.wt = (float*)take((size_t)WT_TOTAL * 4);
  w.wt6 = (uint16_t*)take((size_t)3 * WT_C0F * 2);
  if (train) {
    w.c0 = (uint8_t*)take(Bz * P0);
    w.c1 = (uint8_t*)take(Bz * P1);
    w.c2 = (uint8_t*)take(Bz * P2);
    w.dh = (float*)take(Bz * F * 4);
    w.dy3 = (float*)take(Bz * A3 * 4);
    w.dp2 = (float*)take(Bz * P2 * 4);
    w.dp1 = (float*)take(Bz * P1 * 4);
    w.dp0 = (float*)take(Bz * P0 * 4);
    w.dzv = (float*)take(Bz * MAXA * 4);
    w.terms = (float*)take(Bz * NTERMS * 4);
    const PartialSizes ps = partial_sizes(h, B);
    w.part_h = (float*)take(ps.heads * 4);
    w.part_f = (float*)take(ps.fc1 * 4);
    w.part_3 = (float*)take(ps.conv3 * 4);
    w.part_2 = (float*)take(ps.conv2 * 4);
    w.part_1 = (float*)take(ps.conv1 * 4);
    w.part0 = (float*)take(max_partials0(h, B) * 4);
  }
  w.bytes = off;
  return w;
}

// ---- launch helpers -------------------------------------------------------------------
struct ProbeScope {
  ba3c_handle* h;
  hipStream_t s;
  bool on;
  ProbeScope(ba3c_handle* h_, hipStream_t s_, int kid) : h(h_), s(s_), on(false) {
    if (h->probe_kernel == kid && h->probe_seen++ % (unsigned)h->probe_every == 0 &&
        h->probe_used < (int)h->ev_begin.size()) {
      on = true;
      (void)hipEventRecord(h->ev_begin[h->probe_used], s);
    }
  }
  ~ProbeScope() {
    if (on) {
      (void)hipEventRecord(h->ev_end[h->probe_used], s);
      h->probe_used++;
    }
  }
};

template <int BM, int BN, int WGM, int WGN, class P, int KS = 1>
int launch_gemm(ba3c_handle* h, hipStream_t s, int kid, const P& p, int splits) {
  if (p.M <= 0 || p.N <= 0) return BA3C_OK;
  dim3 grid((p.M + BM - 1) / BM, (p.N + BN - 1) / BN, splits);
  {
    ProbeScope ps(h, s, kid);
    // fewer workgroups than CUs: each walks its K latency-bound, so keep 4 k-tiles in flight
    const bool deep = (int)(grid.x * grid.y * grid.z) < h->cus;
    if (KS == 2 && h->g6 && deep)
      hipLaunchKernelGGL((gemm6_kernel<BM, BN, WGM, WGN, P, 4, KS>), grid, dim3(GEMM_THREADS * KS), 0, s, p);
    else if (KS == 2 && h->g6)
      hipLaunchKernelGGL((gemm6_kernel<BM, BN, WGM, WGN, P, 2, KS>), grid, dim3(GEMM_THREADS * KS), 0, s, p);
    else if (h->g6 && deep)
      hipLaunchKernelGGL((gemm6_kernel<BM, BN, WGM, WGN, P, 4>), grid, dim3(GEMM_THREADS), 0, s, p);
    else if (h->g6)
      hipLaunchKernelGGL((gemm6_kernel<BM, BN, WGM, WGN, P>), grid, dim3(GEMM_THREADS), 0, s, p);
    else
      hipLaunchKernelGGL((gemm_kernel<BM, BN, WGM, WGN, P>), grid, dim3(GEMM_THREADS), 0, s, p);
  }
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

// Every weight-gradient reduction of a backward pass is a job of one launch at its end
// (launch_reduce_all): add one.
int add_reduce(ba3c_handle* h, const float* part, int S, const ReduceMap& mp) {
  ReduceJobs& j = h->rjobs;
  if (j.n >= MAX_RJOBS) return fail(BA3C_ERR_INVALID, "too many deferred reductions");
  j.part[j.n] = part;
  j.S[j.n] = S;
  j.mp[j.n] = mp;
  const int no = mp.kind == 0 ? (mp.M / mp.cin) * mp.cinpad * mp.N : mp.M * mp.N;
  j.vec[j.n] = reduce_vec_ok(mp) ? 1 : 0;
  j.blk0[j.n + 1] = j.blk0[j.n] + (no + (j.vec[j.n] ? 255 : 63)) / (j.vec[j.n] ? 256 : 64);
  ++j.n;
  return BA3C_OK;
}

int launch_reduce_all(ba3c_handle* h, hipStream_t s, const ReduceJobs& jobs) {
  {
    ProbeScope ps(h, s, BA3C_K_WGRAD_REDUCE);
    hipLaunchKernelGGL(wgrad_reduce_all_kernel, dim3(jobs.blk0[jobs.n]), dim3(64 * RED_G), 0, s, jobs);
  }
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

#define CHECK(x)            \
  do {                      \
    int _r = (x);           \
    if (_r != BA3C_OK) return _r; \
  } while (0)

// Split operands of a band-conv launch (fp16 family): the max slots of the staged map, the
// weight job whose scale exponent applies, and the slots that receive max |out| (-1: none).
struct SplitIO {
  int amax_in, wjob, amax_out;
};

template <class L>
Band6Args band6_args(ba3c_handle* h, const BandArgs& a, const Workspace& w, int wt_off, SplitIO io) {
  return Band6Args{a.src, a.code, w.wt6 + L::NS * (size_t)wt_off, a.out, a.out_code, a.relu_count, a.batch,
                   w.am(io.amax_in, h), w.wexp + io.wjob, io.amax_out >= 0 ? w.am(io.amax_out, h) : nullptr};
}

// the jobs' grids and block ranges in a multi-job launch
MultiGrid multi_grid(dim3 g0, dim3 g1, dim3 g2) {
  MultiGrid g;
  const dim3 gs[3] = {g0, g1, g2};
  int end = 0;
  for (int j = 0; j < 3; ++j) {
    g.gx[j] = (int)gs[j].x;
    g.gy[j] = (int)gs[j].y;
    end += (int)(gs[j].x * gs[j].y * gs[j].z);
    g.end[j] = end;
  }
  return g;
}

// One launch of up to three independent jobs (ba3c_multi.h); W2: the two-workgroups-per-CU
// register budget of the band / weight-gradient kernels; T512: 512-thread jobs.
template <bool W2, class J0, class J1, class J2 = NoJob, bool T512 = false>
int launch_multi(hipStream_t s, const typename J0::Args& a0, dim3 g0, const typename J1::Args& a1, dim3 g1,
                 const typename J2::Args& a2 = typename J2::Args{}, dim3 g2 = dim3(0, 1, 1),
                 ba3c_handle* h = nullptr, int kid = -1) {
  const MultiGrid g = multi_grid(g0, g1, g2);
  const int end = g.end[2];
  if (end == 0) return BA3C_OK;
  // the timing probe brackets the whole launch under job 0's kernel id
  std::optional<ProbeScope> probe;
  if (h && kid >= 0) probe.emplace(h, s, kid);
  if constexpr (T512)
    hipLaunchKernelGGL((multi_kernel512<J0, J1, J2>), dim3(end), dim3(512), 0, s, a0, a1, a2, g);
  else if constexpr (W2)
    hipLaunchKernelGGL((multi_kernel_w2<J0, J1, J2>), dim3(end), dim3(256), 0, s, a0, a1, a2, g);
  else
    hipLaunchKernelGGL((multi_kernel<J0, J1, J2>), dim3(end), dim3(256), 0, s, a0, a1, a2, g);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

// A chained multi-job launch (ba3c_multi.h): jobs [0, nsig) signal, the jobs in `wmask` wait
// for them (those in `late` inside their body); `site` picks the launch site's counter words.
// Callers check chain_ok() first.
constexpr int CHAIN_PREP_CONV0 = 0;
bool chain_ok(const ba3c_handle* h) { return h->sw.chain && h->chain != nullptr; }

template <bool W2, class J0, class J1, class J2 = NoJob>
int launch_chain(hipStream_t s, int site, int nsig, int wmask, int late, const typename J0::Args& a0, dim3 g0,
                 const typename J1::Args& a1, dim3 g1, const typename J2::Args& a2 = typename J2::Args{},
                 dim3 g2 = dim3(0, 1, 1), ba3c_handle* h = nullptr, int kid = -1) {
  const MultiGrid g = multi_grid(g0, g1, g2);
  const int end = g.end[2];
  if (end == 0) return BA3C_OK;
  int nwait = 0;
  for (int j = 0; j < 3; ++j)
    if ((wmask >> j) & 1) nwait += g.end[j] - (j ? g.end[j - 1] : 0);
  const ChainArgs c{h->chain + 4 * site, h->chain + 4 * CHAIN_SITES, nsig, wmask, nwait, late};
  std::optional<ProbeScope> probe;
  if (kid >= 0) probe.emplace(h, s, kid);
  if constexpr (W2)
    hipLaunchKernelGGL((multi_chain_kernel_w2<J0, J1, J2>), dim3(end), dim3(256), 0, s, a0, a1, a2, g, c);
  else
    hipLaunchKernelGGL((multi_chain_kernel<J0, J1, J2>), dim3(end), dim3(256), 0, s, a0, a1, a2, g, c);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

// band conv on split MFMA; `ring` (LaunchPlan::ring_fwd / ring_dgrad): a multi-band layout runs
// as the ring-walk persistent kernel (whole images per workgroup)
template <class L>
int launch_band6(ba3c_handle* h, hipStream_t s, int kid, const BandArgs& a, const Workspace& w,
                 int wt_off, SplitIO io, bool ring = false) {
  const Band6Args b = band6_args<L>(h, a, w, wt_off, io);
  const int nbands = a.batch * L::G::NBANDS;
  {
    ProbeScope ps(h, s, kid);
    if constexpr (L::NPH == 1 && L::G::NBANDS > 1 && L::G::SROWS > L::G::RB) {
      if (ring) {
        // (the forward keeps its double-buffered A fragments and no row prefetch: the
        // no-DBUF layout with the prefetch measured 0.36 -> 0.41 ms, r02ai)
        hipLaunchKernelGGL(conv_band6r_kernel<L>, dim3(2 * h->cus), dim3(256), 0, s, b);
        HIP_TRY(hipGetLastError());
        return BA3C_OK;
      }
    }
    hipLaunchKernelGGL(conv_band6_kernel<L>, dim3(nbands), dim3(256), 0, s, b);
  }
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

// split weight-gradient kernel + deterministic reduction into the flat HWIO grads
template <class G>
dim3 wgrad6_grid(int pmax, int batch) {
  return dim3(std::min(pmax, batch * G::NBANDS), G::NCG * G::NOG);
}
template <class G>
int reduce_wgrad6(ba3c_handle* h, const Wg6Args& a, int P, float* dst);
template <class G>
int launch_wgrad6(ba3c_handle* h, hipStream_t s, int kid, const Wg6Args& a, int pmax, float* dst) {
  const dim3 grid = wgrad6_grid<G>(pmax, a.batch);
  {
    ProbeScope ps(h, s, kid);
    hipLaunchKernelGGL(wgrad6_kernel<G>, grid, dim3(256), 0, s, a);
  }
  HIP_TRY(hipGetLastError());
  return reduce_wgrad6<G>(h, a, (int)grid.x, dst);
}
template <class G>
int reduce_wgrad6(ba3c_handle* h, const Wg6Args& a, int P, float* dst) {
  ReduceMap mp{};
  mp.kind = 0;
  mp.M = G::M;
  mp.N = G::COUT;
  mp.cin = G::CIN;
  mp.cinpad = G::CIN;
  mp.dst = dst;
  return add_reduce(h, a.part, P, mp);
}

// Split-path weight preparation arguments (wprep6_kernel): every job, the conv0 fragments and
// the zeroing of the ReLU counters / max slots.
WPrep6Args wprep6_args(ba3c_handle* h, const float* prm, const Workspace& w, bool train) {
  const float* W1 = prm + h->tensors[h->idx_conv[1]].offset;
  const float* W2 = prm + h->tensors[h->idx_conv[2]].offset;
  const float* W3 = prm + h->tensors[h->idx_conv[3]].offset;
  WPrep6Args pa{};
  WPrepArgs& a = pa.jobs;
  a.job[WJ_C1F] = WPrepJob{W1, w.wt + WT_C1F, 5, 5, 32, 32, 0, 800 * 32};
  a.job[WJ_C2F] = WPrepJob{W2, w.wt + WT_C2F, 5, 5, 32, 64, 0, 800 * 64};
  a.job[WJ_C3F] = WPrepJob{W3, w.wt + WT_C3F, 3, 3, 64, 64, 0, 576 * 64};
  a.job[WJ_C1D] = WPrepJob{W1, w.wt + WT_C1D, 5, 5, 32, 32, 1, 800 * 32};
  a.job[WJ_C2D] = WPrepJob{W2, w.wt + WT_C2D, 5, 5, 32, 64, 1, 1600 * 32};
  a.job[WJ_C3D] = WPrepJob{W3, w.wt + WT_C3D, 3, 3, 64, 64, 1, 576 * 64};
  a.njobs = train ? WJ_N : WJ_FWD;
  pa.wt6 = w.wt6;
  const int offs[WJ_N] = {WT_C1F, WT_C2F, WT_C3F, WT_C1D, WT_C2D, WT_C3D};
  for (int j = 0; j < WJ_N; ++j) pa.off[j] = offs[j];
  pa.w0 = prm + h->tensors[h->idx_conv[0]].offset;
  pa.wb0 = reinterpret_cast<uint4*>(w.wt + WT_C0S);
  pa.relu = train ? w.relu : nullptr;
  pa.amax = w.amax;
  pa.n_amax = AMAX_N * (1 + h->cfg.max_batch);
  pa.wexp = w.wexp;
  return pa;
}

// Small batches (split path, C == 4): the conv0 fragments + zeroing launch alone, then the
// band-conv weight jobs run beside conv0's forward in one multi-job launch (they are only
// needed from conv1 on).  B=32: the 8 us weight-prep launch was on the critical path.
int launch_prep_conv0_multi(ba3c_handle* h, hipStream_t s, const float* prm, const uint8_t* state, int B,
                            const Workspace& w, bool train) {
  WPrep6Args first = wprep6_args(h, prm, w, train);
  WPrep6Args rest = first;
  first.jobs.njobs = 0;                 // job row 0 == njobs: conv0 fragments (+ zeroing)
  rest.w0 = nullptr;                    // rows 0..njobs-1 only, no zeroing: conv0 publishes
  rest.relu = nullptr;                  // into those counters concurrently
  rest.amax = nullptr;
  const Conv0SArgs sa{state, reinterpret_cast<const uint4*>(w.wt + WT_C0S), w.p0, train ? w.c0 : nullptr,
                      train ? w.relu : nullptr, B, w.wexp + WX_CONV0, w.am(AM_P0, h)};
  const int nconv0 = conv0_fwd_p(B);
  if (chain_ok(h) && nconv0 <= h->cus) {
    // one launch: the zeroing workgroups signal; conv0's forward (at most one workgroup per
    // CU) splits its own weight fragments and waits for the zeroing before its first
    // publication; the band-conv weight jobs run beside it
    first.coherent = 1;
    first.w0 = nullptr;
    Conv0SArgs sc = sa;
    sc.w0 = prm + h->tensors[h->idx_conv[0]].offset;
    sc.zsig = h->chain + 4 * CHAIN_PREP_CONV0 + 1;
    sc.zneed = 64;
    sc.zerr = h->chain + 4 * CHAIN_SITES;
    return launch_chain<true, WPrep6Job, Conv0SJob, WPrep6Job>(
        s, CHAIN_PREP_CONV0, 1, 2, 2, first, dim3(64, 1), sc, dim3(nconv0), rest,
        dim3(64, rest.jobs.njobs), h, BA3C_K_CONV0_FWD);
  }
  hipLaunchKernelGGL(wprep6_kernel, dim3(64, 1), dim3(256), 0, s, first);
  HIP_TRY(hipGetLastError());
  ProbeScope ps(h, s, BA3C_K_CONV0_FWD);
  // two workgroups per CU (the register budget of conv0's plain kernel): without the bound the
  // compiler gave the fused body 216 VGPRs + 52 AGPRs, one wave per SIMD, so at B=32 the 160 conv0
  // and 192 weight-prep workgroups did not fit the 256 CUs in one round
  return launch_multi<true, Conv0SJob, WPrep6Job>(s, sa, dim3(nconv0), rest,
                                                  dim3(64, rest.jobs.njobs));
}

// split planes of the band-conv weights for this step (forward; + rotated dgrad in training)
// and, for C == 4, conv0's MFMA B fragments: one launch
int launch_wprep(ba3c_handle* h, hipStream_t s, const float* prm, const Workspace& w, bool train) {
  WPrep6Args pa = wprep6_args(h, prm, w, train);
  const bool c0s = h->cfg.channels == 4;
  if (!c0s) pa.w0 = nullptr;
  hipLaunchKernelGGL(wprep6_kernel, dim3(64, pa.jobs.njobs + (c0s ? 1 : 0)), dim3(256), 0, s, pa);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int launch_conv0_band(ba3c_handle* h, hipStream_t s, const BandArgs& a, const Workspace& w) {
  const Conv0SArgs sa{reinterpret_cast<const uint8_t*>(a.src), reinterpret_cast<const uint4*>(w.wt + WT_C0S),
                      a.out, a.out_code, a.relu_count, a.batch, w.wexp + WX_CONV0, w.am(AM_P0, h)};
  ProbeScope ps(h, s, BA3C_K_CONV0_FWD);
  const dim3 grid(conv0_fwd_p(a.batch));
  HIP_TRY(launch_conv0s_fwd(grid, s, sa));   // ba3c_conv0.hip
  return BA3C_OK;
}

// conv3 forward / input gradient: persistent whole-image workgroups, two per CU (ba3c_conv3.h)
template <bool DG>
#ifndef BA3C_C3_WGPC
#define BA3C_C3_WGPC 2   // conv3's whole-image kernels: persistent workgroups per CU (r06z: 1 made
                         // the forward 19.8 -> 23.9 us and the input gradient 29.3 -> 33.8 us)
#endif
int launch_conv3(ba3c_handle* h, hipStream_t s, int kid, const Conv3Args& a) {
  if (a.batch <= 0) return BA3C_OK;
  const dim3 grid(std::min(a.batch, BA3C_C3_WGPC * h->cus));
  {
    ProbeScope ps(h, s, kid);
    hipLaunchKernelGGL(conv3_band_kernel<DG>, grid, dim3(256), 0, s, a);
  }
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

// ---- forward --------------------------------------------------------------------------
#ifndef BA3C_FC_DEPTH
#define BA3C_FC_DEPTH 2       // k-tile ring depth of fc1's forward at full grids (A/B)
#endif

// Split kernels (pl.split): conv0 (C == 4) and the conv1 / conv2 band convolutions on scaled
// fp16 hi/lo MFMA (ba3c_split.h, ba3c_band6.h); C == 12's conv0, conv3 and fc1 on the bf16x6
// GEMM engine.  BA3C_GENERIC=1: every layer on the fp32-MFMA GEMM engine.
template <int CH>
int run_forward(ba3c_handle* h, hipStream_t s, const LaunchPlan& pl, const float* prm, const uint8_t* state,
                int B, const Workspace& w, bool train) {
  using LY = Lay;
  const int F = h->cfg.fc_neurons;
  const float* W0 = prm + h->tensors[h->idx_conv[0]].offset;
  const float* W1 = prm + h->tensors[h->idx_conv[1]].offset;
  const float* W2 = prm + h->tensors[h->idx_conv[2]].offset;
  const float* W3 = prm + h->tensors[h->idx_conv[3]].offset;
  unsigned long long* rc = train ? w.relu : nullptr;
  uint8_t* c0 = train ? w.c0 : nullptr;
  uint8_t* c1 = train ? w.c1 : nullptr;
  uint8_t* c2 = train ? w.c2 : nullptr;
  const SplitIO io1{AM_P0, WJ_C1F, AM_P1}, io2{AM_P1, WJ_C2F, AM_P2};
  if (!pl.split) {
    ConvFwd<true, 84, 84, CH, 16, 5, 5, 32, 0> cv0{state, W0, w.p0, c0, rc, 1.0f / 255.0f, B * 6400, 32, 25 * CH, 0};
    CHECK((launch_gemm<128, 32, 4, 1>(h, s, BA3C_K_CONV0_FWD, cv0, 1)));
    ConvFwd<false, 40, 40, 32, 32, 5, 5, 32, 0> cv1{w.p0, W1, w.p1, c1, rc, 1.0f, B * 1296, 32, 800, 0};
    CHECK((launch_gemm<128, 32, 4, 1>(h, s, BA3C_K_CONV1_FWD, cv1, 1)));
    ConvFwd<false, 18, 18, 32, 32, 5, 5, 64, 0> cv2{w.p1, W2, w.p2, c2, rc, 1.0f, B * 196, 64, 800, 0};
    CHECK((launch_gemm<128, 64, 4, 1>(h, s, BA3C_K_CONV2_FWD, cv2, 1)));
    ConvFwd<false, 7, 7, 64, 64, 3, 3, 64, 2> c3{w.p2, W3, w.a3, nullptr, rc, 1.0f, B * 25, 64, 576, 0};
    // K = 576 in two halves of 9 k-tiles summed in the workgroup (KS = 2) at every batch, so
    // each output's rounding is the same whatever batch it runs in
    CHECK((launch_gemm<64, 64, 2, 2, decltype(c3), 2>(h, s, BA3C_K_CONV3_FWD, c3, 1)));
  } else {
    if (pl.prep_multi) {
      // small batches: weight prep beside conv0's forward (one launch fewer on the critical path)
      CHECK(launch_prep_conv0_multi(h, s, prm, state, B, w, train));
    } else if (pl.fwd01) {
      // the ring batches: conv0's and conv1's forward as ONE persistent launch, each workgroup
      // taking its own images through both layers (fwd01_kernel, ba3c_conv0.hip)
      CHECK(launch_wprep(h, s, prm, w, train));
      const Conv0SArgs a0{state, reinterpret_cast<const uint4*>(w.wt + WT_C0S), w.p0, c0, rc, B,
                          w.wexp + WX_CONV0, w.am(AM_P0, h)};
      const Band6Args a1 = band6_args<typename LY::C1F>(h, BandArgs{w.p0, nullptr, nullptr, w.p1, c1, rc, B}, w,
                                                        WT_C1F, io1);
      {
        ProbeScope ps(h, s, BA3C_K_CONV0_FWD);
        HIP_TRY(launch_fwd01(2 * h->cus, s, a0, a1));
      }
      h->merged[BA3C_K_CONV0_FWD] |= 1u << BA3C_K_CONV1_FWD;
    } else {
      CHECK(launch_wprep(h, s, prm, w, train));
      if constexpr (CH == 4) {
        CHECK(launch_conv0_band(h, s, BandArgs{reinterpret_cast<const float*>(state), nullptr, nullptr, w.p0, c0,
                                               rc, B}, w));
      } else {
        ConvFwd<true, 84, 84, CH, 16, 5, 5, 32, 0> cv0{state, W0, w.p0, c0, rc, 1.0f / 255.0f,
                                                      B * 6400, 32, 25 * CH, 0, w.am(AM_P0, h)};
        CHECK((launch_gemm<128, 32, 4, 1>(h, s, BA3C_K_CONV0_FWD, cv0, 1)));
      }
    }
    if (!pl.fwd01)
      CHECK((launch_band6<typename LY::C1F>(h, s, BA3C_K_CONV1_FWD, BandArgs{w.p0, nullptr, nullptr, w.p1, c1, rc, B},
                                            w, WT_C1F, io1, pl.ring_fwd)));
    const BandArgs a2{w.p1, nullptr, nullptr, w.p2, c2, rc, B};
    if (pl.conv2_small)
      CHECK(launch_band6<typename LY::C2FS>(h, s, BA3C_K_CONV2_FWD, a2, w, WT_C2F, io2));
    else
      CHECK(launch_band6<typename LY::C2F>(h, s, BA3C_K_CONV2_FWD, a2, w, WT_C2F, io2));
    // whole-image workgroups at every batch: an image's a3 does not depend on its batch
    CHECK(launch_conv3<false>(h, s, BA3C_K_CONV3_FWD, Conv3Args{w.p2, w.wt6 + 2 * (size_t)WT_C3F, w.wexp + WJ_C3F,
                                                                  w.a3, rc, nullptr, B, nullptr}));
  }
  // split-K: K = 1600 in FC_SPLIT fixed chunks (a 128x64 tile over all of K is one
  // workgroup's 50 serial k-tiles: latency-bound at any batch); the chunk sums (+ legacy bias,
  // ReLU, count) are finished inside the heads kernel (run_heads), which reads them anyway
  FcFwd fc{w.a3, prm + h->tensors[h->idx_fc1].offset, w.h, rc, h->per, h->wstride,
           h->cfg.replace_with_conv ? 0 : 1, B, F, 1600, FC_KCHUNK, w.fcpart};
  {
    ProbeScope ps(h, s, BA3C_K_FC1_FWD);
    const dim3 grid((B + 127) / 128, (F + 63) / 64, FC_SPLIT);
    constexpr bool HV = true;
    constexpr int KSS = 2;   // small batches: even and odd k-tiles in two groups
    if (h->g6 && B <= 64)   // 64-row tiles: same per-row K order, half the dead rows staged
      hipLaunchKernelGGL((gemm6_kernel<64, 64, 2, 2, FcFwd, 4, KSS, HV>), dim3((B + 63) / 64, grid.y, grid.z),
                         dim3(GEMM_THREADS * KSS), 0, s, fc);
    else if (h->g6 && (int)(grid.x * grid.y * grid.z) < h->cus)
      hipLaunchKernelGGL((gemm6_kernel<128, 64, 2, 2, FcFwd, 4, 1, HV>), grid, dim3(GEMM_THREADS), 0, s, fc);
    else if (h->g6)   // (full grids on 128 x 128 tiles, same K chunks, were bit-identical and
                      // slower: r06v 0.0299 -> 0.0333 ms, not kept)
      hipLaunchKernelGGL((gemm6_kernel<128, 64, 2, 2, FcFwd, BA3C_FC_DEPTH, 1, HV>), grid, dim3(GEMM_THREADS), 0, s, fc);
    else
      hipLaunchKernelGGL((gemm_kernel<128, 64, 2, 2, FcFwd>), grid, dim3(GEMM_THREADS), 0, s, fc);
  }
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

// Create the side stream + fork/join events on the first training call made outside a
// graph capture (stream creation is not a capturable operation).
int ensure_side_stream(ba3c_handle* h, hipStream_t s) {
  if (h->sw.overlap == 0 || h->side) return BA3C_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(s, &cs));
  if (cs != hipStreamCaptureStatusNone) return BA3C_OK;
  HIP_TRY(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
  for (auto& e : h->ev_fork) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
  return BA3C_OK;
}

// One backward pass on the caller's stream.  phase 0: the whole pass.  phase 1: the heads and
// fc1 products and their reductions (those gradients are final when it returns); phase 2:
// conv3..conv0 and theirs.  Phases 1 + 2 compute exactly phase 0; between them a data-parallel
// caller can all-reduce the fc1 + heads bucket (most of the parameters) while the conv layers
// run.
// The weight-gradient kernels (heads, fc1, conv3..conv1) run on `ws`: the side stream where
// the plan asks for it, each after the event that publishes its output gradient (the side
// stream joins a graph capture of `s` through the fork events), else `s`.  The input-gradient
// chain and conv0's weight gradient (own partials region) stay on `s`, which joins `ws` at the
// end.  Under pl.mj* a layer's input- and weight-gradient kernels are one multi-job launch on
// `s` instead (no side stream, no events).  Each layer: the split path, then the BA3C_GENERIC
// engine path (fp32-MFMA GEMMs).
template <int CH>
struct BackwardPass {
  using LY = Lay;
  using W1 = typename LY::W1;
  ba3c_handle* h;
  hipStream_t s, ws;
  const LaunchPlan& pl;
  const Workspace& w;
  const float* prm;
  const uint8_t* state;
  float* grads;
  int B, phase;
  int nfork = 0;

  // every weight-gradient reduction is deferred into one launch at the end (h->rjobs)
  BackwardPass(ba3c_handle* h_, hipStream_t s_, const LaunchPlan& pl_, const Workspace& w_, const float* prm_,
               const uint8_t* state_, float* grads_, int B_, int phase_)
      : h(h_), s(s_), ws(pl_.side_stream && h_->side ? h_->side : s_), pl(pl_), w(w_), prm(prm_), state(state_),
        grads(grads_), B(B_), phase(phase_) {
    h->rjobs.n = 0;
    h->rjobs.blk0[0] = 0;
  }

  const float* param(int t) const { return prm + h->tensors[t].offset; }
  float* grad(int t) const { return grads + h->tensors[t].offset; }
  Wg6Args wa1() const { return Wg6Args{w.p0, w.dp1, w.c1, w.part_1, B, w.am(AM_P0, h), w.am(AM_DP1, h)}; }

  int run() {
    CHECK(fork());
    if (phase != 2) CHECK(fc_and_heads());
    if (phase == 1) return finish();
    CHECK(conv3());
    if (phase == 2 && h->ev_mid) HIP_TRY(hipEventRecord(h->ev_mid, s));
    CHECK(conv2());
    CHECK(conv1());
    CHECK(conv0());
    // all (remaining) weight-gradient reductions: one launch, every gradient element written once
    return finish();
  }

  int fork() {
    if (ws == s) return BA3C_OK;
    HIP_TRY(hipEventRecord(h->ev_fork[nfork], s));
    HIP_TRY(hipStreamWaitEvent(ws, h->ev_fork[nfork], 0));
    ++nfork;
    return BA3C_OK;
  }

  // join the side stream and run the deferred reductions of this phase in one launch
  int finish() {
    if (h->pend_scalars && phase != 1) {   // no launch took the deferred scalar reduction
      // (phase 1 leaves it pending: conv3's input-gradient launch in phase 2 takes it)
      const ScalarsJob::Args& sa = h->scalars_args;
      ProbeScope ps(h, s, BA3C_K_SCALARS);
      hipLaunchKernelGGL(scalars_kernel, dim3(1), dim3(256), 0, s, sa.terms, sa.B, sa.beta, sa.relu, sa.out);
      HIP_TRY(hipGetLastError());
      h->pend_scalars = false;
    }
    if (ws != s) {
      HIP_TRY(hipEventRecord(h->ev_join, ws));
      HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));
    }
    return h->rjobs.n ? launch_reduce_all(h, s, h->rjobs) : BA3C_OK;
  }

  int conv_reduce(int M, int N, int S, int layer, int cin, int cinpad, const float* part) {
    ReduceMap mp{};
    mp.kind = 0;
    mp.M = M;
    mp.N = N;
    mp.cin = cin;
    mp.cinpad = cinpad;
    mp.dst = grad(h->idx_conv[layer]);
    return add_reduce(h, part, S, mp);
  }

  // head and fc1 weight gradients (X = h, G = [dz | dV]: d fc-pi/W, fc-pi/b, fc-v/W, fc-v/b; fc1's
  // + legacy bias) and fc1's input gradient -> dY3 (ReluGrad of conv3 fused)
  int fc_and_heads() {
    const int F = h->cfg.fc_neurons, A = h->cfg.num_actions;
    const bool legacy = !h->cfg.replace_with_conv;
    const WgradPlan ph = plan_wgrad(F + 1, A + 1, B, 128, 32), pf = fc1w_plan(F, B, legacy, pl.fc1_big_tiles);
    const BatchWgrad gh{w.h, w.dzv, w.part_h, F, MAXA, 1, ph.M, ph.N, ph.K, ph.kchunk};
    const BatchWgrad gf{w.a3, w.dh, w.part_f, 1600, F, legacy ? 1 : 0, pf.M, pf.N, pf.K, pf.kchunk};
    const FcDgrad d{w.dh, param(h->idx_fc1), w.a3, w.dy3, h->per, h->wstride, B, 1600, F, 0};
    if (pl.mj_fc) {   // one launch (the engine is the bf16x6 one: mj_fc is a split-path decision)
      const int dbm = pl.fc1_big_tiles ? 128 : 64, fbn = dbm;
      const dim3 gd((d.M + dbm - 1) / dbm, (d.N + dbm - 1) / dbm, 1), ghd((ph.M + 127) / 128, (ph.N + 31) / 32, ph.S),
          gfd((pf.M + 127) / 128, (pf.N + fbn - 1) / fbn, pf.S);
      h->merged[BA3C_K_FC1_DGRAD] |= (1u << BA3C_K_FC1_WGRAD) | (1u << BA3C_K_HEAD_WGRAD);
#ifndef BA3C_FCD_DEPTH
#define BA3C_FCD_DEPTH 2      // k-tile ring depth of the large-batch fc1 backward jobs (A/B)
#endif
      if (!pl.big)
        CHECK((launch_multi<false, Gemm6Job<64, 64, 2, 2, FcDgrad, 4>, Gemm6Job<128, 32, 4, 1, BatchWgrad, 4>,
                            Gemm6Job<128, 64, 2, 2, BatchWgrad, 4>>(s, d, gd, gh, ghd, gf, gfd, h, BA3C_K_FC1_DGRAD)));
      else if (pl.fc1_big_tiles)
        CHECK((launch_multi<false, Gemm6Job<128, 128, 2, 2, FcDgrad, BA3C_FCD_DEPTH>,
                            Gemm6Job<128, 32, 4, 1, BatchWgrad, BA3C_FCD_DEPTH>,
                            Gemm6Job<128, 128, 2, 2, BatchWgrad, BA3C_FCD_DEPTH>>(s, d, gd, gh, ghd, gf, gfd, h,
                                                                                BA3C_K_FC1_DGRAD)));
      else   // (the small tiles at full grids: no plan asks for them today)
        CHECK((launch_multi<false, Gemm6Job<64, 64, 2, 2, FcDgrad, BA3C_FCD_DEPTH>, Gemm6Job<128, 32, 4, 1, BatchWgrad, BA3C_FCD_DEPTH>,
                            Gemm6Job<128, 64, 2, 2, BatchWgrad, BA3C_FCD_DEPTH>>(s, d, gd, gh, ghd, gf, gfd, h, BA3C_K_FC1_DGRAD)));
    } else {
      CHECK((launch_gemm<128, 32, 4, 1>(h, ws, BA3C_K_HEAD_WGRAD, gh, ph.S)));
      CHECK((launch_gemm<128, 64, 2, 2>(h, ws, BA3C_K_FC1_WGRAD, gf, pf.S)));
      CHECK((launch_gemm<64, 64, 2, 2>(h, s, BA3C_K_FC1_DGRAD, d, 1)));
    }
    ReduceMap mh{};
    mh.kind = 2;
    mh.M = ph.M;
    mh.N = ph.N;
    mh.A = A;
    mh.dst = grad(h->idx_piW);
    mh.dst_pib = grad(h->idx_pib);
    mh.dst_vW = grad(h->idx_vW);
    mh.dst_vb = grad(h->idx_vb);
    CHECK(add_reduce(h, w.part_h, ph.S, mh));
    ReduceMap mf{};
    mf.kind = 1;
    mf.M = pf.M;
    mf.N = pf.N;
    mf.per = h->per;
    mf.wstride = h->wstride;
    mf.dst = grad(h->idx_fc1);
    CHECK(add_reduce(h, w.part_f, pf.S, mf));
    return fork();
  }

  int conv3() {
    if (pl.split) {
      // whole-image kernels (ba3c_conv3.h) at every batch: an image's dP2 rounds the same in
      // any batch.  Input gradient first: it publishes dY3's per-image maxima, the weight
      // gradient's scale (both on `s`, whatever the side-stream setting); the deferred
      // TfDictOp reduction rides on it as one extra workgroup
      const Conv3Args da{w.dy3, w.wt6 + 2 * (size_t)WT_C3D, w.wexp + WJ_C3D, w.dp2, nullptr,
                         w.am(AM_DP2, h), B, w.am(AM_DY3, h)};
      const int gx = pl.conv3_slabs;   // one slab per weight-gradient workgroup
      if (pl.mj) {
        // small batches: input and weight gradient in one launch (two 256-thread workgroups per
        // weight-gradient slab; the weight gradient reduces max |dY3| itself, since the input
        // gradient publishes it only as it runs)
        const Conv3WArgs wa{w.p2, w.dy3, w.part_3, B, w.am(AM_P2, h), nullptr, 1};
        CHECK((launch_multi<true, Conv3DJob, Conv3WJob>(s, da, dim3(std::min(B, 2 * h->cus)), wa, dim3(gx, 2),
                                                         0, dim3(0, 1, 1), h, BA3C_K_CONV3_DGRAD)));
        h->merged[BA3C_K_CONV3_DGRAD] |= 1u << BA3C_K_CONV3_WGRAD;
      } else {
        if (pl.big && h->pend_scalars) {
          CHECK((launch_multi<true, Conv3DJob, ScalarsJob>(s, da, dim3(std::min(B, BA3C_C3_WGPC * h->cus)), h->scalars_args,
                                                            dim3(1), 0, dim3(0, 1, 1), h, BA3C_K_CONV3_DGRAD)));
          h->merged[BA3C_K_CONV3_DGRAD] |= 1u << BA3C_K_SCALARS;   // the reduction rode on this launch
          h->pend_scalars = false;
        } else {
          CHECK(launch_conv3<true>(h, s, BA3C_K_CONV3_DGRAD, da));
        }
        const Conv3WArgs wa{w.p2, w.dy3, w.part_3, B, w.am(AM_P2, h), w.am(AM_DY3, h), 0};
        {
          ProbeScope ps(h, s, BA3C_K_CONV3_WGRAD);
          hipLaunchKernelGGL(conv3_wgrad_kernel, dim3(gx), dim3(512), 0, s, wa);
        }
        HIP_TRY(hipGetLastError());
      }
      CHECK(conv_reduce(576, 64, gx, 3, 64, 64, w.part_3));
    } else {
      const WgradPlan p = plan_wgrad(576, 64, B * 25, 128, 64);
      ConvWgrad<false, 7, 7, 64, 3, 3, 64, false> g{w.p2, w.dy3, nullptr, w.part_3, 1.0f, p.M, p.N, p.K, p.kchunk};
      ConvDgrad<7, 7, 64, 3, 3, 64, false> d{w.dy3, nullptr, param(h->idx_conv[3]), w.dp2, B * 49, 64, 576, 0, nullptr};
      CHECK((launch_gemm<128, 64, 4, 1>(h, ws, BA3C_K_CONV3_WGRAD, g, p.S)));
      CHECK((launch_gemm<64, 64, 2, 2>(h, s, BA3C_K_CONV3_DGRAD, d, 1)));
      CHECK(conv_reduce(p.M, p.N, p.S, 3, 64, 64, w.part_3));
    }
    return fork();
  }

  int conv2() {
    if (!pl.split) {
      const WgradPlan p = plan_wgrad(800, 64, B * 196, 128, 64);
      ConvWgrad<false, 18, 18, 32, 5, 5, 64, true> g{w.p1, w.dp2, w.c2, w.part_2, 1.0f, p.M, p.N, p.K, p.kchunk};
      CHECK((launch_gemm<128, 64, 4, 1>(h, ws, BA3C_K_CONV2_WGRAD, g, p.S)));
      CHECK(conv_reduce(p.M, p.N, p.S, 2, 32, 32, w.part_2));
      ConvDgrad<18, 18, 32, 5, 5, 64, true> d{w.dp2, w.c2, param(h->idx_conv[2]), w.dp1, B * 324, 32, 1600, 0};
      CHECK((launch_gemm<128, 32, 4, 1>(h, s, BA3C_K_CONV2_DGRAD, d, 1)));
      return fork();
    }
    using W2 = typename LY::W2;
    const Wg6Args wa{w.p1, w.dp2, w.c2, w.part_2, B, w.am(AM_P1, h), w.am(AM_DP2, h)};
    const BandArgs ba{w.dp2, w.c2, w.wt + WT_C2D, w.dp1, nullptr, nullptr, B};
    const SplitIO io{AM_DP2, WJ_C2D, AM_DP1};
    float* dW2 = grad(h->idx_conv[2]);
    if (!pl.mj && !pl.mj_c2) {
      CHECK(launch_wgrad6<W2>(h, ws, BA3C_K_CONV2_WGRAD, wa, W6_P2, dW2));
      if (pl.conv2_small)
        CHECK(launch_band6<typename LY::C2DS>(h, s, BA3C_K_CONV2_DGRAD, ba, w, WT_C2D, io));
      else
        CHECK(launch_band6<typename LY::C2D>(h, s, BA3C_K_CONV2_DGRAD, ba, w, WT_C2D, io));
      return fork();
    }
    // input and weight gradient in one launch: the small-batch geometry, or the whole-map one
    const dim3 wg = wgrad6_grid<W2>(W6_P2, B);
    if (pl.mj) {
      CHECK((launch_multi<true, Band6Job<typename LY::C2DS>, Wg6Job<W2>>(
          s, band6_args<typename LY::C2DS>(h, ba, w, WT_C2D, io), dim3(B * LY::C2DS::G::NBANDS), wa, wg)));
    } else {
      using C2D = typename LY::C2D;
      CHECK((launch_multi<true, Band6Job<C2D>, Wg6Job<W2>>(s, band6_args<C2D>(h, ba, w, WT_C2D, io),
                                                          dim3(B * C2D::G::NBANDS), wa, wg, 0, dim3(0, 1, 1), h,
                                                          BA3C_K_CONV2_DGRAD)));
    }
    h->merged[BA3C_K_CONV2_DGRAD] |= 1u << BA3C_K_CONV2_WGRAD;
    return reduce_wgrad6<W2>(h, wa, (int)wg.x, dW2);
  }

  // conv1: the weight gradient (alone on `ws`, or a job of the input gradient's launch; the pair
  // with conv0's waits for conv0()), then the input gradient
  int conv1() {
    if (!pl.split) {
      const WgradPlan p = plan_wgrad(800, 32, B * 1296, 128, 32);
      ConvWgrad<false, 40, 40, 32, 5, 5, 32, true> g{w.p0, w.dp1, w.c1, w.part_1, 1.0f, p.M, p.N, p.K, p.kchunk};
      CHECK((launch_gemm<128, 32, 4, 1>(h, ws, BA3C_K_CONV1_WGRAD, g, p.S)));
      CHECK(conv_reduce(p.M, p.N, p.S, 1, 32, 32, w.part_1));
      ConvDgrad<40, 40, 32, 5, 5, 32, true> d{w.dp1, w.c1, param(h->idx_conv[1]), w.dp0, B * 1600, 32, 800, 0};
      return launch_gemm<128, 32, 4, 1>(h, s, BA3C_K_CONV1_DGRAD, d, 1);
    }
    const Wg6Args wa = wa1();
    float* dW1 = grad(h->idx_conv[1]);
    const int P = pl.conv1_slabs;
    const BandArgs ba{w.dp1, w.c1, w.wt + WT_C1D, w.dp0, nullptr, nullptr, B};
    const SplitIO io{AM_DP1, WJ_C1D, AM_DP0};
    if (pl.mj) {
      // small batches: input and weight gradient in one launch
      CHECK((launch_multi<true, Band6Job<typename LY::C1D>, Wg6Job<W1>>(
          s, band6_args<typename LY::C1D>(h, ba, w, WT_C1D, io), dim3(B * LY::C1D::G::NBANDS), wa,
          wgrad6_grid<W1>(P, B))));
      h->merged[BA3C_K_CONV1_DGRAD] |= 1u << BA3C_K_CONV1_WGRAD;
      return reduce_wgrad6<W1>(h, wa, P, dW1);
    }
    if (pl.conv1_wgrad == Conv1Wgrad::whole) {
      {
        ProbeScope ps(h, ws, BA3C_K_CONV1_WGRAD);
        hipLaunchKernelGGL(wgrad6w_kernel<typename LY::W1W>, dim3(P), dim3(256), 0, ws, wa);
      }
      HIP_TRY(hipGetLastError());
      CHECK(reduce_wgrad6<W1>(h, wa, P, dW1));
    } else if (pl.conv1_wgrad == Conv1Wgrad::wgrad6) {
      CHECK(launch_wgrad6<W1>(h, ws, BA3C_K_CONV1_WGRAD, wa, P, dW1));
    }
    return launch_band6<typename LY::C1D>(h, s, BA3C_K_CONV1_DGRAD, ba, w, WT_C1D, io, pl.ring_dgrad);
  }

  // conv0 (no input gradient: the frames are not trainable)
  int conv0() {
    ReduceMap mp{};
    mp.kind = 0;
    mp.N = 32;
    mp.cin = CH;
    mp.cinpad = 16;
    mp.dst = grad(h->idx_conv[0]);
    if (pl.split && CH == 4) {
      const int P = pl.conv0_slabs;
      const Conv0WArgs a0{state, w.dp0, w.c0, w.part0, B, w.am(AM_DP0, h)};
      if (pl.conv1_wgrad == Conv1Wgrad::pair0) {
        // conv1's whole-channel weight gradient (MFMA-bound) beside conv0's (VALU-bound): one
        // workgroup of each per CU, one launch (ba3c_conv0.hip)
        const Wg6Args wa = wa1();
        {
          ProbeScope ps(h, s, BA3C_K_CONV0_WGRAD);
          HIP_TRY(launch_wgrad01_pair(s, wa, pl.conv1_slabs, a0, P));
        }
        h->merged[BA3C_K_CONV0_WGRAD] |= 1u << BA3C_K_CONV1_WGRAD;
        CHECK(reduce_wgrad6<W1>(h, wa, pl.conv1_slabs, grad(h->idx_conv[1])));
      } else {
        ProbeScope ps(h, s, BA3C_K_CONV0_WGRAD);
        HIP_TRY(launch_conv0s_wgrad(dim3(P), s, a0));
      }
      mp.M = Conv0W<2>::M;
      return add_reduce(h, w.part0, P, mp);
    }
    // C == 12, or BA3C_GENERIC: the GEMM engine
    const WgradPlan p = plan_wgrad(25 * CH, 32, B * 6400, 128, 32);
    ConvWgrad<true, 84, 84, CH, 5, 5, 32, true> g{state, w.dp0, w.c0, w.part0, 1.0f / 255.0f, p.M, p.N, p.K, p.kchunk};
    CHECK((launch_gemm<128, 32, 4, 1>(h, s, BA3C_K_CONV0_WGRAD, g, p.S)));
    mp.M = p.M;
    return add_reduce(h, w.part0, p.S, mp);
  }
};

// the PPO form of a training heads launch (ba3c_train_grads_ppo_ext): rows replaces R
struct PpoArgs {
  const float* rows;   // [B][4] {R, V_old, l_old, w}
  float* ratio;        // [B] or null
  float clip_eps, vclip_eps;
  unsigned flags;
};

// the heads instantiation of (F, A) for one loss: features per lane unrolled (heads_sample),
// the smallest instantiation that covers F
template <int LOSS>
void launch_heads(hipStream_t s, int B, const HeadsArgsOf<LOSS>& a) {
  const int F = a.F;
  const dim3 g((B + 3) / 4), t(256);
  // the reference's Atari action sets are mostly 4 actions: compile-time A there (heads_sample)
  if (a.A == 4 && F <= 128 && F > 64) hipLaunchKernelGGL((heads_kernel<2, FC_SPLIT, 4, LOSS>), g, t, 0, s, a);
  else if (a.A == 4 && F <= 512 && F > 256) hipLaunchKernelGGL((heads_kernel<8, FC_SPLIT, 4, LOSS>), g, t, 0, s, a);
  else if (F <= 64) hipLaunchKernelGGL((heads_kernel<1, FC_SPLIT, 0, LOSS>), g, t, 0, s, a);
  else if (F <= 128) hipLaunchKernelGGL((heads_kernel<2, FC_SPLIT, 0, LOSS>), g, t, 0, s, a);
  else if (F <= 256) hipLaunchKernelGGL((heads_kernel<4, FC_SPLIT, 0, LOSS>), g, t, 0, s, a);
  else if (F <= 512) hipLaunchKernelGGL((heads_kernel<8, FC_SPLIT, 0, LOSS>), g, t, 0, s, a);
  else hipLaunchKernelGGL((heads_kernel<0, FC_SPLIT, 0, LOSS>), g, t, 0, s, a);
}

int run_heads(ba3c_handle* h, hipStream_t s, const float* prm, const Workspace& w, int B,
              const int64_t* action, const float* R, float beta, float explore, bool train,
              float* probs, float* probsT, float* value, double* scalars = nullptr,
              bool defer_scalars = false, const PpoArgs* ppo = nullptr) {
  HeadsArgsPpo a{};
  if (ppo) {
    a.rows = reinterpret_cast<const float4*>(ppo->rows);
    a.ratio = ppo->ratio;
    a.clip_eps = ppo->clip_eps;
    a.vclip_eps = ppo->vclip_eps;
    a.flags = ppo->flags;
  }
  a.fcpart = w.fcpart;
  a.fc_split = FC_SPLIT;
  a.per = h->per;
  a.wstride = h->wstride;
  a.fc_w1 = prm + h->tensors[h->idx_fc1].offset;
  a.relu_count = train ? w.relu : nullptr;
  a.done = w.relu + RELU_SLOTS;
  // the scalar reduction rides on the heads launch (last workgroup) for small batches only:
  // with B/4 workgroups all finishing together, B > 256 puts hundreds of same-address atomics
  // and a B-long serial reduction at the kernel's tail (r02f: heads 29 -> 75 us at B=2048)
  const bool fuse_scalars = train && scalars && B <= 256;
  a.scalars = fuse_scalars ? scalars : nullptr;
  a.h = w.h;
  a.piW = prm + h->tensors[h->idx_piW].offset;
  a.pib = prm + h->tensors[h->idx_pib].offset;
  a.vW = prm + h->tensors[h->idx_vW].offset;
  a.vb = prm + h->tensors[h->idx_vb].offset;
  a.action = action;
  a.R = R;
  a.probs = probs;
  a.probsT = probsT;
  a.value = value;
  a.dzv = w.dzv;
  a.dh = w.dh;
  a.terms = w.terms;
  a.B = B;
  a.F = h->cfg.fc_neurons;
  a.A = h->cfg.num_actions;
  a.train = train ? 1 : 0;
  a.legacy = h->cfg.replace_with_conv ? 0 : 1;
  a.beta = beta;
  a.explore = explore;
  a.invB = 1.0f / (float)B;
  {
    ProbeScope ps(h, s, BA3C_K_HEADS);
    if (ppo && train) launch_heads<LOSS_PPO>(s, B, a);
    else launch_heads<LOSS_A3C>(s, B, a);
  }
  HIP_TRY(hipGetLastError());
  if (train && scalars && !fuse_scalars && defer_scalars) {
    h->scalars_args = ScalarsJob::Args{w.terms, B, beta, w.relu, scalars};
    h->pend_scalars = true;      // launched by BackwardPass (conv3's input gradient or finish)
  } else if (train && scalars && !fuse_scalars) {
    ProbeScope ps(h, s, BA3C_K_SCALARS);
    hipLaunchKernelGGL(scalars_kernel, dim3(1), dim3(256), 0, s, w.terms, B, beta, w.relu, scalars);
    HIP_TRY(hipGetLastError());
  }
  return BA3C_OK;
}

// the optimizer id as a compile-time kernel index (apply_update_impl validates the id first)
template <class F>
int with_opt(int32_t opt, F&& f) {
  switch (opt) {
    case BA3C_OPT_ADAM: return f(std::integral_constant<int, 0>{});
    case BA3C_OPT_GD: return f(std::integral_constant<int, 1>{});
    case BA3C_OPT_ADAGRAD: return f(std::integral_constant<int, 2>{});
    case BA3C_OPT_ADADELTA: return f(std::integral_constant<int, 3>{});
    case BA3C_OPT_MOMENTUM: return f(std::integral_constant<int, 4>{});
    case BA3C_OPT_RMS: return f(std::integral_constant<int, 5>{});
    default: return fail(BA3C_ERR_INVALID, "unknown optimizer id");
  }
}

bool check_ptr(const void* p) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

namespace {
struct Rccl {
  ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
  ncclResult_t (*init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                             hipStream_t) = nullptr;
  ncclResult_t (*destroy)(ncclComm_t) = nullptr;
  ncclResult_t (*abort)(ncclComm_t) = nullptr;
  const char* (*error_string)(ncclResult_t) = nullptr;
  bool ok = false;
};
const Rccl& rccl() {
  static Rccl r = [] {
    Rccl x;
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return x;
    x.get_unique_id = reinterpret_cast<decltype(x.get_unique_id)>(dlsym(lib, "ncclGetUniqueId"));
    x.init_rank = reinterpret_cast<decltype(x.init_rank)>(dlsym(lib, "ncclCommInitRank"));
    x.all_reduce = reinterpret_cast<decltype(x.all_reduce)>(dlsym(lib, "ncclAllReduce"));
    x.destroy = reinterpret_cast<decltype(x.destroy)>(dlsym(lib, "ncclCommDestroy"));
    x.abort = reinterpret_cast<decltype(x.abort)>(dlsym(lib, "ncclCommAbort"));
    x.error_string = reinterpret_cast<decltype(x.error_string)>(dlsym(lib, "ncclGetErrorString"));
    x.ok = x.get_unique_id && x.init_rank && x.all_reduce && x.destroy && x.abort && x.error_string;
    return x;
  }();
  return r;
}
int rccl_fail(ncclResult_t e, const char* what) {
  return fail(BA3C_ERR_HIP, std::string(what) + ": " + rccl().error_string(e));
}
}  // namespace

// What a decision entry point takes beyond a step's arguments, as the caller gave it.
struct Decision {
  int32_t* aux;
  int32_t skip_lo, skip_hi, sticky_q16;
  int32_t start_lo = 19, start_hi = 19;   // the fixed start: what a game without drawn starts passes
};

// The argument checks of every step / decision / render entry point of the games, in one order;
// the first that fails is the one reported.  render: no action, no outputs, no limit.  count: the
// entry point's name of a.rows; aux_align: of a decision's aux rows, in bytes.
static int game_check(const EnvArgs& a, const char* count, bool render, const Decision* d, size_t aux_align) {
  if (render ? !a.game : !a.game || !a.action)
    return fail(BA3C_ERR_INVALID, render ? "null game pointer" : "null game / action pointer");
  if (d && !d->aux) return fail(BA3C_ERR_INVALID, "null aux pointer");
  if (!render && (!a.reward || !a.over || !a.ep_score)) return fail(BA3C_ERR_INVALID, "null output pointer");
  if (a.rows < 1 || a.limit < 1)
    return fail(BA3C_ERR_INVALID, std::string(count) + (render ? "" : " and limit") + " must be >= 1");
  if (!check_ptr(a.game) || (a.state && !check_ptr(a.state)) || (reinterpret_cast<uintptr_t>(a.frame) & 3))
    return fail(BA3C_ERR_INVALID, "game / state must be 16-byte and frame 4-byte aligned");
  if (!d) return BA3C_OK;
  if (reinterpret_cast<uintptr_t>(d->aux) & (aux_align - 1))
    return fail(BA3C_ERR_INVALID, "aux must be " + std::to_string(aux_align) + "-byte aligned");
  if (d->skip_lo < 1 || d->skip_hi < d->skip_lo || d->skip_hi > 16)
    return fail(BA3C_ERR_INVALID, "frame skip must satisfy 1 <= skip_lo <= skip_hi <= 16");
  if (d->sticky_q16 < 0 || d->sticky_q16 > 65536)
    return fail(BA3C_ERR_INVALID, "sticky_q16 must be in [0, 65536]");
  if (d->start_lo < 4 || d->start_hi < d->start_lo || d->start_hi > 19)
    return fail(BA3C_ERR_INVALID, "start half-gap must satisfy 4 <= start_lo <= start_hi <= 19");
  return BA3C_OK;
}

// Every step / decision / render entry point of the games (Sim: ba3c_envkernel.h): the checks,
// then sim_kernel over a.rows rows.  d: a decision's arguments (null: a step, or with a null
// a.action and render set, a render, which never writes the row).
template <class Sim>
static int game_launch(void* stream, const EnvArgs& a, const Decision* d = nullptr, bool render = false) {
  if (int rc = game_check(a, Sim::PLAYERS == 1 ? "n_envs" : "n_games", render, d, alignof(typename Sim::Aux)))
    return rc;
  if (render && !a.frame && !a.state) return BA3C_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Decision v = d ? *d : Decision{nullptr, 1, 1, 0};
  const DuelDecideArgs all{{v.aux, v.skip_lo, (uint32_t)(v.skip_hi - v.skip_lo + 1), (uint32_t)v.sticky_q16},
                           v.start_lo, (uint32_t)(v.start_hi - v.start_lo + 1)};
  const typename Sim::DecideArgs& k = all;            // a game without drawn starts takes the base
  const auto kernel = d ? sim_kernel<Sim, true> : sim_kernel<Sim, false>;
  hipLaunchKernelGGL(kernel, dim3(a.rows), dim3(256), 0, s, a, k);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

static EnvArgs render_args(const int32_t* game, int32_t n, uint8_t* frame, uint8_t* state) {
  return EnvArgs{const_cast<int32_t*>(game), nullptr, 1, n, nullptr, nullptr, nullptr, frame, state};
}

// The colour view of selected simulators (env_view_kernel; ba3c_amd/view.py is its oracle).
template <class Rules>
static int env_view(void* stream, const int32_t* game, int32_t n_envs, const int32_t* sel, int32_t n_sel,
                    const uint8_t* palette, const uint8_t* hud, int32_t scale, uint8_t* out) {
  if (!game || !palette || !out) return fail(BA3C_ERR_INVALID, "null game / palette / out pointer");
  if (n_envs < 1 || n_sel < 1) return fail(BA3C_ERR_INVALID, "n_envs and n_sel must be >= 1");
  if (scale < 1 || scale > VIEW_MAX_SCALE) return fail(BA3C_ERR_INVALID, "scale must be in [1, 8]");
  if (!check_ptr(game) || ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(sel) |
                            reinterpret_cast<uintptr_t>(hud)) & 3))
    return fail(BA3C_ERR_INVALID, "game must be 16-byte and sel / hud / out 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ViewArgs a{game, n_envs, sel, palette, hud, scale, out};
  hipLaunchKernelGGL(env_view_kernel<Rules>, dim3(n_sel), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

// =========================================================================================
extern "C" {

int ba3c_version(void) { return 1; }

const char* ba3c_last_error(void) { return g_err.c_str(); }

int ba3c_create(const ba3c_config* cfg, ba3c_handle** out) {
  if (!cfg || !out) return fail(BA3C_ERR_INVALID, "null argument");
  const ba3c_config& c = *cfg;
  if (c.channels != 4 && c.channels != 12)
    return fail(BA3C_ERR_INVALID, "channels must be 4 or 12 (FRAME_HISTORY * --channels)");
  if (c.num_actions < 1 || c.num_actions >= MAXA)
    return fail(BA3C_ERR_INVALID, "num_actions must be in [1, 31]");
  if (c.max_batch < 1 || c.max_batch > kMaxBatch)
    return fail(BA3C_ERR_INVALID, "max_batch must be in [1, 16384]");
  const int splits = c.replace_with_conv ? c.fc_splits : c.ps;
  if (splits < 1 || c.fc_neurons < 4 || c.fc_neurons % splits != 0 || (c.fc_neurons / splits) % 4 != 0)
    return fail(BA3C_ERR_INVALID, "fc_neurons must be a multiple of 4*fc_splits (or 4*ps)");
  // launch-structure switches (each exercised by a GPU test; values outside the listed ones
  // are rejected rather than coerced, so an A/B run measures what it asked for)
  Switches sw;
  struct Switch {
    const char* name;
    const char* digits;   // the accepted values
    void (*set)(Switches&, int);
  };
  const Switch switches[] = {
      {"BA3C_GENERIC", "01", [](Switches& w, int v) { w.generic = v != 0; }},
      {"BA3C_C1PAIR", "02", [](Switches& w, int v) { w.c1pair = v; }},
      {"BA3C_SCALARS_RIDE", "01", [](Switches& w, int v) { w.scalars_ride = v != 0; }},
      {"BA3C_OVERLAP", "012", [](Switches& w, int v) { w.overlap = v; }},
      {"BA3C_MULTI", "01", [](Switches& w, int v) { w.multi = v != 0; }},
      {"BA3C_MULTI_BIG", "0123", [](Switches& w, int v) { w.multi_big = v; }},
      {"BA3C_FUSED_UPDATE", "01", [](Switches& w, int v) { w.fused_update = v != 0; }},
      {"BA3C_RING", "01", [](Switches& w, int v) { w.ring = v != 0; }},
      {"BA3C_CHAIN", "01", [](Switches& w, int v) { w.chain = v != 0; }},
      {"BA3C_FWD01", "01", [](Switches& w, int v) { w.fwd01 = v != 0; }},
  };
  for (const Switch& k : switches) {
    const char* e = getenv(k.name);
    if (!e) continue;
    if (!e[0] || e[1] || !strchr(k.digits, e[0]))
      return fail(BA3C_ERR_INVALID, std::string(k.name) + "=" + e + ": expected one digit of " + k.digits);
    k.set(sw, e[0] - '0');
  }
  ba3c_handle* h = new ba3c_handle();
  h->cfg = c;
  h->sw = sw;
  h->band = h->g6 = !sw.generic;
  {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      h->cus = n;
  }

  const int F = c.fc_neurons, per = F / splits;
  h->per = per;
  int64_t off = 0;
  auto add = [&](const std::string& name, std::initializer_list<int> shape) {
    TensorDesc d;
    d.name = name;
    d.offset = off;
    d.ndim = (int)shape.size();
    int64_t n = 1;
    int i = 0;
    for (int v : shape) {
      d.shape[i++] = v;
      n *= v;
    }
    for (; i < 4; ++i) d.shape[i] = 0;
    d.numel = n;
    h->tensors.push_back(d);
    off = align64(off + n);
    return (int)h->tensors.size() - 1;
  };
  h->idx_conv[0] = add("conv0/W", {5, 5, 16, 32});
  h->idx_conv[1] = add("conv1/W", {5, 5, 32, 32});
  h->idx_conv[2] = add("conv2/W", {5, 5, 32, 64});
  h->idx_conv[3] = add("conv3/W", {3, 3, 64, 64});
  h->idx_fc1 = -1;
  for (int i = 0; i < splits; ++i) {
    int t;
    if (c.replace_with_conv) {
      t = add("fc1_" + std::to_string(i) + "/W", {5, 5, 64, per});
    } else {
      t = add("fc1_" + std::to_string(i) + "/W", {1600, per});
      add("fc1_" + std::to_string(i) + "/b", {per});
    }
    if (i == 0) h->idx_fc1 = t;
  }
  h->wstride = c.replace_with_conv ? 1600 * per : (int)(1600 * per + align64(per));
  h->idx_piW = add("fc-pi/W", {F, c.num_actions});
  h->idx_pib = add("fc-pi/b", {c.num_actions});
  h->idx_vW = add("fc-v/W", {F, 1});
  h->idx_vb = add("fc-v/b", {1});
  h->flat = off;
  if ((int)h->tensors.size() > MAXT) {
    delete h;
    return fail(BA3C_ERR_INVALID, "too many tensors");
  }
  TensorTable& tt = h->table;
  std::memset(&tt, 0, sizeof(tt));
  tt.n = (int)h->tensors.size();
  int ch = 0;
  for (int i = 0; i < tt.n; ++i) {
    tt.off[i] = h->tensors[i].offset;
    tt.numel[i] = (int)h->tensors[i].numel;
    tt.chunk0[i] = ch;
    ch += (int)((h->tensors[i].numel + UPD_CHUNK - 1) / UPD_CHUNK);
  }
  tt.chunk0[tt.n] = ch;
  tt.nchunks = ch;
  // clip_update_kernel's and clip_range_kernel's tagged partials + error words (no device:
  // stay null, two-launch paths)
  const size_t ubytes = ((size_t)tt.nchunks + 1) * sizeof(unsigned long long);
  const size_t cbytes = (4 * CHAIN_SITES + 4) * sizeof(unsigned);
  if (hipMalloc(reinterpret_cast<void**>(&h->utag), 2 * ubytes + cbytes) != hipSuccess) {
    h->utag = nullptr;
    (void)hipGetLastError();
  } else if (hipMemset(h->utag, 0, 2 * ubytes + cbytes) != hipSuccess) {
    (void)hipFree(h->utag);
    h->utag = nullptr;
    (void)hipGetLastError();
  } else {
    h->ctag = h->utag + tt.nchunks + 1;
    h->chain = reinterpret_cast<unsigned*>(h->ctag + tt.nchunks + 1);
  }
  *out = h;
  return BA3C_OK;
}

int ba3c_comm_destroy(ba3c_handle* h, int32_t abort);

void ba3c_destroy(ba3c_handle* h) {
  if (!h) return;
  if (h->comm) (void)ba3c_comm_destroy(h, 0);
  for (auto e : h->ev_begin) (void)hipEventDestroy(e);
  for (auto e : h->ev_end) (void)hipEventDestroy(e);
  for (auto e : h->ev_fork)
    if (e) (void)hipEventDestroy(e);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->side) (void)hipStreamDestroy(h->side);
  if (h->utag) (void)hipFree(h->utag);
  delete h;
}

int ba3c_num_tensors(const ba3c_handle* h) { return h ? (int)h->tensors.size() : 0; }

int ba3c_tensor_info(const ba3c_handle* h, int32_t i, const char** name, int64_t* offset,
                     int64_t* numel, int32_t shape[4], int32_t* ndim) {
  if (!h || i < 0 || i >= (int)h->tensors.size()) return fail(BA3C_ERR_INVALID, "bad tensor index");
  const TensorDesc& d = h->tensors[i];
  if (name) *name = d.name.c_str();
  if (offset) *offset = d.offset;
  if (numel) *numel = d.numel;
  if (shape)
    for (int k = 0; k < 4; ++k) shape[k] = d.shape[k];
  if (ndim) *ndim = d.ndim;
  return BA3C_OK;
}

int64_t ba3c_flat_size(const ba3c_handle* h) { return h ? h->flat : 0; }

int ba3c_workspace_tensor(const ba3c_handle* h, int32_t batch, int32_t train, const char* name,
                          int64_t* offset_bytes, int64_t* bytes) {
  if (!h || !name || batch < 1) return fail(BA3C_ERR_INVALID, "bad argument");
  Workspace w = carve(h, nullptr, batch, train != 0);
  // carve() with a null base returns offsets as pointers from 0
  const size_t Bz = (size_t)batch;
  const int F = h->cfg.fc_neurons;
  struct Item { const char* n; const void* p; size_t b; };
  const Item items[] = {
      {"p0", w.p0, Bz * P0 * 4}, {"p1", w.p1, Bz * P1 * 4}, {"p2", w.p2, Bz * P2 * 4},
      {"a3", w.a3, Bz * A3 * 4}, {"h", w.h, Bz * F * 4},     {"c0", w.c0, Bz * P0},
      {"c1", w.c1, Bz * P1},     {"c2", w.c2, Bz * P2},     {"dh", w.dh, Bz * F * 4},
      {"dy3", w.dy3, Bz * A3 * 4}, {"dp2", w.dp2, Bz * P2 * 4}, {"dp1", w.dp1, Bz * P1 * 4},
      {"dp0", w.dp0, Bz * P0 * 4}};
  for (const Item& it : items) {
    if (std::strcmp(it.n, name) == 0) {
      if (!train && it.n[0] != 'p' && it.n[0] != 'a' && it.n[0] != 'h')
        return fail(BA3C_ERR_INVALID, "tensor only exists in the training workspace");
      if (offset_bytes) *offset_bytes = (int64_t)reinterpret_cast<uintptr_t>(it.p);
      if (bytes) *bytes = (int64_t)it.b;
      return BA3C_OK;
    }
  }
  return fail(BA3C_ERR_INVALID, std::string("unknown workspace tensor ") + name);
}

size_t ba3c_workspace_size(const ba3c_handle* h, int32_t batch, int32_t train) {
  if (!h || batch < 1) return 0;
  return carve(h, nullptr, batch, train != 0).bytes;
}

int ba3c_forward(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                 int32_t batch, float explore_factor, void* workspace, float* probs,
                 float* probsT, float* value) {
  if (!h || !check_ptr(params) || !check_ptr(state) || !check_ptr(workspace))
    return fail(BA3C_ERR_INVALID, "null or misaligned pointer");
  if (batch < 1 || batch > h->cfg.max_batch) return fail(BA3C_ERR_INVALID, "batch out of range");
  hipStream_t s = static_cast<hipStream_t>(stream);
  Workspace w = carve(h, workspace, batch, false);
  std::memset(h->merged, 0, sizeof(h->merged));
  const LaunchPlan pl = plan_launches(h->sw, batch, h->cfg.channels, h->cus, false);
  int r = h->cfg.channels == 4 ? run_forward<4>(h, s, pl, params, state, batch, w, false)
                               : run_forward<12>(h, s, pl, params, state, batch, w, false);
  if (r != BA3C_OK) return r;
  return run_heads(h, s, params, w, batch, nullptr, nullptr, 0.f, explore_factor, false, probs,
                   probsT, value);
}

int ba3c_set_phase2_event(ba3c_handle* h, void* event) {
  if (!h) return fail(BA3C_ERR_INVALID, "null handle");
  h->ev_mid = static_cast<hipEvent_t>(event);
  return BA3C_OK;
}

int ba3c_bucket_tensor(const ba3c_handle* h) { return h ? h->idx_fc1 : -1; }

// ppo: the clipped-surrogate heads (ba3c_train_grads_ppo_ext); its rows stand in for futurereward
static int train_grads_impl(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                            const int64_t* action, const float* futurereward, int32_t batch,
                            float entropy_beta, void* workspace, float* grads, double* scalars,
                            int32_t phase, const PpoArgs* ppo = nullptr) {
  if (phase < 0 || phase > 2) return fail(BA3C_ERR_INVALID, "phase must be 0, 1 or 2");
  if (!h || !check_ptr(params) || !check_ptr(state) || !check_ptr(workspace) || !check_ptr(grads) ||
      !action || (!futurereward && !ppo))
    return fail(BA3C_ERR_INVALID, "null or misaligned pointer");
  if (batch < 1 || batch > h->cfg.max_batch) return fail(BA3C_ERR_INVALID, "batch out of range");
  hipStream_t s = static_cast<hipStream_t>(stream);
  CHECK(ensure_side_stream(h, s));
  Workspace w = carve(h, workspace, batch, true);
  // no memset of `grads`: the backward pass's single reduction launch writes every element
  // of every tensor (incl. conv0's zero-padded channels)
  const LaunchPlan pl = plan_launches(h->sw, batch, h->cfg.channels, h->cus, true);
  auto backward = [&] {
    return h->cfg.channels == 4 ? BackwardPass<4>(h, s, pl, w, params, state, grads, batch, phase).run()
                                : BackwardPass<12>(h, s, pl, w, params, state, grads, batch, phase).run();
  };
  if (phase == 2) return backward();   // conv layers' backward on the workspace phase 1 left
  std::memset(h->merged, 0, sizeof(h->merged));   // a new training pass
  // on the split path the weight-prep launch zeroes the ReLU counters
  if (!h->band) HIP_TRY(hipMemsetAsync(w.relu, 0, RELU_WORDS * 8, s));
  int r = h->cfg.channels == 4 ? run_forward<4>(h, s, pl, params, state, batch, w, true)
                               : run_forward<12>(h, s, pl, params, state, batch, w, true);
  if (r != BA3C_OK) return r;
  // heads + loss + its gradient, fc1's split-K finish and (last workgroup) the TfDictOp scalars
  h->pend_scalars = false;
  CHECK(run_heads(h, s, params, w, batch, action, futurereward, entropy_beta, 1.0f, true, nullptr,
                  nullptr, nullptr, scalars, phase != 2 && h->sw.scalars_ride && h->g6, ppo));
  return backward();
}

int ba3c_train_grads_phase(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                           const int64_t* action, const float* futurereward, int32_t batch,
                           float entropy_beta, void* workspace, float* grads, double* scalars,
                           int32_t phase) {
  return train_grads_impl(h, stream, params, state, action, futurereward, batch, entropy_beta, workspace,
                          grads, scalars, phase);
}

int ba3c_train_grads(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                     const int64_t* action, const float* futurereward, int32_t batch,
                     float entropy_beta, void* workspace, float* grads, double* scalars) {
  return ba3c_train_grads_phase(h, stream, params, state, action, futurereward, batch, entropy_beta,
                                workspace, grads, scalars, 0);
}

int ba3c_train_grads_ppo_ext(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                             const int64_t* action, const float* rows, int32_t batch,
                             float entropy_beta, float clip_eps, float vclip_eps, uint32_t flags,
                             void* workspace, float* grads, double* scalars, float* ratio,
                             int32_t phase) {
  if (!check_ptr(rows)) return fail(BA3C_ERR_INVALID, "rows must be non-null and 16-byte aligned");
  if (ratio && !check_ptr(ratio)) return fail(BA3C_ERR_INVALID, "ratio must be 16-byte aligned (or null)");
  // written so that a NaN fails them
  if (!(clip_eps > 0.f && clip_eps < 1.f)) return fail(BA3C_ERR_INVALID, "clip_eps must be in (0, 1)");
  if (!(vclip_eps >= 0.f && std::isfinite(vclip_eps)))
    return fail(BA3C_ERR_INVALID, "vclip_eps must be finite and >= 0 (0: no value clipping)");
  if (flags & ~BA3C_PPO_ADV_FROM_ROW) return fail(BA3C_ERR_INVALID, "unknown flags bits");
  static_assert(BA3C_PPO_ADV_FROM_ROW == PPO_ADV_FROM_ROW, "the header's bit is the kernel's");
  const PpoArgs ppo{rows, ratio, clip_eps, vclip_eps, flags};
  return train_grads_impl(h, stream, params, state, action, nullptr, batch, entropy_beta, workspace,
                          grads, scalars, phase, &ppo);
}

int ba3c_train_grads_ppo(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                         const int64_t* action, const float* rows, int32_t batch,
                         float entropy_beta, float clip_eps, void* workspace, float* grads,
                         double* scalars, float* ratio, int32_t phase) {
  return ba3c_train_grads_ppo_ext(h, stream, params, state, action, rows, batch, entropy_beta, clip_eps,
                                  0.f, 0, workspace, grads, scalars, ratio, phase);
}

int ba3c_ppo_norm_adv(void* stream, float* rows, int32_t n, double* stats) {
  if (!check_ptr(rows)) return fail(BA3C_ERR_INVALID, "rows must be non-null and 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(stats) & 7) return fail(BA3C_ERR_INVALID, "stats must be 8-byte aligned (or null)");
  if (n < 1) return fail(BA3C_ERR_INVALID, "bad count: n must be >= 1");
  hipLaunchKernelGGL(ppo_norm_adv_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<float4*>(rows), n, stats);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_clip_grads_range(ba3c_handle* h, void* stream, float* grads, void* workspace, int32_t t0,
                          int32_t t1) {
  if (!h || !check_ptr(grads) || !check_ptr(workspace)) return fail(BA3C_ERR_INVALID, "null pointer");
  if (t0 < 0 || t1 > h->table.n || t0 >= t1) return fail(BA3C_ERR_INVALID, "bad tensor range");
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = carve(h, workspace, 1, false).sumsq;
  const int c0 = h->table.chunk0[t0], nc = h->table.chunk0[t1] - c0;
  ProbeScope ps(h, s, BA3C_K_CLIP);
  if (h->ctag && h->sw.fused_update && nc <= h->cus) {
    // one launch (tagged partials), bit-identical to the two below
    const UpdateSync us{h->ctag, reinterpret_cast<unsigned int*>(h->ctag + h->table.nchunks)};
    hipLaunchKernelGGL(clip_range_kernel, dim3(nc), dim3(256), 0, s, grads, h->table, c0, us);
  } else {
    hipLaunchKernelGGL(sumsq_kernel, dim3(nc), dim3(256), 0, s, grads, h->table, part, c0);
    hipLaunchKernelGGL(clip_kernel, dim3(nc), dim3(256), 0, s, grads, h->table, (const float*)part, c0);
  }
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_clip_grads(ba3c_handle* h, void* stream, float* grads, void* workspace) {
  if (!h || !check_ptr(grads) || !check_ptr(workspace)) return fail(BA3C_ERR_INVALID, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = carve(h, workspace, 1, false).sumsq;  // batch-independent first region
  {
    ProbeScope ps(h, s, BA3C_K_CLIP);
    hipLaunchKernelGGL(sumsq_kernel, dim3(h->table.nchunks), dim3(256), 0, s, grads, h->table, part, 0);
    hipLaunchKernelGGL(clip_kernel, dim3(h->table.nchunks), dim3(256), 0, s, grads, h->table,
                       (const float*)part, 0);
  }
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int64_t ba3c_global_clip_scratch(const ba3c_handle* h) { return h ? (int64_t)h->table.nchunks + 2 : 0; }

int ba3c_clip_grads_global(ba3c_handle* h, void* stream, float* grads, double max_norm,
                           double* scratch, int64_t scratch_doubles) {
  if (!h) return fail(BA3C_ERR_INVALID, "null handle");
  if (!check_ptr(grads)) return fail(BA3C_ERR_INVALID, "grads must be non-null and 16-byte aligned");
  // written so that a NaN fails
  if (!(max_norm > 0.0 && std::isfinite(max_norm)))
    return fail(BA3C_ERR_INVALID, "max_norm must be finite and > 0");
  if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 7))
    return fail(BA3C_ERR_INVALID, "scratch must be non-null and 8-byte aligned");
  const int nc = h->table.nchunks;
  if (scratch_doubles < (int64_t)nc + 2)
    return fail(BA3C_ERR_INVALID, "scratch_doubles " + std::to_string((long long)scratch_doubles) +
                                      " is below nchunks + 2 = " + std::to_string(nc + 2));
  hipStream_t s = static_cast<hipStream_t>(stream);
  {
    ProbeScope ps(h, s, BA3C_K_CLIP);
    hipLaunchKernelGGL(gnorm_partials_kernel, dim3(nc), dim3(256), 0, s, (const float*)grads, h->table, scratch);
    hipLaunchKernelGGL(gnorm_scale_kernel, dim3(nc), dim3(256), 0, s, grads, h->table, scratch, max_norm);
  }
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

static int apply_update_impl(ba3c_handle* h, void* stream, int32_t opt, float* params,
                             const float* grads, float* slot0, float* slot1,
                             const ba3c_opt_params* hp, float* dev_powers, float grad_scale,
                             int32_t fuse_clip, void* workspace) {
  if (!h || !hp || !check_ptr(params) || !check_ptr(grads)) return fail(BA3C_ERR_INVALID, "null pointer");
  const bool need0 = opt != BA3C_OPT_GD, need1 = opt == BA3C_OPT_ADAM || opt == BA3C_OPT_RMS || opt == BA3C_OPT_ADADELTA;
  if ((need0 && !check_ptr(slot0)) || (need1 && !check_ptr(slot1)))
    return fail(BA3C_ERR_INVALID, "missing optimizer slot");
  if (fuse_clip && !check_ptr(workspace)) return fail(BA3C_ERR_INVALID, "fuse_clip needs a workspace");
  // validated before anything is launched
  if (opt < BA3C_OPT_ADAM || opt > BA3C_OPT_RMS) return fail(BA3C_ERR_INVALID, "unknown optimizer id");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UpdateArgs a{};
  a.p = params;
  a.g = grads;
  a.s0 = slot0;
  a.s1 = slot1;
  a.grad_scale = grad_scale;
  a.lr = hp->lr;
  // TF-1.2 float32 scalar arithmetic of ApplyAdam: alpha = lr*sqrt(1-b2^t)/(1-b1^t)
  a.alpha = dev_powers ? 0.f : adam_alpha(hp->lr, hp->beta1_power, hp->beta2_power);
  a.dev_powers = dev_powers;
  a.one_minus_b1 = 1.0f - hp->beta1;
  a.one_minus_b2 = 1.0f - hp->beta2;
  a.eps = hp->epsilon;
  a.decay_c = 1.0f - hp->decay;
  a.momentum = hp->momentum;
  a.rho = hp->rho;
  a.one_minus_rho = 1.0f - hp->rho;
  a.beta1 = hp->beta1;
  a.beta2 = hp->beta2;
  float* part = carve(h, workspace, 1, false).sumsq;  // batch-independent first region
  const bool fused = fuse_clip && h->sw.fused_update && h->utag && h->table.nchunks <= h->cus;
  if (fused) {
    a.clip_part = part;
    const dim3 grid(h->table.nchunks);
    const UpdateSync us{h->utag, reinterpret_cast<unsigned int*>(h->utag + h->table.nchunks)};
    {
      ProbeScope ps(h, s, BA3C_K_UPDATE);
      with_opt(opt, [&](auto O) {
        hipLaunchKernelGGL(clip_update_kernel<decltype(O)::value>, grid, dim3(256), 0, s, a, h->table, us);
        return BA3C_OK;
      });
    }
    HIP_TRY(hipGetLastError());
    return BA3C_OK;   // the Adam device powers advanced inside the launch
  }
  if (fuse_clip) {
    hipLaunchKernelGGL(sumsq_kernel, dim3(h->table.nchunks), dim3(256), 0, s, grads, h->table, part, 0);
    HIP_TRY(hipGetLastError());
    a.clip_part = part;
  }
  dim3 grid(h->table.nchunks);
  {
    ProbeScope ps(h, s, BA3C_K_UPDATE);
    with_opt(opt, [&](auto O) {
      hipLaunchKernelGGL(update_kernel<decltype(O)::value>, grid, dim3(256), 0, s, a, h->table);
      return BA3C_OK;
    });
  }
  HIP_TRY(hipGetLastError());
  if (opt == BA3C_OPT_ADAM && dev_powers) {
    hipLaunchKernelGGL(adam_powers_kernel, dim3(1), dim3(64), 0, s, dev_powers, hp->beta1, hp->beta2);
    HIP_TRY(hipGetLastError());
  }
  return BA3C_OK;
}

int ba3c_apply_update(ba3c_handle* h, void* stream, int32_t opt, float* params,
                      const float* grads, float* slot0, float* slot1, const ba3c_opt_params* hp,
                      float grad_scale, int32_t fuse_clip, void* workspace) {
  return apply_update_impl(h, stream, opt, params, grads, slot0, slot1, hp, nullptr, grad_scale,
                           fuse_clip, workspace);
}

int ba3c_apply_update_dev(ba3c_handle* h, void* stream, int32_t opt, float* params,
                          const float* grads, float* slot0, float* slot1,
                          const ba3c_opt_params* hp, float* dev_powers, float grad_scale,
                          int32_t fuse_clip, void* workspace) {
  if (opt == BA3C_OPT_ADAM && !check_ptr(dev_powers) && dev_powers == nullptr)
    return fail(BA3C_ERR_INVALID, "dev_powers required");
  return apply_update_impl(h, stream, opt, params, grads, slot0, slot1, hp, dev_powers, grad_scale,
                           fuse_clip, workspace);
}

int ba3c_sample(void* stream, const float* probs, const double* u, int32_t batch,
                int32_t num_actions, int64_t* actions, int32_t* nonfinite) {
  if (!probs || !u || !actions) return fail(BA3C_ERR_INVALID, "null pointer");
  if (batch < 0 || num_actions < 1 || num_actions >= MAXA) return fail(BA3C_ERR_INVALID, "bad shape");
  if (batch == 0) return BA3C_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sample_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, probs, u, batch,
                     num_actions, actions, nonfinite);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_sample_logp(void* stream, const float* probs, const float* pi, const double* u,
                     int32_t batch, int32_t num_actions, int64_t* actions, float* logp,
                     int32_t* nonfinite) {
  if (!probs || !u || !actions) return fail(BA3C_ERR_INVALID, "null pointer");
  if (!pi || !logp) return fail(BA3C_ERR_INVALID, "null pi or logp");
  if (batch < 0 || num_actions < 1 || num_actions >= MAXA) return fail(BA3C_ERR_INVALID, "bad shape");
  if (batch == 0) return BA3C_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sample_logp_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, probs, pi, u,
                     batch, num_actions, actions, logp, nonfinite);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_greedy(void* stream, const float* probs, const double* u, const int64_t* random_actions,
                int32_t batch, int32_t num_actions, double eps, int64_t* actions) {
  if (batch < 0 || num_actions < 1) return fail(BA3C_ERR_INVALID, "bad shape");
  if (batch == 0) return BA3C_OK;
  if (!probs || !u || !random_actions || !actions) return fail(BA3C_ERR_INVALID, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(greedy_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, probs, u, random_actions,
                     batch, num_actions, eps, actions);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_probe_enable(ba3c_handle* h, int32_t kernel_id) {
  if (!h) return fail(BA3C_ERR_INVALID, "null handle");
  if (kernel_id >= BA3C_NUM_KERNELS) return fail(BA3C_ERR_INVALID, "bad kernel id");
  if (h->ev_begin.empty() && kernel_id >= 0) {
    h->ev_begin.resize(4096);
    h->ev_end.resize(4096);
    // timestamps only: no system-scope fence (its L2 write-back + invalidate left a 5-6 us
    // gap around every probed launch, r06a trace)
    // (BA3C_EVENTS=torch: HIP's default events, the A/B of ba3c_amd/hipevent.py)
    const char* em = getenv("BA3C_EVENTS");
    const unsigned fl = (em && std::strcmp(em, "torch") == 0) ? hipEventDefault : hipEventDisableSystemFence;
    for (size_t i = 0; i < h->ev_begin.size(); ++i) {
      HIP_TRY(hipEventCreateWithFlags(&h->ev_begin[i], fl));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_end[i], fl));
    }
  }
  h->probe_kernel = kernel_id;
  h->probe_seen = 0;
  h->probe_used = 0;
  h->probe_ms = 0.0;
  h->probe_launches = 0;
  return BA3C_OK;
}

int ba3c_nstep_returns(void* stream, const double* reward, const float* value,
                       const int32_t* start, const int32_t* length, const uint8_t* is_over,
                       int32_t n_envs, int32_t slots, double gamma, float* R, int32_t* src,
                       float* init_R, uint8_t* over, int32_t* count) {
  if (!reward || !value || !start || !length || !is_over || !R || !src || !init_R || !over || !count)
    return fail(BA3C_ERR_INVALID, "null pointer");
  if (n_envs < 0 || slots < 1) return fail(BA3C_ERR_INVALID, "bad shape");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ReturnsArgs a{reward, value, start, length, is_over, n_envs, slots, gamma, R, src, init_R, over, count};
  hipLaunchKernelGGL(nstep_returns_kernel, dim3(1), dim3(1024), 0, s, a);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_lambda_returns(void* stream, const double* reward, const float* value,
                        const int32_t* start, const int32_t* length, const uint8_t* is_over,
                        int32_t n_envs, int32_t slots, double gamma, double lambda, float* R,
                        int32_t* src, float* init_R, uint8_t* over, int32_t* count) {
  if (!reward || !value || !start || !length || !is_over || !R || !src || !init_R || !over || !count)
    return fail(BA3C_ERR_INVALID, "null pointer");
  if (n_envs < 0 || slots < 1 || slots > kLambdaMaxSlots ||
      (int64_t)n_envs * slots > INT32_MAX)
    return fail(BA3C_ERR_INVALID, "bad shape (slots must be 1..129)");
  // written so that a NaN fails either test
  if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(BA3C_ERR_INVALID, "lambda must be in [0, 1]");
  if (!(gamma > 0.0 && gamma <= 1.0)) return fail(BA3C_ERR_INVALID, "gamma must be in (0, 1]");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ReturnsArgs a{reward, value, start, length, is_over, n_envs, slots, gamma, R, src, init_R, over, count};
  const int groups = std::max(1, (n_envs + kLambdaEnvs - 1) / kLambdaEnvs);   // n_envs == 0: *count = 0
  hipLaunchKernelGGL(lambda_returns_kernel, dim3(groups), dim3(256), 0, s, a, lambda);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_gather_rows(void* stream, const void* rows, const int32_t* idx, int32_t n,
                     int64_t row_bytes, void* out) {
  if (n < 0) return fail(BA3C_ERR_INVALID, "bad count");
  if (n == 0) return BA3C_OK;
  if (!rows || !idx || !out) return fail(BA3C_ERR_INVALID, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (row_bytes == 8) {
    hipLaunchKernelGGL(gather_i64_kernel, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, s,
                       static_cast<const int64_t*>(rows), idx, n, static_cast<int64_t*>(out));
  } else if (row_bytes > 0 && row_bytes % 16 == 0 && check_ptr(rows) && check_ptr(out)) {
    const int words = (int)(row_bytes / 16);
    const int gx = std::min(8, (words + 255) / 256);
    // gridDim.y is limited to 65535: the kernel folds the row index over it
    hipLaunchKernelGGL(gather_rows16_kernel, dim3(gx, std::min(n, 65535)), dim3(256), 0, s,
                       static_cast<const uint4*>(rows), idx, n, words, static_cast<uint4*>(out));
  } else {
    return fail(BA3C_ERR_INVALID, "row_bytes must be 8 or a multiple of 16 (16-byte aligned rows)");
  }
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_history_push(void* stream, const uint8_t* frame, uint8_t* state, const uint8_t* is_over,
                      int32_t n_envs, int32_t pixels, int32_t hist_len, int32_t channels) {
  if (!frame || !state) return fail(BA3C_ERR_INVALID, "null pointer");
  if (n_envs < 0 || pixels < 1 || hist_len < 1 || channels < 1) return fail(BA3C_ERR_INVALID, "bad shape");
  if (n_envs == 0) return BA3C_OK;
  if (hist_len * channels == 4 && channels == 1 && (!check_ptr(state) || (reinterpret_cast<uintptr_t>(frame) & 3)))
    return fail(BA3C_ERR_INVALID, "state must be 16-byte and frame 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  HistoryArgs a{frame, state, is_over, n_envs, pixels, hist_len, channels};
  const int groups = (pixels + 3) / 4;
  hipLaunchKernelGGL(history_push_kernel, dim3((groups + 255) / 256, n_envs), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_episode_stats(void* stream, const double* reward, const uint8_t* over, int32_t n_envs,
                       double* ret, int32_t* len, double* log_score, int32_t* log_len,
                       int32_t* log_env, int32_t cap, int64_t* head) {
  if (!reward || !over || !ret || !len || !log_score || !log_len || !log_env || !head)
    return fail(BA3C_ERR_INVALID, "null pointer (every buffer of the episode log is required)");
  if (n_envs < 1) return fail(BA3C_ERR_INVALID, "n_envs must be >= 1");
  if (cap < n_envs)
    return fail(BA3C_ERR_INVALID, "cap must be >= the simulators: one launch must not overwrite its own entries");
  auto off = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  if (off(reward, 8) || off(ret, 8) || off(log_score, 8) || off(head, 8) || off(len, 4) || off(log_len, 4) ||
      off(log_env, 4))
    return fail(BA3C_ERR_INVALID,
                "reward / ret / log_score / head must be 8-byte aligned, len / log_len / log_env 4-byte");
  const EpisodeArgs a{reward, over, n_envs, ret, len, log_score, log_len, log_env, cap, head};
  hipLaunchKernelGGL(episode_stats_kernel, dim3(1), dim3(kEpisodeThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_breakout_step(void* stream, int32_t* game, const int64_t* action, int32_t n_envs,
                       int32_t limit, double* reward, uint8_t* over, int32_t* ep_score,
                       uint8_t* frame, uint8_t* state) {
  return game_launch<SoloSim<BreakoutRules>>(stream, {game, action, limit, n_envs, reward, over, ep_score,
                                                      frame, state});
}

int ba3c_breakout_render(void* stream, const int32_t* game, int32_t n_envs, uint8_t* frame,
                         uint8_t* state) {
  return game_launch<SoloSim<BreakoutRules>>(stream, render_args(game, n_envs, frame, state), nullptr, true);
}

int ba3c_boxing_step(void* stream, int32_t* game, const int64_t* action, int32_t n_envs,
                     int32_t limit, double* reward, uint8_t* over, int32_t* ep_score,
                     uint8_t* frame, uint8_t* state) {
  return game_launch<SoloSim<BoxingRules>>(stream, {game, action, limit, n_envs, reward, over, ep_score,
                                                    frame, state});
}

// One decision of ba3c_amd/frameskip.py for every simulator.
int ba3c_breakout_step_skip(void* stream, int32_t* game, int32_t* aux, const int64_t* action, int32_t n_envs,
                            int32_t limit, int32_t skip_lo, int32_t skip_hi, int32_t sticky_q16,
                            double* reward, uint8_t* over, int32_t* ep_score, uint8_t* frame,
                            uint8_t* state) {
  const Decision d{aux, skip_lo, skip_hi, sticky_q16};
  return game_launch<SoloSim<BreakoutRules>>(stream, {game, action, limit, n_envs, reward, over, ep_score,
                                                      frame, state}, &d);
}

int ba3c_boxing_step_skip(void* stream, int32_t* game, int32_t* aux, const int64_t* action, int32_t n_envs,
                          int32_t limit, int32_t skip_lo, int32_t skip_hi, int32_t sticky_q16,
                          double* reward, uint8_t* over, int32_t* ep_score, uint8_t* frame,
                          uint8_t* state) {
  const Decision d{aux, skip_lo, skip_hi, sticky_q16};
  return game_launch<SoloSim<BoxingRules>>(stream, {game, action, limit, n_envs, reward, over, ep_score,
                                                    frame, state}, &d);
}

int ba3c_boxing_render(void* stream, const int32_t* game, int32_t n_envs, uint8_t* frame,
                       uint8_t* state) {
  return game_launch<SoloSim<BoxingRules>>(stream, render_args(game, n_envs, frame, state), nullptr, true);
}

int ba3c_boxing_duel_step(void* stream, int32_t* game, const int64_t* action, int32_t n_games, int32_t limit,
                          double* reward, uint8_t* over, int32_t* ep_score, uint8_t* frame, uint8_t* state) {
  return game_launch<DuelSim>(stream, {game, action, limit, n_games, reward, over, ep_score, frame, state});
}

// One decision of ba3c_amd/duel.py (decide_numpy) for every game.
int ba3c_boxing_duel_decide(void* stream, int32_t* game, int32_t* aux, const int64_t* action, int32_t n_games,
                            int32_t limit, int32_t skip_lo, int32_t skip_hi, int32_t sticky_q16,
                            int32_t start_lo, int32_t start_hi, double* reward, uint8_t* over,
                            int32_t* ep_score, uint8_t* frame, uint8_t* state) {
  const Decision d{aux, skip_lo, skip_hi, sticky_q16, start_lo, start_hi};
  return game_launch<DuelSim>(stream, {game, action, limit, n_games, reward, over, ep_score, frame, state}, &d);
}

int ba3c_boxing_duel_render(void* stream, const int32_t* game, int32_t n_games, uint8_t* frame,
                            uint8_t* state) {
  return game_launch<DuelSim>(stream, render_args(game, n_games, frame, state), nullptr, true);
}

int ba3c_breakout_view(void* stream, const int32_t* game, int32_t n_envs, const int32_t* sel, int32_t n_sel,
                       const uint8_t* palette, const uint8_t* hud, int32_t scale, uint8_t* out) {
  return env_view<BreakoutRules>(stream, game, n_envs, sel, n_sel, palette, hud, scale, out);
}

int ba3c_boxing_view(void* stream, const int32_t* game, int32_t n_envs, const int32_t* sel, int32_t n_sel,
                     const uint8_t* palette, const uint8_t* hud, int32_t scale, uint8_t* out) {
  return env_view<BoxingRules>(stream, game, n_envs, sel, n_sel, palette, hud, scale, out);
}

int ba3c_kernel_split(const ba3c_handle* h, int32_t kid) {
  if (!h || kid < 0 || kid >= BA3C_NUM_KERNELS) return -1;
  const bool c4 = h->cfg.channels == 4;
  switch (kid) {
    case BA3C_K_CONV0_FWD:
    case BA3C_K_CONV0_WGRAD: return (h->band && c4) ? 2 : (h->g6 ? 6 : 1);
    case BA3C_K_CONV1_FWD:
    case BA3C_K_CONV2_FWD:
    case BA3C_K_CONV1_DGRAD:
    case BA3C_K_CONV2_DGRAD:
    case BA3C_K_CONV1_WGRAD:
    case BA3C_K_CONV2_WGRAD: return h->band ? 3 : 1;
    // conv3: whole-image fp16x3 kernels (ba3c_conv3.h)
    case BA3C_K_CONV3_FWD:
    case BA3C_K_CONV3_DGRAD:
    case BA3C_K_CONV3_WGRAD: return h->band ? 3 : (h->g6 ? 6 : 1);
    case BA3C_K_FC1_FWD:
    case BA3C_K_FC1_DGRAD:
    case BA3C_K_FC1_WGRAD:
    case BA3C_K_HEAD_WGRAD: return h->g6 ? 6 : 1;
    case BA3C_K_HEADS:
    case BA3C_K_WGRAD_REDUCE:
    case BA3C_K_CLIP:
    case BA3C_K_UPDATE: return 0;
    default: return 1;
  }
}

int ba3c_kernel_merged(const ba3c_handle* h, int32_t kid) {
  if (!h || kid < 0 || kid >= BA3C_NUM_KERNELS) return -1;
  return (int)h->merged[kid];
}

int ba3c_kernel_family(const ba3c_handle* h, int32_t kid) {
  if (!h || kid < 0 || kid >= BA3C_NUM_KERNELS) return -1;
  const int sp = ba3c_kernel_split(h, kid);
  if (sp <= 1) return sp;
  const bool band_split = kid == BA3C_K_CONV0_FWD || kid == BA3C_K_CONV0_WGRAD || kid == BA3C_K_CONV1_FWD ||
                          kid == BA3C_K_CONV2_FWD || kid == BA3C_K_CONV1_DGRAD || kid == BA3C_K_CONV2_DGRAD ||
                          kid == BA3C_K_CONV1_WGRAD || kid == BA3C_K_CONV2_WGRAD ||
                          kid == BA3C_K_CONV3_FWD || kid == BA3C_K_CONV3_DGRAD || kid == BA3C_K_CONV3_WGRAD;
  if (kid == BA3C_K_CONV0_FWD || kid == BA3C_K_CONV0_WGRAD)
    if (!(h->band && h->cfg.channels == 4)) return 3;
  return band_split ? 2 : 3;
}

int ba3c_device_errors(ba3c_handle* h, uint32_t* flags) {
  if (!h || !flags) return fail(BA3C_ERR_INVALID, "null argument");
  *flags = 0;
  if (!h->utag) return BA3C_OK;
  // every stream, the non-blocking ones torch creates included (a null-stream copy does not
  // wait for those)
  HIP_TRY(hipDeviceSynchronize());
  uint32_t e = 0, e2 = 0, e3 = 0;
  HIP_TRY(hipMemcpy(&e, h->utag + h->table.nchunks, sizeof(e), hipMemcpyDeviceToHost));
  if (h->ctag) HIP_TRY(hipMemcpy(&e2, h->ctag + h->table.nchunks, sizeof(e2), hipMemcpyDeviceToHost));
  if (h->chain) HIP_TRY(hipMemcpy(&e3, h->chain + 4 * CHAIN_SITES, sizeof(e3), hipMemcpyDeviceToHost));
  if (e3 && h->sw.chain) {
    // a chained wait gave up: a late signal may have landed after the last waiter reset the
    // site's words, so they can no longer be trusted.  Zero them from the host and stop
    // chaining on this handle (the error bit stays set)
    h->sw.chain = false;
    HIP_TRY(hipMemset(h->chain, 0, 4 * CHAIN_SITES * sizeof(unsigned)));
  }
  *flags = e | (e2 << 1) | (e3 << 2);
  return BA3C_OK;
}

int ba3c_occupy_cus(void* stream, int32_t n_cus, double usec) {
  if (n_cus < 0 || n_cus > 4096 || !(usec >= 0.0) || usec > 1e6)
    return fail(BA3C_ERR_INVALID, "n_cus in [0, 4096], usec in [0, 1e6]");
  if (n_cus == 0 || usec == 0.0) return BA3C_OK;
  hipLaunchKernelGGL(occupy_kernel, dim3(n_cus), dim3(64), 0, static_cast<hipStream_t>(stream),
                     (unsigned long long)(usec * 100.0));   // 100 MHz realtime clock
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

// ---- gradient exchange through the C ABI ----------
// RCCL is resolved at run time from the library already loaded in the process (torch's copy,
// or /opt/rocm's librccl.so.1 for a caller without torch): both carry the soname
// librccl.so.1, so one RCCL serves torch.distributed and these entry points.

int ba3c_comm_unique_id(void* id_out) {
  if (!id_out) return fail(BA3C_ERR_INVALID, "null argument");
  if (!rccl().ok) return fail(BA3C_ERR_HIP, "RCCL (librccl.so.1) not found");
  ncclUniqueId id;
  const ncclResult_t e = rccl().get_unique_id(&id);
  if (e != ncclSuccess) return rccl_fail(e, "ncclGetUniqueId");
  std::memcpy(id_out, &id, sizeof(id));
  return BA3C_OK;
}

int ba3c_comm_init(ba3c_handle* h, const void* id, int32_t nranks, int32_t rank) {
  if (!h || !id) return fail(BA3C_ERR_INVALID, "null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(BA3C_ERR_INVALID, "bad rank / rank count");
  if (h->comm) return fail(BA3C_ERR_INVALID, "the handle already has a communicator");
  if (!rccl().ok) return fail(BA3C_ERR_HIP, "RCCL (librccl.so.1) not found");
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  const ncclResult_t e = rccl().init_rank(&h->comm, nranks, uid, rank);
  if (e != ncclSuccess) {
    h->comm = nullptr;
    return rccl_fail(e, "ncclCommInitRank");
  }
  h->comm_ranks = nranks;
  return BA3C_OK;
}

int ba3c_comm_destroy(ba3c_handle* h, int32_t abort) {
  if (!h) return fail(BA3C_ERR_INVALID, "null handle");
  if (!h->comm) return BA3C_OK;
  const ncclResult_t e = abort ? rccl().abort(h->comm) : rccl().destroy(h->comm);
  h->comm = nullptr;
  h->comm_ranks = 0;
  if (e != ncclSuccess) return rccl_fail(e, abort ? "ncclCommAbort" : "ncclCommDestroy");
  return BA3C_OK;
}

int ba3c_allreduce_sum(ba3c_handle* h, void* stream, float* buf, int64_t count) {
  if (!h || !buf || count < 0) return fail(BA3C_ERR_INVALID, "bad argument");
  if (!h->comm) return fail(BA3C_ERR_INVALID, "no communicator (ba3c_comm_init)");
  const ncclResult_t e = rccl().all_reduce(buf, buf, (size_t)count, ncclFloat32, ncclSum, h->comm,
                                           static_cast<hipStream_t>(stream));
  if (e != ncclSuccess) return rccl_fail(e, "ncclAllReduce");
  return BA3C_OK;
}

int ba3c_allreduce_mean(ba3c_handle* h, void* stream, float* grads, int64_t count) {
  if (!check_ptr(grads)) return fail(BA3C_ERR_INVALID, "null or misaligned pointer");
  CHECK(ba3c_allreduce_sum(h, stream, grads, count));
  if (h->comm_ranks == 1 || count == 0) return BA3C_OK;   // x / 1 == x
  const float inv = 1.0f / (float)h->comm_ranks;
  hipLaunchKernelGGL(scale_kernel, dim3((unsigned)std::min<int64_t>((count + 1023) / 1024, 4096)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), grads, count, inv);
  HIP_TRY(hipGetLastError());
  return BA3C_OK;
}

int ba3c_probe_every(ba3c_handle* h, int32_t n) {
  if (!h) return fail(BA3C_ERR_INVALID, "null handle");
  if (n < 1) return fail(BA3C_ERR_INVALID, "probe interval must be >= 1");
  h->probe_every = n;
  h->probe_seen = 0;
  return BA3C_OK;
}

int ba3c_probe_read(ba3c_handle* h, double* total_ms, int32_t* launches) {
  if (!h) return fail(BA3C_ERR_INVALID, "null handle");
  for (int i = 0; i < h->probe_used; ++i) {
    HIP_TRY(hipEventSynchronize(h->ev_end[i]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev_begin[i], h->ev_end[i]));
    h->probe_ms += ms;
    h->probe_launches++;
  }
  h->probe_used = 0;
  if (total_ms) *total_ms = h->probe_ms;
  if (launches) *launches = h->probe_launches;
  return BA3C_OK;
}

}  // extern "C"
