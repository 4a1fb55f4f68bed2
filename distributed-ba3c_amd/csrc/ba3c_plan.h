// ba3c_plan.h — the launch structure of one step, decided once: which kernels run as one launch,
// on which stream, at which geometry and over how many partial slabs.  Plain C++ (no HIP, no
// handle, no layout template), so the table is testable on the host (tests/plan_table.cpp).
// This is the one place a launch-structure batch switch point is defined: run_forward,
// BackwardPass and launch_band6 (ba3c_capi.hip) read the LaunchPlan and compare no batch with a
// threshold themselves.
#pragma once
#include <algorithm>

namespace ba3c {

// ---- batch thresholds and slab counts ---------------------------------------------------
// Layout numbers are plain ints here; ba3c_capi.hip static_asserts them against its templates.
constexpr int SMALL_B = 128;     // conv2 forward / input gradient in 2- / 3-row bands up to here
constexpr int OVERLAP_B = 128;   // default side-stream / one-launch backward pairs up to this batch
static_assert(OVERLAP_B <= SMALL_B, "multi-job conv2 input gradient is the small-batch geometry");
// persistent grid bound of conv1's partial slabs
constexpr int WG_P1 = 512;
constexpr int W6_P1 = 256, W6_P2 = 128;   // x (c-groups x o-groups) = 512 workgroups
constexpr int W1_NBANDS = 9;     // bands per image of conv1's weight gradient (Lay::W1)
constexpr int C0F_NBANDS = 5;    // ... of conv0's forward (Conv0S)
constexpr int C0W_NBANDS = 10;   // ... of conv0's weight gradient (Conv0W)
// conv1 weight-gradient workgroups: ~4 bands each, at least 64 (at B=32 one band per
// workgroup made 256 partial slabs of 100 KB — 26 MB written and read back by the reduction
// for 3.3 MB of input).  A function of B alone, so every launch path sums the same slabs.
#ifndef BA3C_C1W_BPW
#define BA3C_C1W_BPW 3        // conv1 weight-gradient bands per workgroup below the ring sizes (r03: 4 -> 3, B=32 0.1966 -> 0.1925 ms)
#endif
inline int conv1_wgrad_p(int B) { return std::max(64, std::min(W6_P1, B * W1_NBANDS / BA3C_C1W_BPW)); }
// conv1 weight gradient with all 32 input channels per workgroup (wgrad6w_kernel) from this
// batch on: whole images per workgroup, two workgroups per CU, one slab each
constexpr int W6W_MIN_B = 512, W6W_P = 512;
static_assert(W6W_P <= WG_P1, "conv1 partial slabs: the allocation covers WG_P1 slabs");
// its slab count: one per CU (whole images, B / CUs each) where conv0's weight gradient can run
// beside it in one launch, else up to W6W_P; a function of B and the CU count alone, so the
// paired and the separate launches sum the same slabs bit for bit
inline bool conv1_pair_geometry(int B, int cus) { return B >= 2 * W6W_MIN_B && B % cus == 0 && cus <= WG_P1; }
inline int conv1_w6w_p(int B, int cus) { return conv1_pair_geometry(B, cus) ? cus : std::min(W6W_P, B); }
constexpr int FW_P0S = 512;   // conv0s_fwd_kernel: persistent, two workgroups per CU
inline int conv0_fwd_p(int B) { return std::min(FW_P0S, B * C0F_NBANDS); }
constexpr int C3W_P = 256;    // conv3_wgrad_kernel: one 512-thread workgroup (and slab) per CU, at most
inline int conv3_wgrad_p(int B, int cus) { return std::min(B, std::min(C3W_P, cus)); }
constexpr int WG_P0S = 512;   // conv0s_wgrad_kernel: 52 KB LDS, two workgroups per CU
// conv0's slab count: one per CU where conv1's weight gradient can share the launch (on every
// launch path, so they all sum the same slabs), else up to WG_P0S
inline int conv0_wgrad_p(int B, int cus) {
  return conv1_pair_geometry(B, cus) ? cus : std::min(WG_P0S, B * C0W_NBANDS);
}
// conv1's slab count on the split path, whichever kernel and launch computes them
inline int conv1_slab_count(int B, int cus) {
  return B >= W6W_MIN_B ? conv1_w6w_p(B, cus) : std::min(conv1_wgrad_p(B), B * W1_NBANDS);
}
// batches at which the ring-walk persistent kernels run (conv1's forward and input gradient;
// the fused conv0 -> conv1 forward): whole images per workgroup, only where they split
// (nearly) evenly over 2 x CUs workgroups
inline bool ring_batch(int B, int cus) {
  const int pr = 2 * cus;
  return B >= pr && (B % pr == 0 || B >= 8 * pr);
}

// ---- the launch-structure switches ba3c_create parses (defaults) --------------
struct Switches {
  // BA3C_GENERIC=1: every convolution and GEMM on the fp32-MFMA GEMM engine (a parity
  // configuration with exact fp32 products) instead of the split-MFMA kernels
  bool generic = false;
  // BA3C_C1PAIR: at the pair geometry conv1's weight gradient shares a launch with conv0's
  // (2, default) or runs alone (0)
  int c1pair = 2;
  // BA3C_SCALARS_RIDE: the large-batch scalar reduction deferred from the heads onto conv3's
  // input-gradient launch as one extra workgroup (default; r04 same-box A/B: step 1.954 ->
  // 1.935 ms).  0: its own launch after the heads
  bool scalars_ride = true;
  // BA3C_OVERLAP: backward weight gradients on a side stream: 0 never, 1 always, 2 (default)
  // for batches <= OVERLAP_B only.  Large batches: r01t/u measured +0.5% step throughput (561k
  // vs 557k samples/s) because conv1's dgrad and wgrad kernels each fill the chip, and
  // concurrent kernels make the per-kernel durations (roofline, rocprof) meaningless.  Small
  // batches: each backward kernel is a few latency-bound workgroups, so the weight-gradient
  // chain runs in the input-gradient chain's shadow.
  int overlap = 2;
  // BA3C_MULTI: batches <= OVERLAP_B on the split path (C == 4): each layer's input- and
  // weight-gradient kernels, and the weight prep beside conv0's forward, as ONE multi-job
  // launch (ba3c_multi.h) on the main stream instead of on two streams joined by events (r02k
  // trace at B=32: 6-11 us of idle queue per fork / join).  0: side stream as before.
  bool multi = true;
  // BA3C_MULTI_BIG bits: backward pairs as multi-job launches at batches > OVERLAP_B too: 1 fc1
  // + heads — r02x at B=2048, 84 -> 64 us for the three products; 2 conv2 — r02aa, 300 -> 292 us.
  // conv3's pair measured slower there (116 -> 134 us), and conv1's products stay on their
  // own (the dominant kernel's roofline probe needs conv1 dgrad alone).
  int multi_big = 3;
  // BA3C_FUSED_UPDATE: fused-clip optimizer applies as one clip_update_kernel launch
  // (ba3c_small.h) when the chunk count fits one workgroup per CU.  0: sumsq_kernel + update_kernel.
  bool fused_update = true;
  // BA3C_RING: conv1 fwd / dgrad as ring-walk persistent kernels at the ring batches
  // (conv_band6r_kernel).  0: one band per workgroup
  bool ring = true;
  // BA3C_CHAIN: chained multi-job launches (ba3c_multi.h: an in-launch dependency instead of a
  // kernel boundary) where the handle has their device words.  0: unchained
  bool chain = true;
  // BA3C_FWD01: at the ring batches (C == 4) conv0's forward and conv1's ring walk as one
  // persistent launch, each workgroup taking its own images through both layers (fwd01_kernel,
  // ba3c_conv0.hip).  0: the two launches
  bool fwd01 = true;
};

// how conv1's weight gradient runs
enum class Conv1Wgrad {
  gemm,     // the fp32 GEMM engine (BA3C_GENERIC)
  wgrad6,   // channel-group bands (wgrad6_kernel; a job of the input gradient's launch under `mj`)
  whole,    // whole-channel kernel alone (wgrad6w_kernel)
  pair0,    // whole-channel kernel beside conv0's weight gradient, one launch (wgrad01_pair_kernel)
};

struct LaunchPlan {
  bool split = true;   // split-MFMA kernels; false: the fp32 GEMM engine, nothing below but side_stream
  // forward
  bool prep_multi = false;    // weight prep beside conv0's forward (one launch, chained if available)
  bool ring_fwd = false;      // conv1's forward as the ring walk
  bool fwd01 = false;         // conv0's forward + conv1's ring walk as one persistent launch
  bool conv2_small = false;   // conv2 forward / input gradient in the small-batch band geometry
  // backward
  bool big = false;           // B > OVERLAP_B: full grids (2-deep k-tile rings; the scalars ride on conv3)
  bool mj = false;            // conv3 / conv2 / conv1: input + weight gradient as one launch each
  bool mj_fc = false;         // fc1 input gradient + fc1 and head weight gradients as one launch
  bool fc1_big_tiles = false; // ... on 128 x 128 tiles with fewer, longer K slabs
  bool mj_c2 = false;         // large batches: conv2's pair as one launch (whole-map geometry)
  bool side_stream = false;   // weight gradients on the side stream, where the handle has one
  bool ring_dgrad = false;    // conv1's input gradient as the ring walk
  Conv1Wgrad conv1_wgrad = Conv1Wgrad::gemm;
  // partial slabs of the split path's weight gradients: functions of (B, CUs, C) alone, so
  // every launch structure sums the same slabs bit for bit (conv0: C == 4 only)
  int conv1_slabs = 0, conv0_slabs = 0, conv3_slabs = 0;
};

inline LaunchPlan plan_launches(const Switches& sw, int B, int channels, int cus, bool train) {
  LaunchPlan p;
  p.split = !sw.generic;
  const bool c4 = channels == 4, small = B <= OVERLAP_B, ring = p.split && sw.ring && ring_batch(B, cus);
  p.prep_multi = p.split && sw.multi && small && c4;
  p.ring_fwd = ring;
  p.fwd01 = ring && c4 && !p.prep_multi && sw.fwd01;
  p.conv2_small = p.split && B <= SMALL_B;
  if (!train) return p;
  const bool mjok = p.split && sw.multi && sw.overlap != 1 && c4;
  p.big = !small;
  p.mj = mjok && small;
  p.mj_fc = p.mj || (mjok && (sw.multi_big & 1));
  p.fc1_big_tiles = p.mj_fc && p.big;
  p.mj_c2 = !p.mj && mjok && (sw.multi_big & 2);
  p.side_stream = !p.mj && (sw.overlap == 1 || (sw.overlap == 2 && small));
  p.ring_dgrad = ring;
  // the pair follows the BA3C_RING switch and the pair geometry, not whether the ring walk runs
  // at this batch (256 CUs, B = 1280: the pair, and the input gradient on one-band kernels)
  if (!p.split) p.conv1_wgrad = Conv1Wgrad::gemm;
  else if (sw.ring && conv1_pair_geometry(B, cus) && sw.c1pair == 2 && c4) p.conv1_wgrad = Conv1Wgrad::pair0;
  else if (B >= W6W_MIN_B) p.conv1_wgrad = Conv1Wgrad::whole;
  else p.conv1_wgrad = Conv1Wgrad::wgrad6;
  p.conv1_slabs = conv1_slab_count(B, cus);
  p.conv0_slabs = c4 ? conv0_wgrad_p(B, cus) : 0;
  p.conv3_slabs = conv3_wgrad_p(B, cus);
  return p;
}

}  // namespace ba3c
