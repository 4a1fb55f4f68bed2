// plan_table — the launch plan (csrc/ba3c_plan.h) on the host, for tests/test_launch_plan.py.
//   plan_table B:C:CUS:TRAIN:generic,c1pair,scalars_ride,overlap,multi,multi_big,fused_update,ring,chain,fwd01 ...
//     one line of key=value per argument: the plan of that batch, channel count, CU count and
//     switch setting
//   plan_table invariants | invariants-sparse
//     every B in 1..16384 (sparse: every 7th, for the sanitizer build), CUS in {64, 256, 304}, C
//     in {4, 12} and every switch combination: prints "invariants ok <plans checked>", or the
//     first violations and exits 1
#include <cstdio>
#include <cstring>

#include "ba3c_plan.h"

using namespace ba3c;

static const char* wgrad_name(Conv1Wgrad k) {
  switch (k) {
    case Conv1Wgrad::gemm: return "gemm";
    case Conv1Wgrad::wgrad6: return "wgrad6";
    case Conv1Wgrad::whole: return "whole";
    default: return "pair0";
  }
}

static void print_plan(int B, int C, int cus, const LaunchPlan& p) {
  std::printf(
      "B=%d C=%d cus=%d split=%d prep_multi=%d ring_fwd=%d fwd01=%d conv2_small=%d big=%d mj=%d mj_fc=%d "
      "fc1_big_tiles=%d mj_c2=%d side_stream=%d ring_dgrad=%d conv1_wgrad=%s conv1_slabs=%d conv0_slabs=%d "
      "conv3_slabs=%d pair_geometry=%d ring_batch=%d\n",
      B, C, cus, p.split, p.prep_multi, p.ring_fwd, p.fwd01, p.conv2_small, p.big, p.mj, p.mj_fc, p.fc1_big_tiles,
      p.mj_c2, p.side_stream, p.ring_dgrad, wgrad_name(p.conv1_wgrad), p.conv1_slabs, p.conv0_slabs, p.conv3_slabs,
      conv1_pair_geometry(B, cus), ring_batch(B, cus));
}

static int violations = 0;
static void expect(bool ok, const char* what, int B, int C, int cus, const Switches& s) {
  if (ok) return;
  if (++violations <= 20)
    std::printf("VIOLATION %s: B=%d C=%d cus=%d switches=%d,%d,%d,%d,%d,%d,%d,%d,%d,%d\n", what, B, C, cus, s.generic,
                s.c1pair, s.scalars_ride, s.overlap, s.multi, s.multi_big, s.fused_update, s.ring, s.chain, s.fwd01);
}

template <int STEP>
static int invariants() {
  long long checked = 0;
  const int cus_list[] = {64, 256, 304}, c_list[] = {4, 12}, c1pair_list[] = {0, 2};
  for (int cus : cus_list)
    for (int C : c_list)
      for (int B = 1; B <= 16384; B += STEP) {
        const LaunchPlan d = plan_launches(Switches{}, B, C, cus, true);
        for (int code = 0; code < 3072; ++code) {
          int c = code;
          auto take = [&c](int n) { const int v = c % n; c /= n; return v; };
          Switches s;
          s.generic = take(2);
          s.c1pair = c1pair_list[take(2)];
          s.scalars_ride = take(2);
          s.overlap = take(3);
          s.multi = take(2);
          s.multi_big = take(4);
          s.fused_update = take(2);
          s.ring = take(2);
          s.chain = take(2);
          s.fwd01 = take(2);
          const LaunchPlan p = plan_launches(s, B, C, cus, true);
          ++checked;
          expect(!p.fwd01 || p.ring_fwd, "fwd01 without ring_fwd", B, C, cus, s);
          expect(p.conv1_wgrad != Conv1Wgrad::pair0 || conv1_pair_geometry(B, cus), "pair outside the pair geometry", B,
                 C, cus, s);
          // what keeps every launch path bit-identical: the slabs summed never depend on a switch
          expect(p.conv1_slabs == d.conv1_slabs && p.conv0_slabs == d.conv0_slabs && p.conv3_slabs == d.conv3_slabs,
                 "slab count depends on a switch", B, C, cus, s);
          // the workspace is carved for these bounds
          expect(p.conv1_slabs >= 1 && p.conv1_slabs <= WG_P1, "conv1 slabs out of [1, WG_P1]", B, C, cus, s);
          expect(p.conv0_slabs >= (C == 4 ? 1 : 0) && p.conv0_slabs <= WG_P0S, "conv0 slabs out of range", B, C, cus, s);
          expect(p.conv3_slabs >= 1 && p.conv3_slabs <= C3W_P, "conv3 slabs out of [1, C3W_P]", B, C, cus, s);
          // a pair launch gives conv1 and conv0 one workgroup per CU each
          expect(p.conv1_wgrad != Conv1Wgrad::pair0 || (p.conv1_slabs == cus && p.conv0_slabs == cus),
                 "pair without one slab per CU", B, C, cus, s);
          // one-launch pairs run on the main stream; the 128 x 128 fc1 tiles are a job geometry
          expect(!(p.mj && p.side_stream), "mj with the side stream", B, C, cus, s);
          expect(!p.fc1_big_tiles || p.mj_fc, "fc1_big_tiles without mj_fc", B, C, cus, s);
          expect(!(p.mj && p.mj_c2), "mj and mj_c2", B, C, cus, s);
          // the fp32 engine takes nothing of the split path
          expect(p.split == !s.generic, "split", B, C, cus, s);
          expect(p.split || (!p.prep_multi && !p.ring_fwd && !p.fwd01 && !p.conv2_small && !p.mj && !p.mj_fc &&
                             !p.fc1_big_tiles && !p.mj_c2 && !p.ring_dgrad && p.conv1_wgrad == Conv1Wgrad::gemm),
                 "split-path decision on the generic engine", B, C, cus, s);
          expect(p.split == (p.conv1_wgrad != Conv1Wgrad::gemm), "conv1_wgrad", B, C, cus, s);
          // an inference plan is the training plan's forward
          const LaunchPlan f = plan_launches(s, B, C, cus, false);
          expect(f.prep_multi == p.prep_multi && f.ring_fwd == p.ring_fwd && f.fwd01 == p.fwd01 &&
                     f.conv2_small == p.conv2_small && f.split == p.split,
                 "forward differs between inference and training", B, C, cus, s);
        }
      }
  if (violations) {
    std::printf("%d violations\n", violations);
    return 1;
  }
  std::printf("invariants ok %lld\n", checked);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "invariants") == 0) return invariants<1>();
  if (argc == 2 && std::strcmp(argv[1], "invariants-sparse") == 0) return invariants<7>();
  if (argc < 2) {
    std::fprintf(stderr, "usage: plan_table invariants | invariants-sparse | plan_table B:C:CUS:TRAIN:<10 switch values> ...\n");
    return 2;
  }
  for (int i = 1; i < argc; ++i) {
    int B, C, cus, train, v[10];
    if (std::sscanf(argv[i], "%d:%d:%d:%d:%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", &B, &C, &cus, &train, &v[0], &v[1], &v[2],
                    &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9]) != 14) {
      std::fprintf(stderr, "bad argument %s\n", argv[i]);
      return 2;
    }
    Switches s;
    s.generic = v[0];
    s.c1pair = v[1];
    s.scalars_ride = v[2];
    s.overlap = v[3];
    s.multi = v[4];
    s.multi_big = v[5];
    s.fused_update = v[6];
    s.ring = v[7];
    s.chain = v[8];
    s.fwd01 = v[9];
    print_plan(B, C, cus, plan_launches(s, B, C, cus, train != 0));
  }
  return 0;
}
