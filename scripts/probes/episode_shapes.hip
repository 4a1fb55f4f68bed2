// A/B of the two kernel shapes for ba3c_episode_stats: the shipped single
// workgroup with a carry against one workgroup of 1024 threads per 4096 simulators that re-sums the
// flags before it, as ba3c_lambda_returns does.  The second shape reads `head` from one buffer and
// writes it to another, alternating: with the entry point's single `head` its write would race the
// other workgroups' reads.  Both log identical rings first; then µs per launch, medians of 20
// event-bracketed batches of 20 launches, alternating, at 100, 4096 and 65536 simulators.
// Not linked into libba3c.  Build: hipcc --offload-arch=gfx950 -O3 episode_shapes.hip -o episode_shapes
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../distributed-ba3c_amd/csrc/ba3c_episodes.h"

using namespace ba3c;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

__global__ void __launch_bounds__(kEpisodeThreads) multi_kernel(const EpisodeArgs a, const int64_t* head_in,
                                                                int64_t* head_out) {
  __shared__ int32_t wave_total[kEpisodeUnroll][kEpisodeWaves];
  __shared__ int32_t before_w[kEpisodeWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t first = (int64_t)blockIdx.x * kEpisodeChunk;
  int cnt = 0;
  for (int64_t base = 0; base < first; base += kEpisodeThreads) {      // first is a multiple of 1024
    const unsigned long long m = __ballot(a.over[base + tid] != 0);
    cnt += __popcll(m);
  }
  if (lane == 0) before_w[wave] = cnt;
  double r[kEpisodeUnroll]; int32_t l[kEpisodeUnroll]; bool o[kEpisodeUnroll]; int below[kEpisodeUnroll];
#pragma unroll
  for (int j = 0; j < kEpisodeUnroll; ++j) {
    const int64_t e = first + j * kEpisodeThreads + tid;
    o[j] = false; r[j] = 0.0; l[j] = 0;
    if (e < a.E) { r[j] = a.ret[e] + a.reward[e]; l[j] = a.len[e] + 1; o[j] = a.over[e] != 0; }
    const unsigned long long m = __ballot(o[j]);
    below[j] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[j][wave] = __popcll(m);
  }
  __syncthreads();
  int64_t before = 0;
  for (int w = 0; w < kEpisodeWaves; ++w) before += before_w[w];
  const int64_t head = *head_in;
  const uint32_t cap = (uint32_t)a.cap;
  const uint32_t base = (uint32_t)((head + before) % a.cap);
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < kEpisodeUnroll; ++j) {
    uint32_t k = run;
#pragma unroll
    for (int w = 0; w < kEpisodeWaves; ++w) {
      const uint32_t t = (uint32_t)wave_total[j][w];
      if (w < wave) k += t;
      run += t;
    }
    const int64_t e = first + j * kEpisodeThreads + tid;
    if (e < a.E) {
      if (o[j]) {
        uint32_t slot = base + k + (uint32_t)below[j];
        if (slot >= cap) slot -= cap;
        a.log_score[slot] = r[j]; a.log_len[slot] = l[j]; a.log_env[slot] = (int32_t)e;
        r[j] = 0.0; l[j] = 0;
      }
      a.ret[e] = r[j]; a.len[e] = l[j];
    }
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) *head_out = head + before + run;
}

struct Bufs {
  double *reward, *ret, *log_score; uint8_t* over; int32_t *len, *log_len, *log_env; int64_t* head; int64_t* head2;
};

static Bufs make(int E, int cap, const std::vector<double>& r, const std::vector<uint8_t>& o) {
  Bufs b;
  CK(hipMalloc(&b.reward, 8 * E)); CK(hipMalloc(&b.ret, 8 * E)); CK(hipMalloc(&b.log_score, 8 * (size_t)cap));
  CK(hipMalloc(&b.over, E)); CK(hipMalloc(&b.len, 4 * E)); CK(hipMalloc(&b.log_len, 4 * (size_t)cap));
  CK(hipMalloc(&b.log_env, 4 * (size_t)cap)); CK(hipMalloc(&b.head, 8)); CK(hipMalloc(&b.head2, 8));
  CK(hipMemcpy(b.reward, r.data(), 8 * E, hipMemcpyHostToDevice));
  CK(hipMemcpy(b.over, o.data(), E, hipMemcpyHostToDevice));
  CK(hipMemset(b.ret, 0, 8 * E)); CK(hipMemset(b.len, 0, 4 * E)); CK(hipMemset(b.log_score, 0, 8 * (size_t)cap));
  CK(hipMemset(b.log_len, 0, 4 * (size_t)cap)); CK(hipMemset(b.log_env, 0, 4 * (size_t)cap));
  CK(hipMemset(b.head, 0, 8)); CK(hipMemset(b.head2, 0, 8));
  return b;
}

int main() {
  const int sizes[] = {100, 4096, 65536};
  for (int E : sizes) {
    const int cap = std::max(4 * E, 1024);
    std::vector<double> r(E); std::vector<uint8_t> o(E);
    srand(E);
    for (int e = 0; e < E; ++e) { r[e] = (rand() % 61 - 30) * 0.1; o[e] = rand() % 100 == 0; }
    Bufs A = make(E, cap, r, o), B = make(E, cap, r, o);
    const EpisodeArgs aa{A.reward, A.over, E, A.ret, A.len, A.log_score, A.log_len, A.log_env, cap, A.head};
    const EpisodeArgs ab{B.reward, B.over, E, B.ret, B.len, B.log_score, B.log_len, B.log_env, cap, B.head};
    const int groups = (E + kEpisodeChunk - 1) / kEpisodeChunk;
    int flip = 0;
    auto one = [&]() { hipLaunchKernelGGL(episode_stats_kernel, dim3(1), dim3(kEpisodeThreads), 0, 0, aa); };
    auto multi = [&]() {
      hipLaunchKernelGGL(multi_kernel, dim3(groups), dim3(kEpisodeThreads), 0, 0, ab, flip ? B.head2 : B.head,
                         flip ? B.head : B.head2);
      flip ^= 1;
    };
    // the same 10 launches through both, then the rings must agree
    for (int i = 0; i < 10; ++i) { one(); multi(); }
    CK(hipDeviceSynchronize());
    std::vector<double> sa(cap), sb(cap); std::vector<int32_t> ea(cap), eb(cap);
    int64_t ha = 0, hb = 0;
    CK(hipMemcpy(sa.data(), A.log_score, 8 * (size_t)cap, hipMemcpyDeviceToHost));
    CK(hipMemcpy(sb.data(), B.log_score, 8 * (size_t)cap, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ea.data(), A.log_env, 4 * (size_t)cap, hipMemcpyDeviceToHost));
    CK(hipMemcpy(eb.data(), B.log_env, 4 * (size_t)cap, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&ha, A.head, 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&hb, flip ? B.head2 : B.head, 8, hipMemcpyDeviceToHost));
    const bool same = ha == hb && sa == sb && ea == eb;
    hipEvent_t t0, t1;
    CK(hipEventCreate(&t0)); CK(hipEventCreate(&t1));
    printf("E=%d cap=%d groups=%d head=%lld same=%d\n", E, cap, groups, (long long)ha, (int)same);
    for (int rep = 0; rep < 3; ++rep) {
      for (int which = 0; which < 2; ++which) {
        std::vector<float> us;
        for (int batch = 0; batch < 20; ++batch) {
          CK(hipEventRecord(t0, 0));
          for (int i = 0; i < 20; ++i) { if (which) multi(); else one(); }
          CK(hipEventRecord(t1, 0));
          CK(hipEventSynchronize(t1));
          float ms = 0; CK(hipEventElapsedTime(&ms, t0, t1));
          us.push_back(ms * 1e3f / 20);
        }
        std::sort(us.begin(), us.end());
        printf("  %s: median %.2f us  min %.2f us\n", which ? "multi " : "single", us[10], us[0]);
      }
    }
    fflush(stdout);
  }
  CK(hipDeviceSynchronize());
  return 0;
}
