// Cnn14_DecisionLevelAtt's decision-level stage, fused against two launches
// (DESIGN.md "Decision-level head"): csrc/decision.hip's one launch (pooling
// inside fc1's A staging) and the form it replaced on paper, a plain pooling
// kernel that writes P [M][2048] followed by seq.hip's launch_linear(act = 1),
// on the same random S >= 0 and weights, same process, alternating.  Prints the
// largest difference between the two results (their summation orders differ)
// and one JSON line per batch size: the mean time per call of three repeats.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -fno-vectorize -Wno-unused-result \
//     -Isound-event-detection_amd/csrc -o decision_bench tools/decision_bench.cpp \
//     sound-event-detection_amd/csrc/decision.hip sound-event-detection_amd/csrc/seq.hip \
//     sound-event-detection_amd/csrc/plan.cpp sound-event-detection_amd/csrc/windows.cpp
//   decision_bench [B ...]        (default 1 32; T5 = 31, a 10 s clip)
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../sound-event-detection_amd/csrc/sedx_internal.h"

#define HIP_OK(x)                                                                 \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));      \
      std::exit(2);                                                               \
    }                                                                             \
  } while (0)

// the two-launch form's first launch: P = max_pool1d(3, 1, 1)(S) + avg_pool1d(3, 1, 1)(S), decision.hip's arithmetic
__global__ __launch_bounds__(256) void pool3_kernel(const float* __restrict__ S, int M, int T, float* __restrict__ P) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // one float4 of [M][2048]
  if (i >= (int64_t)M * 512) return;
  const int m = (int)(i / 512), t = m % T;
  const float4* s = reinterpret_cast<const float4*>(S) + i;
  const bool has_lo = t > 0, has_hi = t < T - 1;
  const float4 c = s[0], lo = has_lo ? s[-512] : make_float4(0.f, 0.f, 0.f, 0.f),
               hi = has_hi ? s[512] : make_float4(0.f, 0.f, 0.f, 0.f);
  auto f = [&](float l, float x, float h) {
    float mx = x;
    if (has_lo) mx = fmaxf(mx, l);
    if (has_hi) mx = fmaxf(mx, h);
    return mx + ((l + x) + h) / 3.0f;
  };
  reinterpret_cast<float4*>(P)[i] = make_float4(f(lo.x, c.x, hi.x), f(lo.y, c.y, hi.y), f(lo.z, c.z, hi.z), f(lo.w, c.w, hi.w));
}

int main(int argc, char** argv) {
  std::vector<int> batches;
  for (int i = 1; i < argc; ++i) batches.push_back(std::atoi(argv[i]));
  if (batches.empty()) batches = {1, 32};
  const int T = 31, W = 2048, iters = 50, repeats = 3;
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> uw(-0.038f, 0.038f), us(0.f, 2.f);   // xavier(2048, 2048) = sqrt(6 / 4096)
  std::vector<float> hw((size_t)W * W), hb(W);
  for (auto& v : hw) v = uw(rng);
  for (auto& v : hb) v = 0.1f * uw(rng) / 0.038f;
  float *W1, *b1;
  HIP_OK(hipMalloc(&W1, hw.size() * 4));
  HIP_OK(hipMalloc(&b1, hb.size() * 4));
  HIP_OK(hipMemcpy(W1, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(b1, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
  hipStream_t s;
  HIP_OK(hipStreamCreate(&s));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  for (int B : batches) {
    if (B < 1 || B > 4096) continue;
    const int M = B * T;
    std::vector<float> hs((size_t)M * W);
    for (auto& v : hs) v = us(rng);
    float *S, *P, *H1, *H2;
    HIP_OK(hipMalloc(&S, hs.size() * 4));
    HIP_OK(hipMalloc(&P, hs.size() * 4));
    HIP_OK(hipMalloc(&H1, hs.size() * 4));
    HIP_OK(hipMalloc(&H2, hs.size() * 4));
    HIP_OK(hipMemcpy(S, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
    auto fused = [&] { sedx::launch_decision(S, B, T, W1, b1, H1, s); };
    auto two = [&] {
      hipLaunchKernelGGL(pool3_kernel, dim3((unsigned)(((int64_t)M * 512 + 255) / 256)), dim3(256), 0, s, S, M, T, P);
      sedx::launch_linear(P, M, W, W1, W, b1, H2, 1, s);
    };
    auto timed = [&](auto&& fn) {
      HIP_OK(hipEventRecord(e0, s));
      for (int i = 0; i < iters; ++i) fn();
      HIP_OK(hipEventRecord(e1, s));
      HIP_OK(hipEventSynchronize(e1));
      float ms = 0.f;
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      return ms * 1000.f / iters;
    };
    for (int i = 0; i < 5; ++i) fused(), two();
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(sedx::take_launch_error());
    HIP_OK(hipGetLastError());
    std::vector<float> a(hs.size()), b(hs.size());
    HIP_OK(hipMemcpy(a.data(), H1, a.size() * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(b.data(), H2, b.size() * 4, hipMemcpyDeviceToHost));
    double dmax = 0, vmax = 0;
    for (size_t i = 0; i < a.size(); ++i) dmax = std::fmax(dmax, std::fabs((double)a[i] - b[i])), vmax = std::fmax(vmax, std::fabs((double)b[i]));
    float tf[3], tt[3];
    for (int r = 0; r < repeats; ++r) tf[r] = timed(fused), tt[r] = timed(two);   // alternating
    std::printf("{\"B\": %d, \"M\": %d, \"fused_us\": [%.2f, %.2f, %.2f], \"two_launch_us\": [%.2f, %.2f, %.2f], "
                "\"max_abs_diff\": %.3g, \"max_abs_value\": %.3g}\n",
                B, M, tf[0], tf[1], tf[2], tt[0], tt[1], tt[2], dmax, vmax);
    for (float* p : {S, P, H1, H2}) HIP_OK(hipFree(p));
  }
  return 0;
}
