// Segment-based tp / fp / fn counts for threshold calibration
// (utils/optimize_thresholds.py:31-101 scores every probe with the
// segment-based F1 of utils/utilities.py:294-340 at a 1 s grid).
//
// Perturbing parameter k of the optimiser only changes class k mod C and the
// segment counts are additive over (clip, class), so one gradient epoch is,
// per class, a handful of (high, low) variants of the same series.  This
// kernel walks every variant of a series in one launch with the series read
// once: activity_detection (mode 0 of events.hip, the same device helpers,
// always with the low threshold) -> events rasterised onto the segment grid
// as a 64-bit mask (bits [bgn / seg, ceil(fin / seg))) -> popcounts against
// the series' target mask.  No event list is materialised.
//
// One wavefront per series, one class per workgroup: a workgroup's waves walk
// a chunk of clips of class k, lane v of a wave keeps the running
// (tp, fp, fn, bad) of variant v, the waves reduce into [V][4] LDS words and
// the workgroup issues one integer atomicAdd per non-zero (variant, counter).
// Integer sums: the result does not depend on the order.
#include <algorithm>

#include "events_walk.h"
#include "sedx_internal.h"

namespace sedx {

namespace {

using namespace evwalk;

constexpr int CAL_WAVES = 4;                        // wavefronts per workgroup (at most)
constexpr int CAL_REG_WORDS = 16;                   // T <= 1024: the series stays in registers
constexpr int64_t CAL_LDS_BYTES = 160 * 1024;
constexpr int64_t CAL_ACC_BYTES = 64 * 4 * 8;       // [V <= 64][4] accumulators
constexpr int64_t CAL_MAX_WORDS = (CAL_LDS_BYTES - CAL_ACC_BYTES) / 16;
constexpr int64_t CAL_MAX_PER_WAVE = 16;            // clips per wave (uint32 lane accumulators: 16 * 64 bits)

__device__ __forceinline__ void cal_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// dynamic LDS: [wpb][2][W] bitmap words (on, below), then [V][4] accumulators.
// grid: C * ceil(N / (wpb * per_wave)) workgroups, class = blockIdx.x % C.
template <bool REG>
__global__ __launch_bounds__(64 * CAL_WAVES) void segment_counts_kernel(CalibArgs a, int64_t W, int wpb,
                                                                        int64_t per_wave) {
  extern __shared__ uint64_t cal_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;   // blockDim.x == 64 * wpb
  const int64_t C = a.C, T = a.T, V = a.V, seg = a.seg;
  const int64_t k = blockIdx.x % C, chunk = blockIdx.x / C;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(cal_lds + (int64_t)wpb * 2 * W);
  for (int i = threadIdx.x; i < V * 4; i += blockDim.x) acc[i] = 0;
  __syncthreads();

  uint64_t* om = cal_lds + (int64_t)wave * 2 * W;
  uint64_t* lm = om + W;
  const int64_t ns = a.n_smooth[k], nsalt = a.n_salt[k];
  const int64_t S = (T + seg - 1) / seg;            // <= 64 (api.cpp checks)
  const uint64_t smask = S >= 64 ? ~0ull : ((1ull << S) - 1);
  const BelowMask bm{lm, W, T};
  uint32_t tp = 0, fp = 0, fn = 0, bad = 0;         // lane v: variant v

  const int64_t n0 = (chunk * wpb + wave) * per_wave;
  const int64_t n1 = n0 + per_wave < a.N ? n0 + per_wave : a.N;
  for (int64_t n = n0; n < n1; ++n) {               // wave-uniform
    const float* xs = a.x + n * T * C + k;
    const uint64_t ref = a.target[n * C + k] & smask;
    float xv[CAL_REG_WORDS];
    if (REG) {
#pragma unroll
      for (int j = 0; j < CAL_REG_WORDS; ++j) {
        const int64_t t = (int64_t)j * 64 + lane;
        xv[j] = t < T ? xs[t * C] : 0.f;
      }
    }
    for (int64_t v = 0; v < V; ++v) {
      const float hi = (float)a.hi[v * C + k];      // float32 compares, as events_series_kernel<0>
      const float lo = (float)a.lo[v * C + k];
      if (REG) {
#pragma unroll
        for (int j = 0; j < CAL_REG_WORDS; ++j) {
          if (j >= W) break;
          const int64_t t = (int64_t)j * 64 + lane;
          const uint64_t bon = __ballot(t < T && xv[j] > hi), bbe = __ballot(t < T && xv[j] < lo);
          if (lane == 0) {
            om[j] = bon;
            lm[j] = bbe;
          }
        }
      } else {                                      // long series: re-read per variant (L2)
        for (int64_t w0 = 0; w0 < W; w0 += 8) {
          float u[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int64_t t = (w0 + j) * 64 + lane;
            u[j] = t < T ? xs[t * C] : 0.f;
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (w0 + j >= W) break;
            const int64_t t = (w0 + j) * 64 + lane;
            const uint64_t bon = __ballot(t < T && u[j] > hi), bbe = __ballot(t < T && u[j] < lo);
            if (lane == 0) {
              om[w0 + j] = bon;
              lm[w0 + j] = bbe;
            }
          }
        }
      }
      cal_wave_sync();
      uint64_t est = 0;
      auto emit = [&](int64_t b, int64_t f) {
        // onset floored, offset ceiled to the grid; 0 <= b, f <= T so s1 <= S
        const int64_t s0 = b / seg, s1 = (f + seg - 1) / seg;
        if (s1 > s0 && s0 < 64) {
          const int64_t len = s1 - s0;
          est |= (len >= 64 ? ~0ull : ((1ull << len) - 1)) << s0;
        }
      };
      const bool ok = walk_runs(om, bm, W, T, true, ns, nsalt, emit);
      cal_wave_sync();                              // bitmaps are rewritten by the next variant
      est &= smask;
      if (lane == v) {
        if (ok) {
          tp += __builtin_popcountll(est & ref);
          fp += __builtin_popcountll(est & ~ref);
          fn += __builtin_popcountll(ref & ~est);
        } else {
          bad += 1;
        }
      }
    }
  }
  if (lane < V) {
    if (tp) atomicAdd(&acc[lane * 4 + 0], (unsigned long long)tp);
    if (fp) atomicAdd(&acc[lane * 4 + 1], (unsigned long long)fp);
    if (fn) atomicAdd(&acc[lane * 4 + 2], (unsigned long long)fn);
    if (bad) atomicAdd(&acc[lane * 4 + 3], (unsigned long long)bad);
  }
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(a.counts);
  for (int i = threadIdx.x; i < V * 4; i += blockDim.x) {
    const unsigned long long s = acc[i];
    if (s) atomicAdd(&out[((int64_t)(i >> 2) * C + k) * 4 + (i & 3)], s);
  }
}

}  // namespace

size_t calib_workspace_bytes(int64_t C, int64_t V) {
  // hi f64 [V][C] + lo f64 [V][C] + n_smooth [C] + n_salt [C], 256-B aligned pieces
  return 2 * align256(V * C * 8) + 2 * align256(C * 8);
}

int64_t calib_max_frames() { return CAL_MAX_WORDS * 64; }

void launch_segment_counts(const CalibArgs& a, hipStream_t s) {
  (void)hipMemsetAsync(a.counts, 0, (size_t)a.V * a.C * 4 * sizeof(int64_t), s);
  if (a.N == 0 || a.C == 0) return;
  const int64_t W = std::max<int64_t>((a.T + 63) / 64, 1);    // <= CAL_MAX_WORDS (api.cpp checks)
  const int wpb = (int)std::min<int64_t>(CAL_WAVES, std::max<int64_t>(1, (CAL_LDS_BYTES - CAL_ACC_BYTES) / (16 * W)));
  // enough workgroups to fill the device before a wave takes several clips
  const int64_t per_wave = std::min<int64_t>(CAL_MAX_PER_WAVE, std::max<int64_t>(1, a.N * a.C / (wpb * 4096)));
  const int64_t chunks = (a.N + wpb * per_wave - 1) / (wpb * per_wave);
  const size_t lds = (size_t)wpb * 2 * W * 8 + CAL_ACC_BYTES;
  // > 64 KB of dynamic LDS must be opted into (per device: launch_info)
  if (!launch_info(reinterpret_cast<const void*>(segment_counts_kernel<true>), 64, CAL_LDS_BYTES).ok ||
      !launch_info(reinterpret_cast<const void*>(segment_counts_kernel<false>), 64, CAL_LDS_BYTES).ok)
    return;
  const dim3 grid((unsigned)(chunks * a.C)), block(64 * wpb);
  if (W <= CAL_REG_WORDS)
    hipLaunchKernelGGL(segment_counts_kernel<true>, grid, block, lds, s, a, W, wpb, per_wave);
  else
    hipLaunchKernelGGL(segment_counts_kernel<false>, grid, block, lds, s, a, W, wpb, per_wave);
}

}  // namespace sedx
