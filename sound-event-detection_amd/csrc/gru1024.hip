// bi-GRU recurrence of the 14-layer model: nn.GRU(2048, 1024, bidirectional)
// (pytorch/models.py:727, :773; torch nn.GRU semantics as seq.hip's gru_kernel).
//
// W_hh is [2][3072][1024] = 25 MB: it cannot live in registers as in gru.hip,
// so it is streamed from L2 / Infinity Cache every step, and the hand-off
// between steps is the launch boundary: ONE launch per time step carries both
// directions (the reverse one walks t downwards) and all clips.  No spins, no
// cross-workgroup hand-offs: nothing here can time out.
//
// Workgroup = (32 hidden units, direction, 32 clips), 12 waves: wave
// (gate g, quarter q) multiplies the 32 clips' h_{t-1}[256 q .. 256 q + 255]
// with the 32 rows of gate g on the fp32 matrix pipe (32x32x2, operands as
// float4 rows straight from global), then the gate math runs in the same launch.
//
// Summation order of a gate's product (fixed, independent of B): four chains,
// one per K quarter, each an in-order fma chain from zero over its 256 k
// ascending; combined ((q0 + q1) + q2) + q3.  Then, as gru_kernel:
//   r = sigmoid(gr + (ar + br)), z = sigmoid(gz + (az + bz)),
//   n = tanh(gn + r (an + bn)),  h = n + z (h_prev - n).
// Step 0 has h_prev = 0: the products are zero and are not computed.
#include "sedx_internal.h"

namespace sedx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int GH = 1024;   // hidden size
__device__ __forceinline__ float sigmoid1024_(float x) { return 1.0f / (1.0f + expf(-x)); }
}  // namespace

// G [B][T][2][3072] = x W_ih^T + b_ih (r | z | n per direction); whh [2][3072][1024];
// bhh [2][3072]; H [B][T][2048] (forward | reverse); step s of T
__global__ __launch_bounds__(768) void gru1024_step_kernel(const float* __restrict__ G, int B, int T, int step,
                                                           const float* __restrict__ whh,
                                                           const float* __restrict__ bhh, float* H) {
  __shared__ float part[12][32][33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, kh = lane >> 5;
  const int gate = wave >> 2, kq = wave & 3;
  const int j0 = blockIdx.x * 32, dir = blockIdx.y, b0 = blockIdx.z * 32;
  const int t = dir == 0 ? step : T - 1 - step;
  const int tp = dir == 0 ? t - 1 : t + 1;   // the previous step's frame
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  if (step > 0) {
    const int bc = min(b0 + i, B - 1);   // clips past B: any valid row, never stored
    const float4* ap = reinterpret_cast<const float4*>(H + ((int64_t)bc * T + tp) * (2 * GH) + dir * GH + kq * 256);
    const float4* wp =
        reinterpret_cast<const float4*>(whh + ((int64_t)dir * 3 * GH + gate * GH + j0 + i) * GH + kq * 256);
    constexpr int Q = 8;   // float4 per row per round (32 k); two rounds in registers
    float4 xa0[Q], xw0[Q], xa1[Q], xw1[Q];
    constexpr int nr = 256 / (4 * Q);
    auto load = [&](float4* xa, float4* xw, int rd) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        xa[q] = ap[rd * Q + q];
        xw[q] = wp[rd * Q + q];
      }
    };
    // k-step 2q: k = 4q + kh; k-step 2q + 1: k = 4q + 2 + kh
    auto mma = [&](const float4* xa, const float4* xw) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float4 a = xa[q], w = xw[q];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? a.y : a.x, kh ? w.y : w.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? a.w : a.z, kh ? w.w : w.z, acc, 0, 0, 0);
      }
    };
    load(xa0, xw0, 0);
    for (int rd = 0; rd < nr; rd += 2) {   // static buffer names: no dynamic register indexing
      load(xa1, xw1, rd + 1);
      mma(xa0, xw0);
      if (rd + 2 < nr) load(xa0, xw0, rd + 2);
      mma(xa1, xw1);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) part[wave][(r & 3) + 8 * (r >> 2) + 4 * kh][i] = acc[r];   // [clip][unit]
  __syncthreads();
  for (int e = tid; e < 32 * 32; e += 768) {
    const int bl = e >> 5, jl = e & 31, b = b0 + bl, j = j0 + jl;
    if (b >= B) continue;
    auto gsum = [&](int g) {
      return ((part[4 * g][bl][jl] + part[4 * g + 1][bl][jl]) + part[4 * g + 2][bl][jl]) + part[4 * g + 3][bl][jl];
    };
    const float ar = gsum(0), az = gsum(1), an = gsum(2);
    const float* g = G + ((int64_t)b * T + t) * (6 * GH) + dir * 3 * GH;
    const float* bh = bhh + dir * 3 * GH;
    const float hp = step > 0 ? H[((int64_t)b * T + tp) * (2 * GH) + dir * GH + j] : 0.0f;
    const float r = sigmoid1024_(g[j] + (ar + bh[j]));
    const float z = sigmoid1024_(g[GH + j] + (az + bh[GH + j]));
    const float n = tanhf(g[2 * GH + j] + r * (an + bh[2 * GH + j]));
    H[((int64_t)b * T + t) * (2 * GH) + dir * GH + j] = n + z * (hp - n);   // ATen GRU cell: (1-z) n + z h
  }
}

void launch_gru1024(const float* G, int B, int T, const float* whh, const float* bhh, float* H, hipStream_t s) {
  if (B <= 0 || T <= 0) return note_launch_error(hipErrorInvalidValue);
  const dim3 grid(GH / 32, 2, (unsigned)((B + 31) / 32));
  for (int step = 0; step < T; ++step) launch_kernel(gru1024_step_kernel, grid, 768, s, G, B, T, step, whh, bhh, H);
}

}  // namespace sedx
