// Cnn14_DecisionLevelAtt's decision-level stage (pytorch/models.py:2765-2770)
// as ONE launch on the fp32 matrix pipe, fp32 in every precision mode:
//
//     x1 = max_pool1d(x, 3, 1, 1);  x2 = avg_pool1d(x, 3, 1, 1);  relu(fc1(x1 + x2))
//
//   S [B][T][2048]   block 6's frequency mean (capture 43), every value >= 0
//   H [B][T][2048]   the head's input (capture 9)
//   M = B T rows m = (b, t), N = 2048 outputs n, K = 2048.
//
// The pooled operand.  P is computed in registers while the A fragments are
// staged and never reaches memory.  With lo = S[b][t-1][k] and hi =
// S[b][t+1][k] where that frame exists IN CLIP b, else 0.0f (avg_pool1d's zero
// padding, count_include_pad: always / 3):
//     P[m][k] = max(S[m][k] and the in-clip neighbours) + ((lo + S[m][k]) + hi) / 3.0f
// (a correctly rounded fp32 division; max_pool1d pads with -inf, i.e. takes the
// in-clip frames only).  Row m reads rows m - 1 and m + 1 only when they are
// frames of its own clip, whatever M tile they fall in: the neighbour of a
// clip's first / last frame is never the next clip's row.
//
// Tiles.  A workgroup (4 waves) owns 32 rows x 16 NT outputs as 2 x NT tiles of
// v_mfma_f32_16x16x4_f32: the two row tiles share a W fragment, the NT column
// tiles share a P fragment; wave q multiplies K quarter q (k = 512 q .. 512 q +
// 511).  NT = 1 below 97 rows, grid (ceil(M / 32), 128): one clip of 10 s
// (M = 31) streams fc1's 16.8 MB through 128 workgroups = 512 waves, each row
// of W read once.  NT = 4 from 97 rows on, grid (ceil(M / 32), 32): P is
// formed 32 times per row instead of 128 times (its divisions are the
// launch's VALU work) and the A operand is read a quarter as often.  Rows
// past M load row M - 1 and are never stored.
//
// Summation order (the tests' CPU emulation follows it).  The MFMA is the
// in-order fma chain over its four k ("fp32 MFMA semantics"); lane
// (i, j = lane >> 4) loads the float4 at k = 16 g + 4 j of a 16-k group g and
// the group's four MFMAs take its components c = 0..3, so for output (m, n):
//     for q in 0..3:  a_q = 0
//       for g in 0..31:  for c in 0..3:  for j in 0..3:
//         k = 512 q + 16 g + 4 j + c;   a_q = fma(P[m][k], W1[n][k], a_q)
//     H[m][n] = max((((a_0 + a_1) + a_2) + a_3) + b1[n], 0)
// The order depends on neither B, M, NT nor the tile a row falls in (the K
// split is the same fixed one at every M, as linear_small_kernel<0, 4>'s is),
// so a clip's outputs are bit-identical at every batch size and position.
//
// Loads come straight from global / L2 as float4 (no LDS staging: the four
// waves of a workgroup read disjoint K quarters), two 32-k rounds in registers
// so that the next round's loads are in flight under this round's MFMAs.
// Plain grid launch on the caller's stream: no spins, no counters.
#include "sedx_internal.h"

namespace sedx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int DEC_W = 2048;            // fc1: Linear(2048, 2048)
constexpr int DEC_KQ = DEC_W / 4;      // k per wave
constexpr int DEC_G = 2;               // 16-k groups per register round
constexpr int DEC_ROUNDS = DEC_KQ / (16 * DEC_G);

template <int NT>
struct DecFrag {
  float4 w[NT][DEC_G], c[2][DEC_G], lo[2][DEC_G], hi[2][DEC_G];
};

__device__ __forceinline__ float pool3(float lo, float c, float hi, bool has_lo, bool has_hi) {
  float mx = c;
  if (has_lo) mx = fmaxf(mx, lo);
  if (has_hi) mx = fmaxf(mx, hi);
  const float l = has_lo ? lo : 0.0f, h = has_hi ? hi : 0.0f;
  return mx + ((l + c) + h) / 3.0f;
}
}  // namespace

template <int NT>
__global__ __launch_bounds__(256) void decision_kernel(const float* __restrict__ S, int M, int T,
                                                       const float* __restrict__ W1,
                                                       const float* __restrict__ b1, float* __restrict__ H) {
  const int lane = threadIdx.x & 63, i = lane & 15, j = lane >> 4, q = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * 16 * NT;
  // this lane's row of each 16-row tile, its in-clip neighbours (its own row where there is none: a valid
  // address whose value pool3 drops) and its W row, all at k = 512 q + 4 j
  const float4 *pc[2], *plo[2], *phi[2];
  bool has_lo[2], has_hi[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int m = min(m0 + 16 * r + i, M - 1), t = m % T;
    has_lo[r] = t > 0;
    has_hi[r] = t < T - 1;
    pc[r] = reinterpret_cast<const float4*>(S + (int64_t)m * DEC_W + q * DEC_KQ + 4 * j);
    plo[r] = has_lo[r] ? pc[r] - DEC_W / 4 : pc[r];
    phi[r] = has_hi[r] ? pc[r] + DEC_W / 4 : pc[r];
  }
  // column tile nt's W row: n0 + 16 nt + i
  const float4* pw = reinterpret_cast<const float4*>(W1 + (int64_t)(n0 + i) * DEC_W + q * DEC_KQ + 4 * j);
  f32x4 acc[2][NT];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[r][nt][e] = 0.0f;
  auto load = [&](DecFrag<NT>& f, int rd) {
#pragma unroll
    for (int g = 0; g < DEC_G; ++g) {
      const int o = 4 * (rd * DEC_G + g);   // float4 index of group g's k = 16 g (+ 4 j in the base pointers)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) f.w[nt][g] = pw[nt * 16 * (DEC_W / 4) + o];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        f.c[r][g] = pc[r][o];
        f.lo[r][g] = plo[r][o];
        f.hi[r][g] = phi[r][o];
      }
    }
  };
  auto mma = [&](const DecFrag<NT>& f) {
#pragma unroll
    for (int g = 0; g < DEC_G; ++g) {
      float4 p[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        p[r].x = pool3(f.lo[r][g].x, f.c[r][g].x, f.hi[r][g].x, has_lo[r], has_hi[r]);
        p[r].y = pool3(f.lo[r][g].y, f.c[r][g].y, f.hi[r][g].y, has_lo[r], has_hi[r]);
        p[r].z = pool3(f.lo[r][g].z, f.c[r][g].z, f.hi[r][g].z, has_lo[r], has_hi[r]);
        p[r].w = pool3(f.lo[r][g].w, f.c[r][g].w, f.hi[r][g].w, has_lo[r], has_hi[r]);
      }
      // each accumulator takes the group's components in the order x, y, z, w
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float4 w = f.w[nt][g];
#pragma unroll
        for (int r = 0; r < 2; ++r) acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[r].x, w.x, acc[r][nt], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 2; ++r) acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[r].y, w.y, acc[r][nt], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 2; ++r) acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[r].z, w.z, acc[r][nt], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 2; ++r) acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[r].w, w.w, acc[r][nt], 0, 0, 0);
      }
    }
  };
  DecFrag<NT> f0, f1;   // static buffer names: no dynamic register indexing
  load(f0, 0);
  for (int rd = 0; rd < DEC_ROUNDS; rd += 2) {
    load(f1, rd + 1);                        // DEC_ROUNDS is even
    mma(f0);
    if (rd + 2 < DEC_ROUNDS) load(f0, rd + 2);
    mma(f1);
  }
  // the K quarters, in order, through LDS: D[row = 4 j + e][col = i] of each tile
  __shared__ float part[3][32][16 * NT + 1];
  if (q > 0)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) part[q - 1][16 * r + 4 * j + e][16 * nt + i] = acc[r][nt][e];
  __syncthreads();
  if (q > 0) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + 16 * nt + i;
    const float bv = b1[n];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * r + 4 * j + e, m = m0 + row;
        float v = acc[r][nt][e];
#pragma unroll
        for (int p = 0; p < 3; ++p) v += part[p][row][16 * nt + i];
        if (m < M) H[(int64_t)m * DEC_W + n] = fmaxf(v + bv, 0.0f);
      }
  }
}

void launch_decision(const float* S, int B, int T, const float* W1, const float* b1, float* H, hipStream_t s) {
  static_assert(DEC_ROUNDS % 2 == 0, "the round loop runs two register buffers per pass");
  if (B < 1 || T < 1 || (int64_t)B * T > INT32_MAX / DEC_W) return note_launch_error(hipErrorInvalidValue);
  const int M = B * T;
  // four column tiles per workgroup once that still leaves 128 workgroups (the same bits either way)
  if (M > 96)
    launch_kernel(decision_kernel<4>, dim3((M + 31) / 32, DEC_W / 64), 256, s, S, M, T, W1, b1, H);
  else
    launch_kernel(decision_kernel<1>, dim3((M + 31) / 32, DEC_W / 16), 256, s, S, M, T, W1, b1, H);
}

}  // namespace sedx
