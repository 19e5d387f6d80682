// Conformer encoder kernels for gfx950 (the sequence layer of
// Cnn_9layers_Conformer_FrameAtt / _FrameAvg, pytorch/models.py:1189-1625;
// ConformerEncoder(512, adim 144, aheads 4, elayers 3, eunits 576, kernel 7),
// pytorch/models_2020/conformer/).  Activations are [items * T][width]
// row-major fp32, T the sequence length after the three time pools.
//
// Everything here is fp32 in every precision mode: sedx_set_precision selects
// the conv trunk's arithmetic only; the encoder's GEMMs and the 144-wide head
// projection run on the fp32 matrix pipe also under SEDX_PRECISION_X3.
//
//   cf_gemm_kernel     C = epi(A W^T + b) on fp32 MFMA 32x32x2, four waves per
//                      32 x 32 tile, operands straight from global (L2) as
//                      float4 rows.  Every output: four chains over the K
//                      quarters (k ascending, the pair (k, k + 1) per MFMA,
//                      zero start) summed ((q0 + q1) + q2) + q3, + bias, then
//                      the epilogue (Swish, 0.5 y + res, y + res) --
//                      independent of M, so of the batch size and the clip's
//                      position.
//   cf_layernorm_kernel  row LayerNorm over 144 (eps 1e-5), one wave per row;
//                      the input layer's variant adds ReLU, x sqrt(144) and
//                      the positional table pe[t] (conformer_encoder.py:22-28)
//   cf_relpos_kernel   r[blk][j] = [sin(p f), cos(p f)], p = T - 1 - j
//                      (attention.py:135-137, :216), on device every forward
//   cf_relattn_kernel  Transformer-XL relative attention core (attention.py:
//                      250-277): score = ((q + r_w_bias) k + shifted (q +
//                      r_r_bias) r_k) / 6, exact two-pass softmax, P v.
//                      _rel_shift is index math (below), never materialised;
//                      no [T, T] tensor leaves the workgroup
//   cf_glu_dwconv_kernel  GLU, depthwise 7-tap conv over time (zero padded per
//                      clip), folded BatchNorm1d and Swish in one pass
//                      (convolution.py:38-55)
#include "sedx_internal.h"

namespace sedx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float cf_sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---------------------------------------------------------------------------
// GEMM.  grid (ceil(M / 32), ceil(N / 32)), 256 threads = one 32 x 32 tile:
// wave q chains K quarter q (A / W fragments straight from global as float4
// rows, rounds of Q float4 per row, the next round's loads in flight while
// the current round's MFMAs run: the layers here are small and a wave's time
// is load latency, so a quarter-length chain and Q float4 in flight per
// operand matter more than operand reuse), the quarters are summed through
// LDS in the fixed order ((q0 + q1) + q2) + q3.  K % (16 Q) == 0: Q = 9 for
// K = 144 / 576, Q = 8 for K = 512.  Rows / columns past M / N read a valid
// row and are not stored.  res (EPI 2, 3) and C have row stride N and may
// alias: each element is read and written by one thread.
// ---------------------------------------------------------------------------
template <int EPI, int Q>
__global__ __launch_bounds__(256) void cf_gemm_kernel(const float* __restrict__ A, int M, int K,
                                                      const float* __restrict__ W, int N,
                                                      const float* __restrict__ bias, const float* res,
                                                      float* C) {
  __shared__ float part[3][32][33];
  const int lane = threadIdx.x & 63, i = lane & 31, kh = lane >> 5, wq_ = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const int KQ = K / 4;   // this wave's K range: [wq_ KQ, (wq_ + 1) KQ)
  const float4* ap = reinterpret_cast<const float4*>(A + (int64_t)min(m0 + i, M - 1) * K + wq_ * KQ);
  const float4* wp = reinterpret_cast<const float4*>(W + (int64_t)min(n0 + i, N - 1) * K + wq_ * KQ);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float4 xa0[Q], xw0[Q], xa1[Q], xw1[Q];
  const int nr = KQ / (4 * Q);
  auto load = [&](float4* xa, float4* xw, int rd) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      xa[q] = ap[rd * Q + q];
      xw[q] = wp[rd * Q + q];
    }
  };
  // k-step 2q: k = 4q + kh (element kh); k-step 2q + 1: k = 4q + 2 + kh
  auto mma = [&](const float4* xa, const float4* xw) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float4 a = xa[q], b = xw[q];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? a.y : a.x, kh ? b.y : b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? a.w : a.z, kh ? b.w : b.z, acc, 0, 0, 0);
    }
  };
  load(xa0, xw0, 0);
  for (int rd = 0; rd < nr; rd += 2) {   // static buffer names: no dynamic register indexing
    if (rd + 1 < nr) load(xa1, xw1, rd + 1);
    mma(xa0, xw0);
    if (rd + 1 < nr) {
      if (rd + 2 < nr) load(xa0, xw0, rd + 2);
      mma(xa1, xw1);
    }
  }
  if (wq_ > 0)
#pragma unroll
    for (int r = 0; r < 16; ++r) part[wq_ - 1][(r & 3) + 8 * (r >> 2) + 4 * kh][i] = acc[r];
  __syncthreads();
  if (wq_ > 0) return;
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[r] += part[q][(r & 3) + 8 * (r >> 2) + 4 * kh][i];
  const int n = n0 + i;
  if (n >= N) return;
  const float bv = bias ? bias[n] : 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
    if (m < M) {
      float v = acc[r] + bv;
      if (EPI == CF_EPI_SWISH) v = v * cf_sigmoid_(v);
      if (EPI == CF_EPI_HALF_RES) v = 0.5f * v + res[(int64_t)m * N + n];
      if (EPI == CF_EPI_RES) v = v + res[(int64_t)m * N + n];
      C[(int64_t)m * N + n] = v;
    }
  }
}

template <int Q>
static void cf_gemm_dispatch(const float* A, int M, int K, const float* W, int N, const float* bias,
                             const float* res, float* C, int epi, hipStream_t s) {
  const dim3 grid((M + 31) / 32, (N + 31) / 32);
  switch (epi) {
    case CF_EPI_NONE: return launch_kernel(cf_gemm_kernel<CF_EPI_NONE, Q>, grid, 256, s, A, M, K, W, N, bias, res, C);
    case CF_EPI_SWISH:
      return launch_kernel(cf_gemm_kernel<CF_EPI_SWISH, Q>, grid, 256, s, A, M, K, W, N, bias, res, C);
    case CF_EPI_HALF_RES:
      return launch_kernel(cf_gemm_kernel<CF_EPI_HALF_RES, Q>, grid, 256, s, A, M, K, W, N, bias, res, C);
    case CF_EPI_RES: return launch_kernel(cf_gemm_kernel<CF_EPI_RES, Q>, grid, 256, s, A, M, K, W, N, bias, res, C);
    default: return note_launch_error(hipErrorInvalidValue);
  }
}

void launch_cf_gemm(const float* A, int M, int K, const float* W, int N, const float* bias, const float* res,
                    float* C, int epi, hipStream_t s) {
  if (M <= 0 || N <= 0 || K <= 0 || ((epi == CF_EPI_HALF_RES || epi == CF_EPI_RES) && !res))
    return note_launch_error(hipErrorInvalidValue);
  if (K % (16 * 9) == 0) return cf_gemm_dispatch<9>(A, M, K, W, N, bias, res, C, epi, s);
  if (K % (16 * 8) == 0) return cf_gemm_dispatch<8>(A, M, K, W, N, bias, res, C, epi, s);
  note_launch_error(hipErrorInvalidValue);
}

// ---------------------------------------------------------------------------
// LayerNorm over CF_D = 144.  One wave per row (lane l: elements l, l + 64 and,
// for l < 16, l + 128), 4 rows per workgroup; mean, then the biased variance
// of the centred values, both by a xor butterfly (every lane the same sum).
// POS: relu(y) * 12 + pe[row % T] (the encoder's input layer).  x and y may
// alias: a row is read whole before it is written.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float cf_wave_sum_(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

template <bool POS>
__global__ __launch_bounds__(256) void cf_layernorm_kernel(const float* x, int M, int T,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           const float* __restrict__ pe, float* y) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (int64_t)row * CF_D;
  const bool third = lane < CF_D - 128;
  const float v0 = xr[lane], v1 = xr[lane + 64], v2 = third ? xr[lane + 128] : 0.0f;
  const float mean = cf_wave_sum_((v0 + v1) + v2) * (1.0f / CF_D);
  const float d0 = v0 - mean, d1 = v1 - mean, d2 = third ? v2 - mean : 0.0f;
  const float var = cf_wave_sum_((d0 * d0 + d1 * d1) + d2 * d2) * (1.0f / CF_D);
  const float rstd = 1.0f / sqrtf(var + 1e-5f);
  const float* per = POS ? pe + (int64_t)(row % T) * CF_D : nullptr;
  float* yr = y + (int64_t)row * CF_D;
  auto fin = [&](float d, int c) {
    float o = d * rstd * gamma[c] + beta[c];
    if (POS) o = fmaxf(o, 0.0f) * 12.0f + per[c];
    yr[c] = o;
  };
  fin(d0, lane);
  fin(d1, lane + 64);
  if (third) fin(d2, lane + 128);
}

void launch_cf_layernorm(const float* x, int M, const float* gamma, const float* beta, float* y, hipStream_t s) {
  if (M <= 0) return note_launch_error(hipErrorInvalidValue);
  launch_kernel(cf_layernorm_kernel<false>, dim3((M + 3) / 4), 256, s, x, M, 1, gamma, beta,
                static_cast<const float*>(nullptr), y);
}

void launch_cf_input_norm(const float* x, int B, int T, const float* gamma, const float* beta, const float* pe,
                          float* y, hipStream_t s) {
  if (B <= 0 || T <= 0 || T > CF_MAX_T) return note_launch_error(hipErrorInvalidValue);
  const int M = B * T;
  launch_kernel(cf_layernorm_kernel<true>, dim3((M + 3) / 4), 256, s, x, M, T, gamma, beta, pe, y);
}

// ---------------------------------------------------------------------------
// r[blk][j][0..71] = sin(p f[blk][d]), [72..143] = cos(p f[blk][d]), p = T-1-j
// as a float, the product in fp32 like torch.ger; accurate sinf / cosf.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cf_relpos_kernel(const float* __restrict__ inv_freq, int T, int nblk,
                                                        float* __restrict__ r) {
  const int64_t total = (int64_t)nblk * T * CF_D;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int d = (int)(e % CF_D);
    const int64_t bj = e / CF_D;
    const int j = (int)(bj % T), blk = (int)(bj / T);
    const float p = (float)(T - 1 - j);
    const float a = p * inv_freq[blk * (CF_D / 2) + (d < CF_D / 2 ? d : d - CF_D / 2)];
    r[e] = d < CF_D / 2 ? sinf(a) : cosf(a);
  }
}

void launch_cf_relpos(const float* inv_freq, int T, int nblk, float* r, hipStream_t s) {
  if (T <= 0 || nblk <= 0) return note_launch_error(hipErrorInvalidValue);
  const int64_t total = (int64_t)nblk * T * CF_D;
  launch_kernel(cf_relpos_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), 256, s, inv_freq, T,
                nblk, r);
}

// ---------------------------------------------------------------------------
// Relative attention core.  QKV [B][T][432] (q | k | v, head n = columns
// 36 n .. 36 n + 35 of each), rk [T][144] (r_net(r), same head columns), rwb /
// rrb [4][36].  One workgroup per (clip, head, block of 32 queries), 128
// threads: 4 lanes per query row, lane quarter g owns dims 9 g .. 9 g + 8; a
// score is the 4 partial dots summed by two quad shuffles (fixed order).
//
// _rel_shift (attention.py:203-214: pad a zero column, view [T + 1, T], drop
// the first row, view back) in closed form, BD0[i][j] = (q_i + rrb) . rk[j]:
//   j <= i      BD[i][j] = BD0[i][j + T - 1 - i]
//   j == i + 1  BD[i][j] = 0
//   j >= i + 2  BD[i][j] = BD0[i + 1][j - i - 2]      (the NEXT query's row)
// K / V chunks of 64 keys are staged in LDS; rk rows come from L2 (the index
// differs per query row).  Exact two-pass softmax (row maximum, then exp / sum
// / P v), scores recomputed in the second pass.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(128) void cf_relattn_kernel(const float* __restrict__ QKV, int T, int nqb,
                                                         const float* __restrict__ rk,
                                                         const float* __restrict__ rwb,
                                                         const float* __restrict__ rrb, float* __restrict__ O) {
  constexpr int KC = 64, DG = 9, DH = CF_D / 4, LD = 3 * CF_D;
  __shared__ float Ks[KC][DH + 1];
  __shared__ float Vs[KC][DH + 1];
  const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
  const int b = bh >> 2, head = bh & 3;
  const int g = threadIdx.x & 3;
  const int qi = qb * 32 + (threadIdx.x >> 2);
  const bool valid = qi < T;
  const int i = valid ? qi : T - 1;                 // index math of rows past T stays in range
  const float* base = QKV + (int64_t)b * T * LD + head * DH;
  const float* rkh = rk + head * DH + DG * g;
  float qw[DG], qr[DG], qn[DG], o[DG];
#pragma unroll
  for (int d = 0; d < DG; ++d) {
    const float q = base[(int64_t)i * LD + DG * g + d];
    const float q1 = i + 1 < T ? base[(int64_t)(i + 1) * LD + DG * g + d] : 0.0f;
    const float bw = rwb[head * DH + DG * g + d], br = rrb[head * DH + DG * g + d];
    qw[d] = q + bw;
    qr[d] = q + br;
    qn[d] = q1 + br;
    o[d] = 0.0f;
  }
  // (AC + BD)[i][c0 + jj] * scale
  auto score = [&](int c0, int jj) {
    const int j = c0 + jj;
    const bool lo = j <= i, zero = j == i + 1;
    const int idx = lo ? j + T - 1 - i : (zero ? 0 : j - i - 2);
    const float* rr = rkh + (int64_t)idx * CF_D;
    float ac = 0.f, bd = 0.f;
#pragma unroll
    for (int d = 0; d < DG; ++d) {
      ac = fmaf(qw[d], Ks[jj][DG * g + d], ac);
      bd = fmaf(lo ? qr[d] : qn[d], rr[d], bd);
    }
    float sc = ac + (zero ? 0.0f : bd);
    sc += __shfl_xor(sc, 1);
    sc += __shfl_xor(sc, 2);
    return sc * (1.0f / 6.0f);
  };
  auto stage = [&](int c0, int nk, bool v) {
    __syncthreads();
    for (int e = threadIdx.x; e < nk * DH; e += 128) {
      const int jj = e / DH, d = e - jj * DH;
      const float* src = base + (int64_t)(c0 + jj) * LD + d;
      Ks[jj][d] = src[CF_D];
      if (v) Vs[jj][d] = src[2 * CF_D];
    }
    __syncthreads();
  };
  float mx = -INFINITY;
  for (int c0 = 0; c0 < T; c0 += KC) {
    const int nk = min(KC, T - c0);
    stage(c0, nk, false);
    for (int jj = 0; jj < nk; ++jj) mx = fmaxf(mx, score(c0, jj));
  }
  float l = 0.f;
  for (int c0 = 0; c0 < T; c0 += KC) {
    const int nk = min(KC, T - c0);
    stage(c0, nk, true);
    for (int jj = 0; jj < nk; ++jj) {
      const float p = expf(score(c0, jj) - mx);
      l += p;
#pragma unroll
      for (int d = 0; d < DG; ++d) o[d] = fmaf(p, Vs[jj][DG * g + d], o[d]);
    }
  }
  if (valid) {
    const float inv = 1.0f / l;
    float* dst = O + ((int64_t)b * T + qi) * CF_D + head * DH + DG * g;
#pragma unroll
    for (int d = 0; d < DG; ++d) dst[d] = o[d] * inv;
  }
}

void launch_cf_relattn(const float* QKV, int B, int T, const float* rk, const float* rwb, const float* rrb,
                       float* O, hipStream_t s) {
  const int nqb = (T + 31) / 32;
  if (B <= 0 || T <= 0 || T > CF_MAX_T || (int64_t)nqb * B * 4 > INT32_MAX)
    return note_launch_error(hipErrorInvalidValue);
  launch_kernel(cf_relattn_kernel, dim3((unsigned)(nqb * B * 4)), 128, s, QKV, T, nqb, rk, rwb, rrb, O);
}

// ---------------------------------------------------------------------------
// GLU + depthwise conv + folded BN + Swish.  Y [B][T][288] (a | b halves of the
// first pointwise conv), wt [7][144] = tap-major depthwise weights times the
// BN scale, bf [144] the folded bias; Z [B][T][144].  Workgroup = (clip, 32
// frames): the 38 x 144 GLU values a sigmoid(b) of its frames and the 3-frame
// halo land in LDS once (frames outside the clip are zero: the conv's own
// zero padding, never the neighbouring clip), then the 7 taps in ascending
// order, + bias, Swish.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cf_glu_dwconv_kernel(const float* __restrict__ Y, int T,
                                                            const float* __restrict__ wt,
                                                            const float* __restrict__ bf, float* __restrict__ Z) {
  constexpr int TT = 32, KW = 7, HALO = KW / 2;
  __shared__ float G[TT + 2 * HALO][CF_D];
  const int b = blockIdx.x, t0 = blockIdx.y * TT;
  const float* yb = Y + (int64_t)b * T * (2 * CF_D);
  for (int e = threadIdx.x; e < (TT + 2 * HALO) * CF_D; e += 256) {
    const int tt = e / CF_D, c = e - tt * CF_D;
    const int t = t0 + tt - HALO;
    float v = 0.0f;
    if (t >= 0 && t < T) {
      const float* yr = yb + (int64_t)t * (2 * CF_D);
      v = yr[c] * cf_sigmoid_(yr[CF_D + c]);
    }
    G[tt][c] = v;
  }
  __syncthreads();
  const int nt = min(TT, T - t0);
  for (int e = threadIdx.x; e < nt * CF_D; e += 256) {
    const int tt = e / CF_D, c = e - tt * CF_D;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < KW; ++k) acc = fmaf(wt[k * CF_D + c], G[tt + k][c], acc);
    acc += bf[c];
    Z[((int64_t)b * T + t0 + tt) * CF_D + c] = acc * cf_sigmoid_(acc);
  }
}

void launch_cf_glu_dwconv(const float* Y, int B, int T, const float* wt, const float* bf, float* Z, hipStream_t s) {
  if (B <= 0 || T <= 0 || T > CF_MAX_T) return note_launch_error(hipErrorInvalidValue);
  launch_kernel(cf_glu_dwconv_kernel, dim3(B, (T + 31) / 32), 256, s, Y, T, wt, bf, Z);
}

}  // namespace sedx
