// The Conformer encoder's relative attention core on the fp32 matrix pipe of gfx950 (v_mfma_f32_16x16x4_f32; the
// head width 36 is nine K = 4 steps).  Same operands and output as cf_relattn_kernel (conformer.hip), selected by
// SEDX_TUNE_CF_ATTN: QKV [B][T][432] (q | k | v, head n = columns 36 n .. 36 n + 35 of each), rk [T][144] =
// r_net(r), rwb / rrb [4][36] -> O [B][T][144]; score = ((q + r_w_bias) k + shifted (q + r_r_bias) r_k) / 6,
// softmax over all T keys, P v (attention.py:250-277).  fp32 throughout, 1 <= T <= CF_MAX_T; a plain grid launch.
//
// A workgroup is (clip, head, 64 queries): four waves of 16 queries, keys in chunks of 64 through LDS.  A wave
// holds a 64 key x 16 query score tile transposed -- keys are the MFMA's C rows, queries its columns (lane & 15)
// -- so lane group g = lane >> 4 and register r of 16-key tile kt hold key 16 kt + 4 g + r, which is exactly the
// B operand of the P v MFMAs (V is read as the A operand by the same key map): no re-layout of the probabilities.
//
// _rel_shift by index math, on the offset d = j - i alone.  With e = d + T - 1 and the extended table
//   E[e] = rk[e] (0 <= e <= T - 1),  0 (e = T: the j = i + 1 zero),  rk[e - T - 1] (T + 1 <= e <= 2 T - 2),
// BD[i][j] = (q_i + rrb) . E[e] for e <= T - 1 and (q_{i+1} + rrb) . E[e] for e >= T (the NEXT query's row;
// conformer.hip states the closed form).  A wave's 16 x 64 tile needs the 79 consecutive rows e = e0 .. e0 + 78,
// e0 = j0 - i0 - 15 + T - 1: five 16-row MFMA tiles G[m][ii] = E[e0 + m] . q_ii (from q_i where the tile's rows
// have e <= T - 1, from q_{i+1} where they have e >= T, both and a per-row select where a tile straddles T), written
// to a per-wave LDS scratch and read back skewed: element (key jj, query ii) is G[jj - ii + 15][ii].  No [T, T]
// tensor leaves the workgroup; rows of E outside [0, 2 T - 2] and keys past T are staged as zeros, keys past T
// get the score -inf, queries past T are computed on row T - 1 and not stored.
//
// Softmax: exact, online over the chunks in ascending key order: running maximum m, the sum and the output
// rescaled by exp(m_old - m_new) at every chunk, p = exp(s - m_new) with expf.
// Per-output summation order (independent of B and of the clip's position: a workgroup reads one clip):
//   a score: AC and each G element are in-order fp32 fma chains over the 36 dims, d ascending, from zero (one
//     MFMA per 4 dims: k = lane group); score = (AC + G) * (1 / 6).
//   the sum l of a query: per lane group g, chunk by chunk l_g = l_g * alpha + p in (kt, r) ascending order over
//     its keys 16 kt + 4 g + r; at the end l = (l_0 + l_1) + (l_2 + l_3) (two xor shuffles; every lane the same).
//   O[i][d]: one chain over the keys, chunk by chunk (the chain times alpha first), inside a chunk kt ascending,
//     then r ascending, then g ascending (one MFMA per (kt, r): keys 16 kt + r, + 4, + 8, + 12); then * (1 / l).
#include "sedx_internal.h"

namespace sedx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int MX_DH = CF_D / 4;   // 36 dims of a head
constexpr int MX_KC = 64;         // keys of a chunk
constexpr int MX_EB = 128;        // rows of E staged per chunk: e = j0 - I0 - 63 + T - 1 + x
constexpr int MX_GS = 84;         // row stride of the skew scratch (80 band columns; 16-byte rows)
}  // namespace

__global__ __launch_bounds__(256) void cf_relattn_mx_kernel(const float* __restrict__ QKV, int T, int nqb,
                                                            const float* __restrict__ rk,
                                                            const float* __restrict__ rwb,
                                                            const float* __restrict__ rrb, float* __restrict__ O) {
  constexpr int DH = MX_DH, LD = 3 * CF_D, NS = DH / 4;
  // row stride 36: lane (row = lane & 15, k = lane >> 4) of an A fragment reads bank 36 row + k, all 64 distinct
  __shared__ __attribute__((aligned(16))) float Ks[MX_KC][DH];
  __shared__ __attribute__((aligned(16))) float Vs[MX_KC][DH];
  __shared__ __attribute__((aligned(16))) float Es[MX_EB][DH];
  __shared__ __attribute__((aligned(16))) float Gs[4][16][MX_GS];
  const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
  const int b = bh >> 2, head = bh & 3;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int I0 = qb * 64, i0 = I0 + 16 * w;
  const int qi = i0 + c;                 // this lane's query: the column of every tile below
  const int i = min(qi, T - 1);          // index math of rows past T stays in range
  const bool wave_active = i0 < T;       // (uniform per wave) a wave with no query still stages and waits
  const float* base = QKV + (int64_t)b * T * LD + head * DH;
  const float* rkh = rk + head * DH;
  // B fragments: lane holds dim 4 s + g of its query at k-step s
  float qw[NS], qr[NS], qn[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int d = 4 * s + g;
    const float q = base[(int64_t)i * LD + d];
    const float q1 = i + 1 < T ? base[(int64_t)(i + 1) * LD + d] : 0.0f;
    const float bw = rwb[head * DH + d], br = rrb[head * DH + d];
    qw[s] = q + bw;
    qr[s] = q + br;
    qn[s] = q1 + br;
  }
  f32x4 o[3];
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrun = -INFINITY, lsum = 0.0f;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  for (int j0 = 0; j0 < T; j0 += MX_KC) {
    __syncthreads();   // every wave is done with the previous chunk's K, V and E
    for (int e = tid; e < MX_KC * (DH / 4); e += 256) {
      const int jj = e / (DH / 4), c4 = e - jj * (DH / 4), j = j0 + jj;
      float4 kv = zero4, vv = zero4;
      if (j < T) {
        const float4* src = reinterpret_cast<const float4*>(base + (int64_t)j * LD);
        kv = src[CF_D / 4 + c4];
        vv = src[2 * CF_D / 4 + c4];
      }
      *reinterpret_cast<float4*>(&Ks[jj][4 * c4]) = kv;
      *reinterpret_cast<float4*>(&Vs[jj][4 * c4]) = vv;
    }
    const int eb = j0 - I0 - 63 + T - 1;
    for (int e = tid; e < MX_EB * (DH / 4); e += 256) {
      const int x = e / (DH / 4), c4 = e - x * (DH / 4), ee = eb + x;
      const int idx = ee <= T - 1 ? ee : ee - T - 1;             // ee = T: -1
      const bool ok = ee >= 0 && ee <= 2 * T - 2 && idx >= 0;    // so 0 <= idx <= T - 1
      float4 v = zero4;
      if (ok) v = reinterpret_cast<const float4*>(rkh + (int64_t)idx * CF_D)[c4];
      *reinterpret_cast<float4*>(&Es[x][4 * c4]) = v;
    }
    __syncthreads();
    if (!wave_active) continue;

    // ---- AC^T: keys x queries, four 16-key tiles chained side by side ----
    f32x4 sc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        sc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[16 * kt + c][4 * s + g], qw[s], sc[kt], 0, 0, 0);

    // ---- the band G[m][ii], m = 0 .. 79: rows xw + m of Es, e = ew0 + m ----
    const int xw = 48 - 16 * w;
    const int ew0 = eb + xw;   // = j0 - i0 - 15 + T - 1
    f32x4 g1[5], g2[5];
#pragma unroll
    for (int mt = 0; mt < 5; ++mt) g1[mt] = g2[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool need1 = ew0 <= T - 1;        // some row has e <= T - 1: this query's row of BD0
    const bool need2 = ew0 + 79 >= T + 1;   // some row has e >= T + 1: the next query's row
    if (need1) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int mt = 0; mt < 5; ++mt)
          g1[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Es[xw + 16 * mt + c][4 * s + g], qr[s], g1[mt], 0, 0, 0);
    }
    if (need2) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int mt = 0; mt < 5; ++mt)
          g2[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Es[xw + 16 * mt + c][4 * s + g], qn[s], g2[mt], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < 5; ++mt) {
      float4 v;
      const int e_row = ew0 + 16 * mt + 4 * g;   // e of register 0
      v.x = e_row + 0 <= T - 1 ? g1[mt][0] : g2[mt][0];
      v.y = e_row + 1 <= T - 1 ? g1[mt][1] : g2[mt][1];
      v.z = e_row + 2 <= T - 1 ? g1[mt][2] : g2[mt][2];
      v.w = e_row + 3 <= T - 1 ? g1[mt][3] : g2[mt][3];
      *reinterpret_cast<float4*>(&Gs[w][c][16 * mt + 4 * g]) = v;
    }
    __builtin_amdgcn_wave_barrier();   // the scratch is this wave's own: its LDS accesses complete in order

    // ---- scores, the chunk's maximum ----
    float cmax = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jj = 16 * kt + 4 * g + r;
        const float bd = Gs[w][c][jj - c + 15];
        float sv = (sc[kt][r] + bd) * (1.0f / 6.0f);
        if (j0 + jj >= T) sv = -INFINITY;
        sc[kt][r] = sv;
        cmax = fmaxf(cmax, sv);
      }
    __builtin_amdgcn_wave_barrier();
    cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
    cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
    const float mnew = fmaxf(mrun, cmax);   // finite: key j0 < T is in every chunk
    const float alpha = expf(mrun - mnew);  // 0 at the first chunk
    mrun = mnew;
    lsum *= alpha;
#pragma unroll
    for (int dt = 0; dt < 3; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
    // ---- P^T as the B operand, V as the A operand (dims x keys) ----
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = expf(sc[kt][r] - mnew);
        lsum += p;
        const float* vrow = Vs[16 * kt + 4 * g + r];
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
          const float av = (dt < 2 || c < DH - 32) ? vrow[min(16 * dt + c, DH - 1)] : 0.0f;
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, p, o[dt], 0, 0, 0);
        }
      }
  }
  if (!wave_active) return;
  lsum += __shfl_xor(lsum, 16);
  lsum += __shfl_xor(lsum, 32);
  if (qi >= T) return;
  const float inv = 1.0f / lsum;
  float* dst = O + ((int64_t)b * T + qi) * CF_D + head * DH;
  // o[dt][r] = O^T[dim 16 dt + 4 g + r][query c]
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
    const int d0 = 16 * dt + 4 * g;
    if (d0 < DH)
      *reinterpret_cast<float4*>(dst + d0) =
          make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
  }
}

void launch_cf_relattn_mx(const float* QKV, int B, int T, const float* rk, const float* rwb, const float* rrb,
                          float* O, hipStream_t s) {
  const int nqb = (T + 63) / 64;
  if (B <= 0 || T <= 0 || T > CF_MAX_T || (int64_t)nqb * B * 4 > INT32_MAX)
    return note_launch_error(hipErrorInvalidValue);
  launch_kernel(cf_relattn_mx_kernel, dim3((unsigned)(nqb * B * 4)), 256, s, QKV, T, nqb, rk, rwb, rrb, O);
}

}  // namespace sedx
