// The 14-layer trunk's deep layers: fp32 direct 3x3 conv (pad 1) + folded BN +
// ReLU (+ epilogue) as implicit GEMM on the fp32 matrix pipe, for the layers
// where a Winograd tile is mostly padding: F in {8, 4, 2} bins, 512 / 1024 /
// 2048 channels (block 4's pooled conv2, blocks 5 and 6).
//
//   M = output pixels (clip, t, f), N = output channels, K = 9 taps x Cin.
//
// Tiles.  A workgroup (4 waves) owns 64 pixels of ONE clip - 64 / F whole rows
// of all F bins, starting at an even row - times 128 output channels; wave w
// owns channels 32 w .. 32 w + 31 of them as two 32 x 32 MFMA tiles (pixels
// 0..31 and 32..63).  A tile never crosses a clip, so a halo row outside the
// clip is a zero row, never the neighbouring clip's; a 2x2 pool pair (rows
// 2i, 2i + 1) never straddles a tile; rows past the clip's last (and an odd
// last row under the pool) are computed on zeros / dropped, never stored.
//
// Summation order (the tests' CPU emulation follows it).  Every output is ONE
// in-order fp32 fma chain from zero over K = 9 Cin terms
// (v_mfma_f32_32x32x2_f32: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C))):
//     for chunk in 0 .. Cin/16 - 1:            (16 input channels)
//       for tap in 0 .. 8:                     (tap = 3 dy + dx, row-major)
//         for c in 16 chunk .. 16 chunk + 15:  acc = fma(x[c][t+dy-1][f+dx-1], w[o][c][tap], acc)
// then v = max(acc + bias[o], 0).  K is not split.  The chain does not depend
// on B, on the clip's position in the batch or on the tile a pixel falls in,
// so a clip's outputs are bit-identical across batch sizes.  Epilogues on v:
//   EPI_STORE  v                                             -> [B][T][F][Cout]
//   EPI_POOL2  ((v00 + v01) + (v10 + v11)) * 0.25            -> [B][T/2][F/2][Cout]
//   EPI_FMEAN  (v_0 + v_1 + .. + v_{F-1}, in order) * (1/F)  -> [B][T][Cout]
//
// Staging.  A chunk's zero-bordered halo ((64/F + 2) x (F + 2) pixels x 16
// channels, 20 floats per pixel) goes global -> registers -> LDS through a
// 2-slot ring: the next chunk's loads are in flight while this chunk's 9 x 16
// MFMAs per tile run, one barrier per chunk (seq.hip's linear_kernel shape).
// Weights come straight from global / L2 in pack_conv_deep's layout
// (weights.cpp): a wave reads one (chunk, tap, 4 channels) of its 32 output
// channels as 512 contiguous bytes, one tap ahead of its use.  The workgroups
// of one channel group are consecutive in the grid, so they stream the same
// slab through L2 together.  The ReLU'd tile passes through LDS once for the
// epilogue, which stores 128 consecutive channels per pixel.
//
// Plain grid launch on the caller's stream: no spins, no cross-workgroup
// hand-offs, no counters.
#include "sedx_internal.h"

namespace sedx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int DEEP_BM = 64;            // pixels per workgroup
constexpr int DEEP_PS = DEEP_CK + 4;   // floats per halo pixel in LDS (16 channels + 4 of padding)
constexpr int DEEP_LD = DEEP_BN + 4;   // floats per pixel of the epilogue tile
constexpr int cmax(int a, int b) { return a > b ? a : b; }
}  // namespace

template <int F, int EPI>
__global__ __launch_bounds__(256) void conv_deep_kernel(const float* __restrict__ in, int T, int Cin, int Cout,
                                                        const float4* __restrict__ wd,
                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                        int tiles_per_clip, int in_c4) {
  constexpr int R = DEEP_BM / F;          // rows of a tile
  constexpr int FW = F + 2;               // halo columns
  constexpr int HP = (R + 2) * FW;        // halo pixels
  constexpr int NV = HP * 4;              // float4 of a chunk's halo
  constexpr int NL = (NV + 255) / 256;    // per thread
  constexpr int HALO = HP * DEEP_PS;      // floats per ring slot
  __shared__ __attribute__((aligned(16))) float sm[cmax(2 * HALO, DEEP_BM * DEEP_LD)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, kh = lane >> 5;
  const int b = blockIdx.x / tiles_per_clip;
  const int t0 = (blockIdx.x % tiles_per_clip) * R;
  const int nchunk = Cin / DEEP_CK;

  // ---- this thread's share of a chunk's halo: float4 v = (pixel, channel quad) ----
  int64_t src[NL];   // float offset of chunk 0 (-1: outside the clip, zeros)
  const int64_t cstep = in_c4 ? (int64_t)16 * T * F : 16;   // floats from one chunk to the next
#pragma unroll
  for (int e = 0; e < NL; ++e) {
    const int v = tid + 256 * e, px = v >> 2, q4 = v & 3;
    const int t = t0 + px / FW - 1, f = px % FW - 1;
    const bool ok = v < NV && t >= 0 && t < T && f >= 0 && f < F;
    src[e] = !ok     ? -1
             : in_c4 ? ((((int64_t)b * (Cin / 4) + q4) * T + t) * F + f) * 4
                     : (((int64_t)b * T + t) * F + f) * Cin + 4 * q4;
  }
  float4 hreg[NL];
  auto load_halo = [&](int ch) {
#pragma unroll
    for (int e = 0; e < NL; ++e)
      hreg[e] = src[e] < 0 ? make_float4(0.f, 0.f, 0.f, 0.f)
                           : *reinterpret_cast<const float4*>(in + src[e] + ch * cstep);
  };
  auto store_halo = [&](int slot) {
#pragma unroll
    for (int e = 0; e < NL; ++e) {
      const int v = tid + 256 * e;
      if (v < NV) *reinterpret_cast<float4*>(&sm[slot * HALO + (v >> 2) * DEEP_PS + 4 * (v & 3)]) = hreg[e];
    }
  };

  // ---- weights: this wave's 32 output channels, lane i one of them ----
  const float4* wbase = wd + (int64_t)(blockIdx.y * 4 + wave) * nchunk * (9 * 4 * 32) + i;
  float4 wc[4], wn[4];
  auto load_w = [&](float4* w, int ch, int tap) {
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = wbase[(int64_t)((ch * 9 + tap) * 4 + q) * 32];
  };

  // ---- A fragments: pixel j * 32 + i of the tile, at the halo's (row, col) + tap ----
  int abase[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = j * 32 + i;
    abase[j] = ((p / F) * FW + p % F) * DEEP_PS;
  }
  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

  load_halo(0);
  store_halo(0);
  load_w(wc, 0, 0);
  __syncthreads();
  for (int ch = 0; ch < nchunk; ++ch) {
    const int slot = ch & 1;
    const bool more = ch + 1 < nchunk;
    if (more) load_halo(ch + 1);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (tap < 8)
        load_w(wn, ch, tap + 1);
      else if (more)
        load_w(wn, ch + 1, 0);
      const int toff = ((tap / 3) * FW + tap % 3) * DEEP_PS;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 a0 = *reinterpret_cast<const float4*>(&sm[slot * HALO + abase[0] + toff + 4 * q]);
        const float4 a1 = *reinterpret_cast<const float4*>(&sm[slot * HALO + abase[1] + toff + 4 * q]);
        const float4 w = wc[q];
        // k-step 1: channels 4q (lanes 0-31) and 4q + 1 (lanes 32-63); k-step 2: 4q + 2 and 4q + 3
        const float w01 = kh ? w.y : w.x, w23 = kh ? w.w : w.z;
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? a0.y : a0.x, w01, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? a1.y : a1.x, w01, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? a0.w : a0.z, w23, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? a1.w : a1.z, w23, acc[1], 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) wc[q] = wn[q];
    }
    if (more) store_halo(slot ^ 1);   // slot ^ 1 was last read in chunk ch - 1 (barrier below it)
    __syncthreads();
  }

  // ---- epilogue: relu(acc + bias) through LDS (every halo read is behind the last barrier) ----
  const int n0 = blockIdx.y * DEEP_BN;
  {
    const float bv = bias[n0 + wave * 32 + i];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = j * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        sm[p * DEEP_LD + wave * 32 + i] = fmaxf(acc[j][r] + bv, 0.0f);
      }
  }
  __syncthreads();
  const int c = tid & (DEEP_BN - 1);
  if (EPI == EPI_STORE) {
    for (int p = tid >> 7; p < DEEP_BM; p += 2) {
      const int t = t0 + p / F, f = p % F;
      if (t < T) out[(((int64_t)b * T + t) * F + f) * Cout + n0 + c] = sm[p * DEEP_LD + c];
    }
  } else if (EPI == EPI_POOL2) {
    constexpr int F2 = F / 2;
    const int T2 = T / 2;
    for (int op = tid >> 7; op < DEEP_BM / 4; op += 2) {
      const int orow = op / F2, ocol = op % F2, to = t0 / 2 + orow;
      const float* s = &sm[(2 * orow * F + 2 * ocol) * DEEP_LD + c];
      if (to < T2)
        out[(((int64_t)b * T2 + to) * F2 + ocol) * Cout + n0 + c] =
            ((s[0] + s[DEEP_LD]) + (s[F * DEEP_LD] + s[(F + 1) * DEEP_LD])) * 0.25f;
    }
  } else {
    for (int row = tid >> 7; row < R; row += 2) {
      const int t = t0 + row;
      float sum = sm[row * F * DEEP_LD + c];
#pragma unroll
      for (int f = 1; f < F; ++f) sum += sm[(row * F + f) * DEEP_LD + c];
      if (t < T) out[((int64_t)b * T + t) * Cout + n0 + c] = sum * (1.0f / F);
    }
  }
}

void launch_conv3x3_deep(const float* in, int B, int T, int F, int Cin, int Cout, const float* wd,
                         const float* bias, float* out, int epi, bool in_c4, hipStream_t s) {
  const int rows = epi == EPI_POOL2 ? 2 * (T / 2) : T;
  if (B <= 0 || rows < 1 || Cin % DEEP_CK != 0 || Cout % DEEP_BN != 0 || (F != 8 && F != 4 && F != 2))
    return note_launch_error(hipErrorInvalidValue);
  const int R = DEEP_BM / F, tiles = (rows + R - 1) / R;
  if ((int64_t)B * tiles > INT32_MAX) return note_launch_error(hipErrorInvalidValue);
  const dim3 grid((unsigned)(B * tiles), (unsigned)(Cout / DEEP_BN));
  const float4* w4 = reinterpret_cast<const float4*>(wd);
  const int c4 = in_c4 ? 1 : 0;
#define SEDX_DEEP(FF, EE)                                                                                      \
  if (F == FF && epi == EE)                                                                                    \
    return launch_kernel(conv_deep_kernel<FF, EE>, grid, 256, s, in, T, Cin, Cout, w4, bias, out, tiles, c4)
  SEDX_DEEP(8, EPI_POOL2);
  SEDX_DEEP(4, EPI_STORE);
  SEDX_DEEP(4, EPI_POOL2);
  SEDX_DEEP(2, EPI_STORE);
  SEDX_DEEP(2, EPI_FMEAN);
#undef SEDX_DEEP
  note_launch_error(hipErrorInvalidValue);   // no kernel for this epilogue at this F
}

}  // namespace sedx
