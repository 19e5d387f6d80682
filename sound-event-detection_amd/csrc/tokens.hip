// Cnn_9layers_Conformer's two copy kernels for gfx950 (pytorch/models.py:2159-2164, :2177-2179).  No arithmetic
// in either: every output float is one input float.
//
//   tokens_kernel      the Conformer encoder's input S [B][Ts][512], Ts = 8 T3 + 1.  Row 0 of every clip is the
//                      tag token (linear_emb on a tensor of ones, folded on the host: pack_tag_token,
//                      weights.cpp); row 1 + 8 t + f is pixel (t, f) of block 4's conv2 output -- the
//                      reference's reshape(B, 512, T3 * 8) and permute.  The pixels come from the chunk-of-4
//                      layout [B][128][T3][8][4] (C4: a 32 token x 32 chunk tile goes through LDS, so both the
//                      reads and the writes are 512-byte runs) or from [B][T3][8][512] (a shifted copy).
//   token_head_kernel  logits [B][Ts][ldl] -> clipwise [B][C] (token 0) and framewise [B][Ts - 1][C]
//                      (tokens 1..), columns 0..C-1.
#include "sedx_internal.h"

namespace sedx {

// grid (ceil(Ts / 32), 4, B), 256 threads.  C4: block y moves chunks 32 y .. 32 y + 31 of tokens 32 x .. 32 x + 31:
// thread (a = tid / 32, l = tid % 32) reads token l of chunks a, a + 8, a + 16, a + 24 and writes chunk l of
// tokens a, a + 8, a + 16, a + 24.  !C4: block y moves floats 128 y .. 128 y + 127 of the same tokens.
template <bool C4>
__global__ __launch_bounds__(256) void tokens_kernel(const float4* __restrict__ in, int T3, int Ts,
                                                     const float4* __restrict__ tag, float4* __restrict__ S) {
  __shared__ float4 tile[32][33];
  const int l = threadIdx.x & 31, a = threadIdx.x >> 5;
  const int tok0 = blockIdx.x * 32, q0 = blockIdx.y * 32, b = blockIdx.z;
  const int npx = 8 * T3;   // pixels of a clip = Ts - 1
  float4* Sb = S + (int64_t)b * Ts * 128;
  if (C4) {
    const float4* inb = in + (int64_t)b * 128 * npx;
    const int tok = tok0 + l;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = q0 + a + 8 * k;
      if (tok < Ts) tile[a + 8 * k][l] = tok == 0 ? tag[q] : inb[(int64_t)q * npx + tok - 1];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = tok0 + a + 8 * k;
      if (t < Ts) Sb[(int64_t)t * 128 + q0 + l] = tile[l][a + 8 * k];
    }
  } else {
    const float4* inb = in + (int64_t)b * npx * 128;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = tok0 + a + 8 * k, q = q0 + l;
      if (t < Ts) Sb[(int64_t)t * 128 + q] = t == 0 ? tag[q] : inb[(int64_t)(t - 1) * 128 + q];
    }
  }
}

void launch_tokens(const float* in, int B, int T3, bool c4, const float* tag, float* S, hipStream_t s) {
  if (B <= 0 || T3 <= 0 || B > 65535 || 8 * (int64_t)T3 + 1 > CF_MAX_T) return note_launch_error(hipErrorInvalidValue);
  const int Ts = 8 * T3 + 1;
  const dim3 grid((Ts + 31) / 32, 4, B);
  const float4* in4 = reinterpret_cast<const float4*>(in);
  const float4* tag4 = reinterpret_cast<const float4*>(tag);
  float4* S4 = reinterpret_cast<float4*>(S);
  if (c4) launch_kernel(tokens_kernel<true>, grid, 256, s, in4, T3, Ts, tag4, S4);
  else launch_kernel(tokens_kernel<false>, grid, 256, s, in4, T3, Ts, tag4, S4);
}

// one thread per output float: e < B Ts C, (b, t, c) = (e / (Ts C), e / C % Ts, e % C)
__global__ __launch_bounds__(256) void token_head_kernel(const float* __restrict__ logits, int Ts, int C, int ldl,
                                                         int64_t total, float* __restrict__ framewise,
                                                         float* __restrict__ clipwise) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const int64_t row = e / C;   // b Ts + t
  const int t = (int)(row % Ts);
  const int64_t b = row / Ts;
  const float v = logits[row * ldl + c];
  if (t == 0) clipwise[b * C + c] = v;
  else framewise[(b * (Ts - 1) + t - 1) * C + c] = v;
}

void launch_token_head(const float* logits, int B, int Ts, int C, int ldl, float* framewise, float* clipwise,
                       hipStream_t s) {
  const int64_t total = (int64_t)B * Ts * C;
  if (B <= 0 || Ts < 2 || C <= 0 || C > ldl || (total + 255) / 256 > INT32_MAX)
    return note_launch_error(hipErrorInvalidValue);
  launch_kernel(token_head_kernel, dim3((unsigned)((total + 255) / 256)), 256, s, logits, Ts, C, ldl, total, framewise,
                clipwise);
}

}  // namespace sedx
