// The VGGish models' own launches for gfx950 (pytorch/models.py:2219-2592), fp32
// in every precision mode: the trunk's first layer and the two heads.  Convs 2-6
// run conv.hip's exact fp32 kernel with its max-pool epilogues (EPI_MAXPOOL2,
// EPI_MAXPOOL2_FMEAN; the summation order is stated in that file's header).
//
// vgg_conv1_kernel: Conv2d(1, 64, 3, padding 1) with bias + ReLU +
// MaxPool2d(2, 2) in one launch.  x [B][T][64] is the raw log-mel (bn0 is never
// applied, models.py:2347-2349), out [B][T/2][32][64] channels-last.  Only the
// pooled tensor is written: the full-resolution 64-channel activation
// [B][T][64][64] (the write that bounds the 9-layer conv1 launches) never
// exists in memory.  The pool floors: with an odd T the last conv row belongs
// to no window and is not computed, but input row T - 1 is still the bottom
// neighbour of conv row T - 2.
//   Summation order of one conv output (t, f, c): taps k = 0..8 in row-major
//   order (k = 3 dt + df, input pixel (t + dt - 1, f + df - 1), zero outside
//   the T x 64 image), one fma chain from zero: s = fma(w[c][k], x_k, s); then
//   v = max(s + bias[c], 0).  The pooled value is the maximum of the four v of
//   its 2x2 window (max is exact: no order).
// One workgroup per (clip, pooled row): the 4 input rows of the row pair with
// their zero border in LDS, thread = (channel c = tid & 63, bin group tid >> 6)
// with w[c][0..8] and the bias in registers; a wave stores 64 consecutive
// channels (256 B) per pooled pixel.
//
// vgg_att_head_kernel (VGGish_FrameAtt, VGGish_Gru_FrameAtt; AttBlock,
// models.py:144-169): per class, a = exp(clamp(att, -10, 10)) + 1e-6 and
// cla = sigmoid(.) of the T sequence frames; tot = the sum of a over t = 0 ..
// T - 1 in ascending order, one fp32 chain from zero; clipwise = the sum over
// t ascending of (a_t * (1 / tot)) * cla_t, one fp32 chain from zero.
// Framewise frame f is cla of sequence frame min(f / ratio, T - 1): x12
// (interpolate, :2375), then the last frame up to 1000 (pad_framewise_output,
// :2376).  emb = cla [B][C][T].
//
// vgg_fc_head_kernel (VGGish_FrameAvg, :2576-2585): p_t = sigmoid(fc logit);
// framewise as above with ratio = 1000 // T.  clipwise is torch.mean over all
// 1000 padded frames: every p_t stands for `ratio` frames and p_(T-1) for the
// npad = 1000 - ratio T padded ones more, so it is
// (ratio * S + npad * p_(T-1)) / 1000 with S = the sum of p_t over t ascending,
// all in float64 (one chain from zero), rounded to fp32 once.
#include "sedx_internal.h"

namespace sedx {

__global__ __launch_bounds__(256) void vgg_conv1_kernel(const float* __restrict__ x, int T, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, float* __restrict__ out) {
  constexpr int F = 64, CS = F + 2;
  __shared__ float xs[4][CS];   // input rows 2 to - 1 .. 2 to + 2, columns -1 .. 64
  const int To = T / 2;
  const int b = blockIdx.x / To, to = blockIdx.x - b * To;
  const int tid = threadIdx.x;
  for (int i = tid; i < 4 * CS; i += 256) {
    const int r = i / CS, c = i - r * CS;
    const int t = 2 * to - 1 + r, f = c - 1;
    xs[r][c] = (t >= 0 && t < T && f >= 0 && f < F) ? x[((int64_t)b * T + t) * F + f] : 0.0f;
  }
  const int c = tid & 63, fq = tid >> 6;
  float w[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = w1[c * 9 + k];
  const float bv = b1[c];
  __syncthreads();
  float* o = out + ((int64_t)b * To + to) * (F / 2) * 64 + c;
#pragma unroll 2
  for (int j = 0; j < 8; ++j) {
    const int fo = fq + 4 * j;   // pooled bin: conv columns 2 fo, 2 fo + 1 = LDS columns 2 fo .. 2 fo + 3
    float win[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) win[r][q] = xs[r][2 * fo + q];
    float m = 0.0f;   // ReLU outputs are >= 0
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int df = 0; df < 2; ++df) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) s = fmaf(w[k], win[dt + k / 3][df + k % 3], s);
        m = fmaxf(m, fmaxf(s + bv, 0.0f));
      }
    o[fo * 64] = m;
  }
}

void launch_vgg_conv1(const float* x, int B, int T, const float* w1, const float* b1, float* out, hipStream_t s) {
  if (B <= 0 || T < 2 || (int64_t)B * (T / 2) > INT32_MAX) return note_launch_error(hipErrorInvalidValue);
  launch_kernel(vgg_conv1_kernel, dim3(B * (T / 2)), 256, s, x, T, w1, b1, out);
}

namespace {
constexpr int VGG_TC = 128;   // sequence frames staged at a time
__device__ __forceinline__ float vgg_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
}  // namespace

// one workgroup per clip; classes in chunks of 32, thread = (class cc = tid & 31, frame lane tq = tid >> 5)
__global__ __launch_bounds__(256) void vgg_att_head_kernel(const float* __restrict__ logits, int T, int C, int ldl,
                                                           int out_frames, int ratio, float* __restrict__ fw,
                                                           float* __restrict__ clip, float* __restrict__ emb) {
  __shared__ float s_att[VGG_TC][33];   // exp(clamp(att)) + 1e-6
  __shared__ float s_cla[VGG_TC][33];   // sigmoid(cla)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cc = tid & 31, tq = tid >> 5;
  const float* lg = logits + (int64_t)b * T * ldl;
  for (int c0 = 0; c0 < C; c0 += 32) {
    const int nc = min(32, C - c0);
    __syncthreads();   // the previous chunk's readers are done
    if (cc < nc)
      for (int t = tq; t < T; t += 8) {
        const float a = lg[(int64_t)t * ldl + c0 + cc];
        s_att[t][cc] = expf(fminf(fmaxf(a, -10.0f), 10.0f)) + 1e-6f;
        s_cla[t][cc] = vgg_sigmoid(lg[(int64_t)t * ldl + C + c0 + cc]);
      }
    __syncthreads();
    if (tid < nc) {
      float tot = 0.0f;
      for (int t = 0; t < T; ++t) tot += s_att[t][tid];
      const float inv_tot = 1.0f / tot;
      float acc = 0.0f;
      for (int t = 0; t < T; ++t) acc += (s_att[t][tid] * inv_tot) * s_cla[t][tid];
      clip[(int64_t)b * C + c0 + tid] = acc;
    }
    if (cc < nc)
      for (int f = tq; f < out_frames; f += 8)
        fw[((int64_t)b * out_frames + f) * C + c0 + cc] = s_cla[min(f / ratio, T - 1)][cc];
    if (emb)
      for (int i = tid; i < nc * T; i += 256) {
        const int k = i / T, t = i - k * T;
        emb[((int64_t)b * C + c0 + k) * T + t] = s_cla[t][k];
      }
  }
}

void launch_vgg_att_head(const float* logits, int B, int T, int C, int ldl, int out_frames, int ratio,
                         float* framewise, float* clipwise, float* emb_cla, hipStream_t s) {
  // the whole sequence is staged at once: 1000 / 12 = 83 frames at most
  if (B <= 0 || T <= 0 || T > VGG_TC || C <= 0 || ldl < 2 * C || ratio <= 0 || (int64_t)ratio * T > out_frames)
    return note_launch_error(hipErrorInvalidValue);
  hipLaunchKernelGGL(vgg_att_head_kernel, dim3(B), dim3(256), 0, s, logits, T, C, ldl, out_frames, ratio, framewise,
                     clipwise, emb_cla);
}

__global__ __launch_bounds__(256) void vgg_fc_head_kernel(const float* __restrict__ logits, int T, int C, int ldl,
                                                          int out_frames, int ratio, float* __restrict__ fw,
                                                          float* __restrict__ clip) {
  __shared__ float s_p[VGG_TC][33];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cc = tid & 31, tq = tid >> 5;
  const float* lg = logits + (int64_t)b * T * ldl;
  const int npad = out_frames - ratio * T;   // frames past ratio T repeat the last one
  for (int c0 = 0; c0 < C; c0 += 32) {
    const int nc = min(32, C - c0);
    double sum = 0.0;
    for (int t0 = 0; t0 < T; t0 += VGG_TC) {
      const int nt = min(VGG_TC, T - t0);
      __syncthreads();   // the previous chunk's readers are done
      if (cc < nc)
        for (int t = tq; t < nt; t += 8) s_p[t][cc] = vgg_sigmoid(lg[(int64_t)(t0 + t) * ldl + c0 + cc]);
      __syncthreads();
      if (tid < nc)
        for (int t = 0; t < nt; ++t) sum += (double)s_p[t][tid];
      if (cc < nc) {
        for (int fr = tq; fr < nt * ratio; fr += 8)
          fw[((int64_t)b * out_frames + (int64_t)t0 * ratio + fr) * C + c0 + cc] = s_p[fr / ratio][cc];
        if (t0 + nt == T)
          for (int f = ratio * T + tq; f < out_frames; f += 8)
            fw[((int64_t)b * out_frames + f) * C + c0 + cc] = s_p[nt - 1][cc];
      }
      if (tid < nc && t0 + nt == T)
        clip[(int64_t)b * C + c0 + tid] =
            (float)(((double)ratio * sum + (double)npad * (double)s_p[nt - 1][tid]) / (double)out_frames);
    }
  }
}

void launch_vgg_fc_head(const float* logits, int B, int T, int C, int ldl, int out_frames, int ratio,
                        float* framewise, float* clipwise, hipStream_t s) {
  if (B <= 0 || T <= 0 || C <= 0 || ldl < C || ratio <= 0 || (int64_t)ratio * T > out_frames)
    return note_launch_error(hipErrorInvalidValue);
  hipLaunchKernelGGL(vgg_fc_head_kernel, dim3(B), dim3(256), 0, s, logits, T, C, ldl, out_frames, ratio, framewise,
                     clipwise);
}

}  // namespace sedx
