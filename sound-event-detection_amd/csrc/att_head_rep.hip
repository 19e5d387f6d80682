// AttBlock finish for any frame repeat ratio, gfx950 (Cnn_14layers_Conformer_FrameAtt, pytorch/models.py:1786-1794;
// AttBlock :161-175, interpolate :84-95, pad_framewise_output :65-81).  att_head_kernel (seq.hip) takes the ratio
// as a shift (8 or 32); this model repeats each of its T <= 1000 sequence frames 1000 // T times: 1000, 500, 333,
// 66, 32, 7, 2, 1.  A kernel of its own, so the other models' launches and their bits stay what they are.
//
// logits [B][T][ldl]: columns 0..C-1 att, C..2C-1 cla.  One workgroup of 256 threads per clip, classes in groups
// of 32, the sequence in staging chunks of 128 frames (att and cla of a chunk land in LDS by coalesced loads).
//
// Arithmetic and the order of every sum, per (clip, class), all fp32.  Thread (class slot cs = tid / 8, t-lane
// l = tid % 8):
//   a_t   = E(min(max(att_t, -10), 10)) + 1e-6, E(x) = e^x by the operations listed at rep_exp_ below (range
//           reduction by ln 2 in two parts, a degree-5 polynomial as an fma chain, ldexp: within 1 ulp of expf
//           on [-10, 10]); spelled out, not expf, so that a host can reproduce a_t, tot and clipwise bit for bit
//           from the logits (tests/conformer14_refs.py does)
//   p_l   = a_l + a_(l+8) + a_(l+16) + ...             ascending t over the whole sequence, from 0.0f
//   tot   = ((p_0 + p_1) + (p_2 + p_3)) + ((p_4 + p_5) + (p_6 + p_7))
//   s_t   = 1 / (1 + expf(-cla_t))                      the framewise value
//   q_l   = fma(a_t * (1 / tot), s_t, q_l) over t = l, l + 8, ... ascending, from 0.0f
//   clipwise = ((q_0 + q_1) + (q_2 + q_3)) + ((q_4 + q_5) + (q_6 + q_7))
// (the three xor-shuffle steps 1, 2, 4 give every lane that tree; fp32 addition commutes, so all 8 lanes hold
// the same bits).  The chunks of 128 are a multiple of 8, so lane l's frames are t = l (mod 8) in every chunk.
// clipwise sums over the T sequence frames, never over the padded ones.
//
// framewise [B][out_frames][C]: frame f = s of sequence frame min(f / ratio, T - 1).  No division runs: the
// kernel walks the sequence frames and writes `ratio` copies of each (ratio >= 8: the 8 row lanes take the copies
// of one frame; below 8: the row lanes take 8 frames and each writes its copies), then the last frame from
// ratio T up to out_frames.  A row's C values are stored by consecutive lanes, rows are contiguous in memory.
#include "sedx_internal.h"

namespace sedx {

namespace {
// e^x for |x| <= 10, every operation written out (one rounding each; fmaf = one fused multiply-add):
//   n = rint(x * log2(e)) to nearest-even;  r = fma(n, -0.693359375, x);  r = fma(n, 2.12194440e-4, r)
//   p = c0;  p = fma(p, r, c_i) for c1 .. c5;  y = fma(p, r * r, r) + 1;  E = ldexp(y, n)
__device__ __forceinline__ float rep_exp_(float x) {
  const float n = rintf(x * 1.44269504088896341f);
  float r = fmaf(n, -0.693359375f, x);
  r = fmaf(n, 2.12194440e-4f, r);
  float p = 1.9875691500e-4f;
  p = fmaf(p, r, 1.3981999507e-3f);
  p = fmaf(p, r, 8.3334519073e-3f);
  p = fmaf(p, r, 4.1665795894e-2f);
  p = fmaf(p, r, 1.6666665459e-1f);
  p = fmaf(p, r, 5.0000001201e-1f);
  const float r2 = r * r;
  const float y = fmaf(p, r2, r) + 1.0f;
  return ldexpf(y, (int)n);
}
__device__ __forceinline__ float rep_att_exp_(float a) { return rep_exp_(fminf(fmaxf(a, -10.0f), 10.0f)) + 1e-6f; }
__device__ __forceinline__ float rep_sum8_(float v) {   // over the 8 lanes of a class
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}
}  // namespace

__global__ __launch_bounds__(256) void att_head_rep_kernel(const float* __restrict__ logits, int T, int C, int ldl,
                                                           int out_frames, int ratio, float* __restrict__ fw,
                                                           float* __restrict__ clip) {
  // row stride 36: the reductions read [t = l + 8 k][cs] with (l, cs) = (lane & 7, lane >> 3): bank 4 l + cs is
  // distinct over a half wave's 8 x 4 lanes (at 33 floats it would be l + cs, 8 lanes on a bank); the staging
  // and the stores read and write a row's 32 consecutive floats either way
  constexpr int TC = 128, LD = 36;
  __shared__ float s_att[TC][LD];
  __shared__ float s_cla[TC][LD];   // cla logits, then sigmoid(cla)
  __shared__ float s_last[32];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cs = tid >> 3, l = tid & 7;
  const int cc = tid & 31, rl = tid >> 5;   // the stores' class lane and row lane
  const float* lg = logits + (int64_t)b * T * ldl;
  float* fwb = fw + (int64_t)b * out_frames * C;
  for (int c0 = 0; c0 < C; c0 += 32) {
    const int nc = min(32, C - c0);
    const bool act = cs < nc;
    auto stage = [&](int t0, int nt) {
      __syncthreads();
      const int j = tid & 63, half = j >> 5, sc = j & 31;
      if (sc < nc)
        for (int t = tid >> 6; t < nt; t += 4) {
          const float v = lg[(int64_t)(t0 + t) * ldl + half * C + c0 + sc];
          if (half) s_cla[t][sc] = v;
          else s_att[t][sc] = v;
        }
      __syncthreads();
    };
    // pass 1: tot
    float sum = 0.f;
    for (int t0 = 0; t0 < T; t0 += TC) {
      const int nt = min(TC, T - t0);
      stage(t0, nt);
      if (act)
        for (int t = l; t < nt; t += 8) sum += rep_att_exp_(s_att[t][cs]);
    }
    sum = rep_sum8_(sum);
    const float inv_tot = 1.0f / sum;
    // pass 2: clipwise, and sigmoid(cla) of a chunk -> its ratio x nt framewise rows
    float acc = 0.f;
    for (int t0 = 0; t0 < T; t0 += TC) {
      const int nt = min(TC, T - t0);
      if (T > TC) stage(t0, nt);   // else still staged from pass 1
      if (act)
        for (int t = l; t < nt; t += 8) {
          const float cl = 1.0f / (1.0f + expf(-s_cla[t][cs]));
          acc = fmaf(rep_att_exp_(s_att[t][cs]) * inv_tot, cl, acc);
          s_cla[t][cs] = cl;
        }
      __syncthreads();
      if (cc < nc) {
        // row (t0 + t) ratio + r of the clip: below ratio T <= out_frames
        float* dst = fwb + (int64_t)t0 * ratio * C + c0 + cc;
        if (ratio >= 8) {
          for (int t = 0; t < nt; ++t, dst += (int64_t)ratio * C) {
            const float v = s_cla[t][cc];
            for (int r = rl; r < ratio; r += 8) dst[(int64_t)r * C] = v;
          }
        } else {
          dst += (int64_t)rl * ratio * C;
          for (int t = rl; t < nt; t += 8, dst += (int64_t)8 * ratio * C) {
            const float v = s_cla[t][cc];
            for (int r = 0; r < ratio; ++r) dst[(int64_t)r * C] = v;
          }
        }
      }
      if (t0 + nt == T && tid < nc) s_last[tid] = s_cla[nt - 1][tid];
    }
    acc = rep_sum8_(acc);
    if (act && l == 0) clip[(int64_t)b * C + c0 + cs] = acc;
    __syncthreads();
    if (cc < nc)   // the last frame, repeated from ratio T up to out_frames
      for (int f = T * ratio + rl; f < out_frames; f += 8) fwb[(int64_t)f * C + c0 + cc] = s_last[cc];
  }
}

void launch_att_head_rep(const float* logits, int B, int T, int C, int ldl, int out_frames, int ratio,
                         float* framewise, float* clipwise, hipStream_t s) {
  // every framewise store lands below out_frames rows: ratio T <= out_frames
  if (B <= 0 || T < 1 || T > 1000 || C < 1 || ldl < 2 * C || ratio < 1 || (int64_t)ratio * T > out_frames ||
      out_frames > 1000)
    return note_launch_error(hipErrorInvalidValue);
  launch_kernel(att_head_rep_kernel, dim3(B), 256, s, logits, T, C, ldl, out_frames, ratio, framewise, clipwise);
}

}  // namespace sedx
