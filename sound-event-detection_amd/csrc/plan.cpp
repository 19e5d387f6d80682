// plan.h: the forward plan and the windowed drivers' layout (host only).
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace sedx {

Geometry geometry_from_T(const Model& m, int64_t T) {
  Geometry g;
  g.T = T;
  g.T1 = T / 2;
  g.T2 = g.T1 / 2;
  g.T3 = g.T2 / 2;
  g.fw_len = 8 * g.T3;
  g.out_frames = g.fw_len;
  // pad_framewise_output(roundup) models.py:678-681: Cnn_9layers_Gru_FrameAtt
  // (Cnn_9layers_Gru_FrameAvg returns the 8 T3 frames, :551) and the two
  // Conformer models (:1359-1360, :1571-1572)
  const bool pad100 = m.cfg.model_type == SEDX_MODEL_GRU_FRAMEATT || m.seq == SEQ_CONFORMER;
  if (pad100 && g.fw_len != 1000)
    g.out_frames = (g.fw_len % 100 == 0) ? g.fw_len : g.fw_len + 100 - g.fw_len % 100;
  return g;
}

namespace {
// the next region of `floats` floats (or ints)
Region take(size_t& end, size_t floats) { return Region{carve(end, floats * 4) / 4, floats}; }
}  // namespace

const char* plan_forward(const Model& m, const Tuning& t, int64_t B, int64_t T, ForwardPlan* p) {
  const Geometry g = geometry_from_T(m, T);
  p->g = g;
  p->B = B;
  p->M = (int)(B * g.T3);
  // ---- which kernels ----
  const bool wino = t.precision == SEDX_PRECISION_WINOGRAD, x3 = t.precision == SEDX_PRECISION_X3;
  // Winograd block 1 (SEDX_TUNE_WINO_BLOCK1): 1 = conv1's activation
  // [B][T][64][64] into A by its own launch; 2 = conv1 inside the F(2x2,3x3)
  // launch.  F(4x4,3x3) block 1 (SEDX_TUNE_WINO_F43 2): conv1 by its own
  // launch in both (2: in the chunk-of-4 layout), then the F(4x4,3x3) conv2
  if (x3) p->block1 = B1_PAD_X3;
  else if (!wino || t.wino_block1 == 0) p->block1 = B1_PAD_EXACT;
  else if (t.wino_f43 == 2) p->block1 = t.wino_block1 == 2 ? B1_CONV1C4_F43 : B1_CONV1_F43;
  else p->block1 = t.wino_block1 == 2 ? B1_F23_FUSED : B1_CONV1_F23;
  p->family = x3 ? CONV_X3 : !wino ? CONV_EXACT : t.wino_f43 ? CONV_WINO43 : CONV_WINO;
  p->c4 = wino && t.wino_f43 && t.wino_block1 == 2;
  p->claims = x3 || (p->family == CONV_WINO43 && B >= 8);
  // AUTO: 16 slices (half the recurrence's serial product); on a pipelined
  // handle dealt over every XCD (spread, below): beside the next batch's conv
  // stack the shorter recurrence then costs it less than the 8-slice kernel's
  // half-size footprint (12,238-12,303 vs 11,886-11,923 clips/s, profiles/r05za_*)
  static const int variant[8] = {2, -1, 0, 1, 3, 3, 4, 5};   // COOP, SIMPLE, TAG16, TAG8, COOP16, AUTO, KSPLIT, PAIR
  p->gru_variant = variant[t.gru_kernel];
  p->gru_fast = t.gru_handoff == SEDX_GRU_HANDOFF_AUTO || t.gru_handoff == SEDX_GRU_HANDOFF_LOCAL;
  // AUTO on a pipelined handle: the recurrence runs beside the next batch's
  // conv stack, whose items are dealt to the 8 XCDs evenly — slices on one
  // XCD cost that XCD a quarter of its CUs and the whole launch waits for it
  // (b1c2 0.61 vs 0.51 ms in the timed region, profiles/r05t_*)
  p->gru_spread = t.gru_handoff == SEDX_GRU_HANDOFF_SPREAD || (t.gru_handoff == SEDX_GRU_HANDOFF_AUTO && t.pipelined);
  // ---- where ----
  size_t end = 0;
  p->x0 = take(end, (size_t)B * T * 64);
  const size_t a0 = end;   // A starts here; its three phases (conv stack, head, Conformer) each carve from it
  // conv stack: block 1's first launch into A, then the layers ping-pong P / A
  size_t a_conv = p->block1 == B1_F23_FUSED                             ? 0
                  : p->block1 == B1_PAD_EXACT || p->block1 == B1_PAD_X3 ? block1_pad_floats((int)B, (int)T)
                                                                         : (size_t)B * T * 64 * 64;
  size_t p_conv = 0;
  const int64_t Ts[4] = {g.T, g.T1, g.T2, g.T3};
  for (int i = 0; i < 7; ++i) {
    const int blk = (i + 1) / 2, cout = 64 << blk, Tl = (int)Ts[blk], F = 64 >> blk, pool = i % 2 == 0 && i < 6;
    p->layers[i] = ConvLayer{Tl, F, i == 0 ? 64 : i % 2 ? cout / 2 : cout, cout,
                             i == 6 ? EPI_FMEAN : pool ? EPI_POOL2 : EPI_STORE,
                             pool ? Tl / 2 : Tl, i == 6 ? 1 : pool ? F / 2 : F, 0, 0};
    size_t& ext = i % 2 ? a_conv : p_conv;
    ext = std::max(ext, (size_t)B * p->layers[i].To * p->layers[i].Fo * cout);
  }
  const size_t M = (size_t)p->M;
  size_t e_head = a0;
  p->G = take(e_head, M * 1536);
  p->Hs = take(e_head, M * 512);
  p->O = take(e_head, M * 512);
  p->LG = take(e_head, M * m.nac);
  p->gru = take(e_head, gru_coop_workspace_bytes((int)B) / 4);
  size_t e_a = std::max(a0 + align256(a_conv * 4), e_head);
  if (m.seq == SEQ_CONFORMER) {
    size_t e_cf = a0;
    p->X = take(e_cf, M * CF_D);
    p->Xn = take(e_cf, M * CF_D);
    p->Hb = take(e_cf, M * CF_FF);
    p->AV = take(e_cf, M * CF_D);
    p->Rr = take(e_cf, (size_t)CF_BLOCKS * g.T3 * CF_D);
    p->RK = take(e_cf, (size_t)CF_BLOCKS * g.T3 * CF_D);
    p->LG = take(e_cf, M * m.nac);
    e_a = std::max(e_a, e_cf);
  }
  p->A = Region{a0 / 4, (e_a - a0) / 4};
  end = e_a;
  p->P = take(end, p_conv);
  p->sched = take(end, 7 * CONV_SCHED_INTS);
  p->total_bytes = end;
  for (int i = 0; i < 7; ++i) {
    p->layers[i].in = i % 2 ? p->P.off : p->A.off;
    p->layers[i].out = i % 2 ? p->A.off : p->P.off;
  }
  if (p->block1 == B1_F23_FUSED) p->layers[0].in = p->x0.off;
  // ---- shapes no forward runs ----
  p->reject[0] = 0;
  if (g.T3 < 1) snprintf(p->reject, sizeof(p->reject), "input too short for the 3 pooling stages");
  else if (seq_too_long(m, g.T3))
    snprintf(p->reject, sizeof(p->reject), "%lld sequence frames: the Conformer encoder holds %d", (long long)g.T3,
             CF_MAX_T);
  else if (B * g.T > INT32_MAX / 64) snprintf(p->reject, sizeof(p->reject), "batch too large");   // 32-bit launch sizes
  return p->reject[0] ? p->reject : nullptr;
}

const char* window_geometry(const Model& m, int64_t L_clip, const sedx_window_spec* spec, bool avg, WinGeom* wg) {
  if (!spec) return "null window spec";
  const int sr = m.cfg.sample_rate;
  if (const char* why = window_loop(sr, L_clip, *spec, &wg->loop)) return why;
  // int(100 * overlap_value) in float64 (utilities.py:406, :426)
  const double stepd = 100.0 * spec->overlap_value;
  if (!(std::fabs(stepd) < 1e9)) return "overlap_value out of range";
  wg->step = (int64_t)stepd;
  wg->sd = spec->sample_duration;
  wg->n_win = (int)wg->loop.start.size();
  wg->full_len = (int64_t)spec->sample_duration * sr;
  wg->clip_len = spec->driver == SEDX_DRIVER_MAIN_STRONG ? std::min<int64_t>(L_clip, (int64_t)sr * 10) : L_clip;
  wg->groups.clear();
  std::vector<int64_t> frames(wg->n_win);
  auto refuse = [&](const char* fmt, int w, long long n, int k) {
    snprintf(wg->reject, sizeof(wg->reject), fmt, w, n, k);
    return wg->reject;
  };
  for (int w = 0; w < wg->n_win; ++w) {
    const int64_t len = wg->loop.len[w];
    // the model raises on these windows: STFT reflect padding needs more
    // than n_fft/2 samples (stft.py:237), the third 2x2 pool one frame
    // (models.py:139)
    if (len <= m.cfg.window_size / 2)
      return refuse("window %d has %lld samples: too short for the STFT's reflect padding", w, (long long)len, 0);
    if (wg->groups.empty() || wg->groups.back().len != len) {
      WinGroup g;
      g.w0 = w;
      g.len = len;
      g.g = geometry_from_T(m, conv_T(m, len));
      if (g.g.T3 < 1) return refuse("window %d too short for the CNN", w, 0, 0);
      if (seq_too_long(m, g.g.T3))
        return refuse("window %d gives %lld sequence frames: the Conformer encoder holds %d", w, (long long)g.g.T3,
                      CF_MAX_T);
      wg->groups.push_back(g);
    }
    ++wg->groups.back().nw;
    frames[w] = wg->groups.back().g.out_frames;
  }
  return build_merge_plan(frames, wg->step, wg->sd, avg, &wg->plan);
}

WinLayout win_layout(const Model& m, const Tuning& t, int64_t n_clips, const WinGeom& wg) {
  WinLayout l;
  const size_t C = m.cfg.classes_num;
  ForwardPlan fp;
  for (const auto& g : wg.groups) {
    plan_forward(m, t, n_clips * g.nw, g.g.T, &fp);
    l.model_bytes = std::max(l.model_bytes, fp.total_bytes);
  }
  size_t end = l.model_bytes;
  for (const auto& g : wg.groups) l.fw_off.push_back(take(end, (size_t)n_clips * g.nw * g.g.out_frames * C).off);
  for (const auto& g : wg.groups) l.clip_off.push_back(take(end, (size_t)n_clips * g.nw * C).off);
  l.vthr = take(end, 2 * C).off;   // [C] f64
  l.tables = end / 4;
  size_t b = 0;
  l.t_start = carve(b, 8 * (size_t)wg.n_win);
  l.t_wb = carve(b, 8 * (size_t)wg.n_win);
  l.t_wcs = carve(b, 8 * (size_t)wg.n_win);
  l.t_off = carve(b, 4 * ((size_t)wg.plan.N + 1));
  l.t_src = carve(b, 8 * wg.plan.src.size());
  l.t_div = carve(b, 4 * (size_t)wg.plan.N);
  l.table_bytes = b;
  l.total_bytes = end + b;
  return l;
}

}  // namespace sedx
