// plan.h: the forward plan and the windowed drivers' layout (host only).
#include "plan.h"

#include "wino_geom.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace sedx {

Geometry geometry_from_T(const Model& m, int64_t T) {
  const FrameRule& r = m.frames;
  Geometry g;
  g.T = T;
  g.T1 = T / 2;
  g.T2 = g.T1 / 2;
  g.T3 = g.T2 / 2;
  g.T4 = g.T3 / 2;
  g.T5 = g.T4 / 2;
  g.Ts = r.pools == 3 ? g.T3 : r.pools == 4 ? g.T4 : g.T5;
  // a fixed repeat, or 1000 // seq_len; shapes no forward runs keep -rep
  g.rep = r.rep > 0 ? r.rep : g.Ts >= 1 && g.Ts <= r.max_seq ? (int)(1000 / g.Ts) : -r.rep;
  g.fw_len = g.rep * g.Ts;
  // the tag token and every (frame, bin) pixel of block 4: one output frame per pixel token
  if (r.tokens) g.Ts = g.T3 >= 1 ? r.tokens * g.T3 + 1 : 0, g.fw_len = r.tokens * g.T3;
  g.out_frames = g.fw_len;
  if (r.pad == PAD_TO_1000) g.out_frames = 1000;
  else if (r.pad == PAD_TO_100 && g.fw_len != 1000 && g.fw_len % 100 != 0) g.out_frames = g.fw_len + 100 - g.fw_len % 100;
  // where the model has no output (too few frames, a multiple of 32: refused by every caller) the repeated frames stand
  else if (r.pad == PAD_TO_T_LESS_1 && g.Ts >= 1 && T % 32 != 0) g.out_frames = T - 1;
  return g;
}

const char* shape_refusal(const Model& m, int64_t T, char* buf, size_t n) {
  const FrameRule& r = m.frames;
  const long long seq = geometry_from_T(m, T).Ts;
  if (seq < 1 && m.vgg)
    snprintf(buf, n, "%lld frames: the VGGish trunk's %d pooling stages need %d", (long long)T, r.pools, 1 << r.pools);
  else if (seq < 1) snprintf(buf, n, "input too short for the %d pooling stages", r.pools);
  else if (r.pad == PAD_TO_T_LESS_1 && T % 32 == 0)
    snprintf(buf, n, "%lld frames: a multiple of 32 has no output (the reference pads by -1 frames)", (long long)T);
  else if (seq <= r.max_seq) return nullptr;
  else if (r.pad == PAD_TO_1000 && r.rep > 0)
    snprintf(buf, n, "%lld sequence frames: x%d passes the 1000-frame output (at most %d)", seq, r.rep, r.max_seq);
  else if (r.pad == PAD_TO_1000) snprintf(buf, n, "%lld sequence frames: VGGish_FrameAvg has 1000 output frames", seq);
  else if (r.rep < 0) snprintf(buf, n, "%lld sequence frames: more than %d leave no framewise output", seq, r.max_seq);
  else snprintf(buf, n, "%lld sequence frames: the Conformer encoder holds %d", seq, r.max_seq);
  return buf;
}

namespace {
// the next region of `floats` floats (or ints)
Region take(size_t& end, size_t floats) { return Region{carve(end, floats * 4) / 4, floats}; }
}  // namespace

// ---- a gamma model's own frontend ---------------------------------------------
int64_t audio_T(const Model& m, int64_t L) {
  if (m.cfg.feature_type != SEDX_FEATURE_GAMMA) return conv_T(m, L);
  GammaGeom gg;
  gamma_geometry(m.cfg.sample_rate, m.cfg.window_size, m.cfg.hop_size, &gg);
  return L < gg.nfft || gg.hop < 1 ? 0 : 1 + (L - gg.nfft) / gg.hop;
}

const char* audio_refusal(const Model& m, int64_t L, char* buf, size_t n) {
  if (m.cfg.feature_type == SEDX_FEATURE_GAMMA) {
    GammaGeom gg;
    gamma_geometry(m.cfg.sample_rate, m.cfg.window_size, m.cfg.hop_size, &gg);
    if (L >= gg.nfft) return nullptr;
    snprintf(buf, n, "input of %lld samples is shorter than the gammatone FFT (%d)", (long long)L, gg.nfft);
    return buf;
  }
  // STFT reflect padding needs more than n_fft / 2 samples (stft.py:237)
  if (L > m.cfg.window_size / 2) return nullptr;
  snprintf(buf, n, "input of %lld samples is too short for reflect padding of %d", (long long)L, m.cfg.window_size / 2);
  return buf;
}

size_t frontend_bytes(const Model& m, int64_t items, int64_t L) {
  if (m.cfg.feature_type != SEDX_FEATURE_GAMMA) return 0;
  GammaGeom gg;
  gamma_geometry(m.cfg.sample_rate, m.cfg.window_size, m.cfg.hop_size, &gg);
  if (items < 1 || L < gg.nfft || gg.hop < 1) return 0;
  return gamma_layout(items, L, gg.nfft, gg.hop).total_bytes;
}

AudioLayout audio_layout(const Model& m, const Tuning& t, int64_t B, int64_t L) {
  AudioLayout l;
  ForwardPlan fp;
  plan_forward(m, t, B, audio_T(m, L), &fp);
  l.model_bytes = fp.total_bytes;
  l.fe_bytes = frontend_bytes(m, B, L);
  if (!l.fe_bytes) {   // a log-mel model: the forward's own workspace
    l.total_bytes = l.model_bytes;
    return l;
  }
  size_t end = align256(l.model_bytes);
  l.fe = carve(end, l.fe_bytes);
  l.total_bytes = end;
  return l;
}

const char* plan_forward(const Model& m, const Tuning& t, int64_t B, int64_t T, ForwardPlan* p) {
  const Geometry g = geometry_from_T(m, T);
  p->g = g;
  p->B = B;
  p->M = (int)(B * g.Ts);
  const bool deep = m.depth == 14;
  p->nlayers = m.vgg ? VGG_LAYERS - 1 : deep ? 11 : 7;
  p->first_deep = m.vgg ? p->nlayers : deep ? 6 : 7;
  // ---- which kernels ----
  const bool wino = t.precision == SEDX_PRECISION_WINOGRAD, x3 = t.precision == SEDX_PRECISION_X3;
  // fp16 conv stack: the packed layers on conv_f16.hip, everything else (sequence layer, head) as in exact
  const bool f16 = t.precision == SEDX_PRECISION_F16;
  // Winograd block 1 (SEDX_TUNE_WINO_BLOCK1): 1 = conv1's activation
  // [B][T][64][64] into A by its own launch; 2 = conv1 inside the F(2x2,3x3)
  // launch.  F(4x4,3x3) block 1 (SEDX_TUNE_WINO_F43 2): conv1 by its own
  // launch in both (2: in the chunk-of-4 layout), then the F(4x4,3x3) conv2
  if (x3) p->block1 = B1_PAD_X3;
  else if (f16) p->block1 = B1_PAD_F16;
  else if (!wino || t.wino_block1 == 0) p->block1 = B1_PAD_EXACT;
  else if (t.wino_f43 == 2) p->block1 = t.wino_block1 == 2 ? B1_CONV1C4_F43 : B1_CONV1_F43;
  else p->block1 = t.wino_block1 == 2 ? B1_F23_FUSED : B1_CONV1_F23;
  p->family = x3 ? CONV_X3 : f16 ? CONV_F16 : !wino ? CONV_EXACT : t.wino_f43 ? CONV_WINO43 : CONV_WINO;
  p->c4 = wino && t.wino_f43 && t.wino_block1 == 2;
  // block 1's chunk-of-4 pair stays reachable for A/B: SEDX_TUNE_WINO_ORDER 3 (every launch's order as 1)
  p->b1_planar = p->block1 == B1_CONV1C4_F43 && t.wino_order != 3;
  const int wino_order = t.wino_order == 3 ? 1 : t.wino_order;
  p->claims = x3 || f16 || (p->family == CONV_WINO43 && B >= 8);
  // the VGGish trunk: launch_vgg_conv1, then launch_conv3x3 on every layer, in every precision mode
  if (m.vgg) p->block1 = B1_VGG, p->family = CONV_EXACT, p->c4 = false, p->b1_planar = false, p->claims = false;
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
  // SEDX_TUNE_CF_ATTN 2: cf_relattn_kernel on ids 7, 8 and 19 (they keep their output bits), the matrix-pipe
  // kernel on Cnn_9layers_Conformer: at 32 x 1001 tokens its three launches take 1.56-1.57 ms against 7.58-7.97 ms
  // ("Token model")
  p->attn_mx = m.seq == SEQ_CONFORMER && (t.cf_attn == 1 || (t.cf_attn == 2 && m.token));
  // ---- where ----
  size_t end = 0;
  p->x0 = take(end, (size_t)B * T * 64);
  const size_t a0 = end;   // A starts here; its three phases (conv stack, head, Conformer) each carve from it
  // conv stack: block 1's first launch into A, then the layers ping-pong P / A
  size_t a_conv = p->block1 == B1_VGG                                   ? (size_t)B * g.T1 * 32 * 64
                  : p->block1 == B1_F23_FUSED                           ? 0
                  : p->block1 == B1_PAD_EXACT || p->block1 == B1_PAD_X3 || p->block1 == B1_PAD_F16
                      ? block1_pad_floats((int)B, (int)T)
                      : (size_t)B * T * 64 * 64;
  size_t p_conv = 0;
  const int64_t Ts[4] = {g.T, g.T1, g.T2, g.T3};
  // 14-layer trunk: block 4's conv2 pools 2x2; block 5 at F = 4, block 6 at F = 2 (its conv2: the mean of 2 bins)
  for (int i = 6; i < p->nlayers; ++i) {
    const int blk = (i + 1) / 2, cout = 64 << blk, F = 64 >> blk, last = i == 10, pool = i % 2 == 0 && !last;
    const int Tl = (int)(blk == 3 ? g.T3 : blk == 4 ? g.T4 : g.T5);
    p->layers[i] = ConvLayer{Tl, F, i % 2 ? cout / 2 : cout, cout, last ? EPI_FMEAN : pool ? EPI_POOL2 : EPI_STORE,
                             pool ? Tl / 2 : Tl, last ? 1 : pool ? F / 2 : F, 0, 0, 0};
    size_t& ext = i % 2 ? a_conv : p_conv;
    ext = std::max(ext, (size_t)B * p->layers[i].To * p->layers[i].Fo * cout);
  }
  // VGGish trunk: conv2 .. conv4_2 at (T1, 32), (T2, 16) x 2, (T3, 8) x 2; max pools after conv2, conv3_2 and
  // conv4_2, the last with the mean of its 4 pooled bins.  A layer's T is the pooled row count of the one
  // before it, so a row that a flooring pool dropped is nowhere: the next layer's bottom halo is zeros
  for (int i = 0; m.vgg && i < p->nlayers; ++i) {
    const int l = i + 1, cout = VGG_COUT[l], blk = (i + 1) / 2, F = 32 >> blk, last = i == 4, pool = i % 2 == 0;
    const int Tl = (int)(blk == 0 ? g.T1 : blk == 1 ? g.T2 : g.T3);
    p->layers[i] = ConvLayer{Tl, F, VGG_CIN[l], cout, last ? EPI_MAXPOOL2_FMEAN : pool ? EPI_MAXPOOL2 : EPI_STORE,
                             pool ? Tl / 2 : Tl, last ? 1 : pool ? F / 2 : F, 0, 0, 0};
    size_t& ext = i % 2 ? a_conv : p_conv;
    ext = std::max(ext, (size_t)B * p->layers[i].To * p->layers[i].Fo * cout);
  }
  for (int i = 0; !m.vgg && i < (deep ? 6 : 7); ++i) {
    const int blk = (i + 1) / 2, cout = 64 << blk, Tl = (int)Ts[blk], F = 64 >> blk, pool = i % 2 == 0 && i < 6;
    const bool fmean = i == 6 && !m.token;   // Cnn_9layers_Conformer keeps block 4's 8 bins (tokens.hip reads them)
    p->layers[i] = ConvLayer{Tl, F, i == 0 ? 64 : i % 2 ? cout / 2 : cout, cout,
                             fmean ? EPI_FMEAN : pool ? EPI_POOL2 : EPI_STORE,
                             pool ? Tl / 2 : Tl, fmean ? 1 : pool ? F / 2 : F, 0, 0,
                             i == 0 && p->block1 == B1_CONV1_F23 ? 0 : wino_order};
    size_t& ext = i % 2 ? a_conv : p_conv;
    ext = std::max(ext, (size_t)B * p->layers[i].To * p->layers[i].Fo * cout);
  }
  const size_t M = (size_t)p->M;
  size_t e_head = a0;
  // (Cnn14_DecisionLevelAtt: H [M][2048] and the logits only)
  // (Cnn_14layers_Conformer_FrameAtt: none of G / H / O; the encoder's regions below)
  // (Cnn_9layers_Conformer: as the line above, at M = B (8 T3 + 1) rows)
  const bool cf14 = (deep || m.token) && m.seq == SEQ_CONFORMER;
  p->G = take(e_head, m.decision || cf14 ? 0 : M * (deep && m.seq == SEQ_GRU ? 6144 : 1536));
  p->Hs = take(e_head, cf14 ? 0 : M * (deep ? 2048 : 512));
  p->O = take(e_head, m.decision || cf14 ? 0 : M * 512);
  p->LG = take(e_head, M * m.nac);
  p->gru = take(e_head, deep ? 0 : gru_coop_workspace_bytes((int)B) / 4);   // gru1024.hip: no scratch
  size_t e_a = std::max(a0 + align256(a_conv * 4), e_head);
  if (m.seq == SEQ_CONFORMER) {
    // from A's start: the conv stack is done and its last layer (the 9-layer trunk's block 4, the deep stack's
    // block 6) wrote the sequence input into P, so on the 14-layer trunk these follow the deep stack's regions
    // in time and share none of P
    size_t e_cf = a0;
    // Cnn_9layers_Conformer: the encoder's input [M][512], written by tokens.hip from block 4's pixels in P
    p->Tok = take(e_cf, m.token ? M * m.sw : 0);
    p->X = take(e_cf, M * CF_D);
    p->Xn = take(e_cf, M * CF_D);
    p->Hb = take(e_cf, M * CF_FF);
    p->AV = take(e_cf, M * CF_D);
    p->Rr = take(e_cf, (size_t)CF_BLOCKS * g.Ts * CF_D);
    p->RK = take(e_cf, (size_t)CF_BLOCKS * g.Ts * CF_D);
    p->LG = take(e_cf, M * m.nac);
    e_a = std::max(e_a, e_cf);
  }
  p->A = Region{a0 / 4, (e_a - a0) / 4};
  end = e_a;
  p->P = take(end, p_conv);
  p->sched = take(end, 7 * CONV_SCHED_INTS);
  p->total_bytes = end;
  for (int i = 0; i < p->nlayers; ++i) {
    p->layers[i].in = i % 2 ? p->P.off : p->A.off;
    p->layers[i].out = i % 2 ? p->A.off : p->P.off;
  }
  if (p->block1 == B1_F23_FUSED) p->layers[0].in = p->x0.off;
  // ---- the sequence layer's and the head's GEMMs, in launch order ----
  // fp32 (launch_linear) on the 14-layer trunk in every mode, split-bf16 elsewhere in x3 mode; the Conformer
  // encoder and its head by launch_cf_gemm in every mode
  p->ngemms = 0;
  auto gemm = [&](int stage, int Mr, int K, int N, int act, int by) {
    p->gemms[p->ngemms++] = GemmRow{stage, Mr, K, N, act, by, GemmLaunch{}};
  };
  const int by = x3 && !deep ? GEMM_BY_X3 : GEMM_BY_LINEAR, Mi = p->M;
  if (m.seq == SEQ_CONFORMER) {
    for (int b = 0; b < CF_BLOCKS; ++b) gemm(9, (int)g.Ts, CF_D, CF_D, 0, GEMM_BY_CF);   // r_net of every block
    gemm(9, Mi, m.sw, CF_D, 0, GEMM_BY_CF);                                              // input layer
    for (int b = 0; b < CF_BLOCKS; ++b) {
      gemm(9, Mi, CF_D, CF_FF, 0, GEMM_BY_CF), gemm(9, Mi, CF_FF, CF_D, 0, GEMM_BY_CF);      // ffn1
      gemm(9, Mi, CF_D, 3 * CF_D, 0, GEMM_BY_CF), gemm(9, Mi, CF_D, CF_D, 0, GEMM_BY_CF);    // mhsa: qkv_net, o_net
      gemm(9, Mi, CF_D, 2 * CF_D, 0, GEMM_BY_CF), gemm(9, Mi, CF_D, CF_D, 0, GEMM_BY_CF);    // conv module: pointwise convs
      gemm(9, Mi, CF_D, CF_FF, 0, GEMM_BY_CF), gemm(9, Mi, CF_FF, CF_D, 0, GEMM_BY_CF);      // ffn2
    }
  } else if (m.seq == SEQ_GRU) {
    gemm(9, Mi, m.sw, 3 * m.sw, 0, by);                            // both directions' gates: 1536, or 6144
  } else if (m.seq == SEQ_MHA) {
    gemm(9, Mi, m.sw, 1536, 0, by), gemm(9, Mi, 512, m.sw, 1, by);   // q|k|v, then fc + ReLU
  }   // (launch_decision pools inside its own fc1 staging: not a GEMM launcher's launch)
  gemm(10, Mi, m.hw, m.nac, 0, m.seq == SEQ_CONFORMER ? GEMM_BY_CF : by);   // the head projection
  // ---- shapes no forward runs ----
  p->reject[0] = 0;
  if (!shape_refusal(m, T, p->reject, sizeof(p->reject)) && B * g.T > INT32_MAX / 64)
    snprintf(p->reject, sizeof(p->reject), "batch too large");   // 32-bit launch sizes
  return p->reject[0] ? p->reject : nullptr;
}

// ---- one Winograd conv launch -----------------------------------------------
// items per persistent workgroup (compile-time inputs of A/B builds)
#ifndef SEDX_WINO_ITEMS
#define SEDX_WINO_ITEMS 4
#endif
// block 1's one-launch kernel: ~8 items per workgroup (isolated 0.731-0.733
// ms against 0.735-0.744 at 4 and 0.748-0.752 at 2; the two-stream headline
// the same within noise over four alternating rounds, tools/gpu_ab_iso.sh)
#ifndef SEDX_WINO_ITEMS_B1
#define SEDX_WINO_ITEMS_B1 8
#endif
// F(4x4,3x3).  Alone on the chip 16 (one persistent workgroup per
// CU: one exposed prologue per CU) is fastest — blocks 1-4 2.41 -> 2.35 ms
// (profiles/r05n_w43_items.log; 3 and 6 are slower:
// their grids break the L2 round order) — but in the two-stream headline
// long-lived workgroups hold the CUs the other batch's frontend / GRU /
// head need: 11,362-11,424 clips/s at 16, 11,546-11,585 at 4,
// 11,708-11,724 at 2 (profiles/r05p_items_ab.log).  2 stays.
#ifndef SEDX_W43_ITEMS
#define SEDX_W43_ITEMS 2
#endif

namespace {
constexpr int64_t ceil8(int64_t n) { return (n + 7) / 8 * 8; }

// what the plan reads of an item's geometry (wino_geom.h)
struct Item {
  int TG, NT;
  int trw, nch, wg_per_cu;   // tile rows and output channels of an item, workgroups a CU holds
  int64_t slab, halo;        // bytes of an item's weight slab and halo per input channel
};
template <int F, int TG, int NT, bool C1 = false>
constexpr Item f23_item() {
  using G = WinoGeom<F, TG, NT, C1>;
  return Item{TG, NT, G::TRW, G::NCH, G::WG_PER_CU, 16 * G::NCH * 4, G::PL * 4};
}
template <int TG, int NT>
Item f23_item(int F) {
  return F == 64 ? f23_item<64, TG, NT>() : F == 32 ? f23_item<32, TG, NT>() : F == 16 ? f23_item<16, TG, NT>()
                                                                                      : f23_item<8, TG, NT>();
}
// nt1: 16-channel items (NT 1) of the same tiles; __launch_bounds__(.., 1): one workgroup per CU
template <int F, int TG>
constexpr Item f43_item(bool nt1) {
  using G = W43Geom<F, TG>;
  return Item{TG, nt1 ? 1 : G::NT, G::TRW, nt1 ? 16 : G::NCH, 1, 36 * G::NCH * 4, G::RT * G::CS * 4};
}
Item f43_item(int F, int TG, bool nt1) {
  if (TG == 1) return F == 16 ? f43_item<16, 1>(nt1) : f43_item<8, 1>(nt1);   // 16-tile items: F = 16 / 8 only
  return F == 64 ? f43_item<64, 2>(nt1) : F == 32 ? f43_item<32, 2>(nt1) : F == 16 ? f43_item<16, 2>(nt1)
                                                                                   : f43_item<8, 2>(nt1);
}

// Persistent workgroups, a multiple of 8 (XCD-aware item decode), each
// walking its items with the next item's first chunks landing during the
// current one's last: ~items_per_wg items per workgroup, but at least one
// resident round — the hardware dispatcher still balances the workgroups over
// the CUs (a CU shared with another stream's kernel finishes its workgroups later)
int64_t persistent_grid(int64_t nitems, int64_t resident, int items_per_wg) {
  const int64_t per = (nitems + items_per_wg - 1) / items_per_wg;
  return std::min(nitems, std::max(std::max<int64_t>(8, resident), ceil8(per)));
}

// Rounds of 32 / G tile blocks x G channel groups: the G (< ngroups, dividing
// it) whose round streams the fewest bytes through an XCD's L2 — G weight
// slabs + 32 / G halos — with whole rounds of tile blocks per XCD and no
// padding; 0: the default order, tile block major.  (F(2x2) b4c2: 4 slabs of
// 2 MB + 8 halos of 0.7 MB instead of 8 + 4.)
int l2_round_order(int ngroups, int64_t tblocks, int64_t slab, int64_t halo) {
  int order2d = 0;
  int64_t best = (int64_t)ngroups * slab + (32 / std::min(ngroups, 32)) * halo;
  for (int gr = 1; gr <= 8 && gr < ngroups; gr *= 2) {
    const int64_t bytes = gr * slab + (32 / gr) * halo;
    if (ngroups % gr == 0 && tblocks % (8 * (32 / gr)) == 0 && bytes < best) best = bytes, order2d = gr;
  }
  return order2d;
}
}  // namespace

ConvLaunch plan_conv_launch(WinoFamily family, int ncu, int64_t B, int T, int F, int Cin, int Cout, int epi, int order,
                            bool c4, int nt_force, bool sched) {
  ConvLaunch p;
  auto refuse = [&p](const char* why) { return p.reject = why, p; };
  const bool b1 = family == WINO_F23_BLOCK1, f43 = family == WINO_F43;
  if (b1) F = Cin = Cout = 64, epi = EPI_POOL2, order = 0;   // X0 in, conv1's 64 channels, the pooled conv2 out
  if (B <= 0 || T < (b1 ? 2 : 1)) return refuse("empty batch or clip");
  if (F != 64 && F != 32 && F != 16 && F != 8) return refuse("F is not 64, 32, 16 or 8");
  if (Cin % 8 != 0 || Cin < (f43 ? 16 : 32) || Cout % 64 != 0 || Cout > 512) return refuse("channel counts");
  // F(2x2): halo lanes outside the clip step through the zero block by the
  // chunk's channel offset, so it must hold Cin + 4 floats
  if (family == WINO_F23 && Cin + 4 > ZERO_BLOCK_FLOATS) return refuse("Cin past the zero block");
  // the instantiated epilogues: the freq mean at F = 8 only and no pool
  // there; F(4x4) at F = 64 is block 1's conv2 (pooled)
  if (!(epi == EPI_STORE ? !(f43 && F == 64) : epi == EPI_POOL2 ? F != 8 : epi == EPI_FMEAN && F == 8))
    return refuse("no kernel for this epilogue at this F");
  // offsets in the kernels are 32-bit — elements, F(4x4)'s buffer DMA bytes:
  // a batch whose input passes 2^31 runs as launches over whole clips (same
  // per-clip work, so the outputs do not depend on the split)
  p.in_clip = b1 ? (int64_t)T * 64 : (int64_t)T * F * Cin;
  p.out_clip = (int64_t)Cout * (epi == EPI_STORE ? (int64_t)T * F : epi == EPI_POOL2 ? (int64_t)(T / 2) * (F / 2) : T);
  p.clips_per_launch = (f43 ? INT32_MAX / 4 - 1 : INT32_MAX - 1) / p.in_clip;
  if (p.clips_per_launch < 1) return refuse("one clip passes the 32-bit offsets");
  p.clips = (int)std::min(B, p.clips_per_launch);
  // ---- the item ----
  // tile rows of a clip: POOL2 drops an odd last row, the others keep it
  const int rows = epi == EPI_POOL2 ? 2 * (T / 2) : T;
  const int trows = f43 ? (rows + 3) / 4 : (rows + 1) / 2;
  auto tblocks_of = [&](const Item& i) { return (int64_t)p.clips * ((trows + i.trw - 1) / i.trw); };
  Item it;
  if (f43) {
    // nt_force: 0 = choose; 4 = 64-channel items; 1 = 16-channel items of 32
    // tiles; 2 = 16-channel items of 16 tiles (F = 16 / 8, chunk-of-4).
    // 16-channel items (NT 1, bit-identical) when 64-channel ones would give
    // at most a quarter of the CUs one (measured, profiles/r05q_small_batch.log:
    // at 128 items — b3c2 at B = 4, b4 at B = 8 — NT 1's four times the items
    // at a quarter the work each were slower; at <= 64 faster)
    const int64_t tb2 = tblocks_of(f43_item(F, 2, false));
    const bool nt1 = nt_force ? nt_force != 4 : ceil8(tb2) * (Cout / 64) <= ncu / 4;
    // 16-channel items of one tile group (16 tiles, 6 waves) where those of
    // two would leave CUs idle (one clip: the 256- and 512-channel layers, 128
    // and 64 items of 32 tiles; bit-identical — the same chains per output)
    const bool tg1 = (F == 16 || F == 8) && c4 && nt1 && (nt_force ? nt_force == 2 : ceil8(Cout / 16) * tb2 < ncu);
    if (nt_force == 2 && !tg1) return refuse("16-tile items: F = 16 / 8 in the chunk-of-4 layout only");
    it = f43_item(F, tg1 ? 1 : 2, nt1);
  } else if (b1) {
    // 2 tile groups x 64 channels (64 tiles, 8 waves) at every batch size (with
    // 1 tile group the 4 waves would not cover the halo's conv1 pixel groups)
    it = f23_item<64, 2, 2, true>();
  } else {
    // 2 tile groups x 64 channels (8 waves) when that gives every CU a
    // workgroup, else 1 x 64, else 1 x 32: the same per-(tile, channel) work
    auto fills = [&](const Item& i) { return tblocks_of(i) * (Cout / i.nch) >= ncu; };
    it = fills(f23_item<2, 2>(F)) ? f23_item<2, 2>(F) : fills(f23_item<1, 2>(F)) ? f23_item<1, 2>(F) : f23_item<1, 1>(F);
#ifdef SEDX_WINO_TG4   // A/B builds: 4 (and before it 3) tile groups x 32 channels where they fill the CUs
    if (fills(f23_item<4, 1>(F))) it = f23_item<4, 1>(F);
#endif
#ifdef SEDX_WINO_TG3
    if (fills(f23_item<3, 1>(F))) it = f23_item<3, 1>(F);
#endif
  }
  p.TG = it.TG, p.NT = it.NT;
  // ---- items and grid ----
  p.tb_per_clip = (trows + it.trw - 1) / it.trw;
  p.ngroups = Cout / it.nch;
  const int64_t tblocks = tblocks_of(it);
  // F(4x4) NT 1: 8 XCD lanes x ceil(groups / 8) channel tiles x every tile block
  const int64_t nitems = f43 && it.NT == 1 ? ceil8(p.ngroups) * tblocks : ceil8(tblocks) * p.ngroups;
  if (nitems > INT32_MAX || tblocks <= 0) return refuse("no tile row, or items past 2^31");
  // F(4x4)'s U: the NT 4 pack, then the NT 1 pack, behind one 32-bit buffer range
  if (f43 && 2 * (int64_t)Cin * Cout * 36 * 4 >= INT32_MAX) return refuse("U passes the 32-bit buffer range");
  const int64_t resident = (int64_t)ncu * it.wg_per_cu / 8 * 8;
  const int64_t grid = persistent_grid(nitems, resident, f43 ? SEDX_W43_ITEMS : b1 ? SEDX_WINO_ITEMS_B1 : SEDX_WINO_ITEMS);
  // F(4x4) item claims where there are more than two items per CU: one
  // persistent workgroup per CU (nwg a multiple of 8: every XCD lane has
  // workgroups).  Below that the first claim's latency is not amortised (B = 4
  // block 1: 0.0645 vs 0.0627 ms static, profiles/r06zb_*) and the static order
  // runs.  (plan_forward passes no counters below 8 clips: ForwardPlan::claims.)
  p.claim = f43 && SEDX_W43_CLAIM && sched && nitems > 2 * resident && resident >= 8;
  const int64_t nwg = p.claim ? resident : grid;
  p.nitems = (int)nitems, p.nwg = (int)nwg;
  // ---- the item order: whole 32-item rounds per XCD, a workgroup keeps its
  // slot in the round from item to item ----
  const bool rounds = order && nwg % 256 == 0 && (nitems / 8) % 32 == 0;
  if (f43 && F == 64) p.order2d = order == 2 && it.NT != 1 ? -1 : 0;   // block 1's contiguous per-XCD order
  else if (rounds && !b1 && !(f43 && it.NT == 1))
    p.order2d = l2_round_order(p.ngroups, tblocks, it.slab * Cin, it.halo * Cin);
  return p;
}

bool conv_launch_family(const ForwardPlan& p, int i, WinoFamily* family) {
  if (p.block1 == B1_VGG) return false;   // launch_conv3x3 on every layer
  const bool b1 = i == 0 && p.block1 != B1_PAD_EXACT && p.block1 != B1_PAD_X3 && p.block1 != B1_PAD_F16;   // a Winograd stage 2
  if (b1) *family = p.block1 == B1_F23_FUSED ? WINO_F23_BLOCK1 : p.block1 == B1_CONV1_F23 ? WINO_F23 : WINO_F43;
  else *family = p.family == CONV_WINO ? WINO_F23 : WINO_F43;
  return b1 || (i > 0 && (p.family == CONV_WINO || p.family == CONV_WINO43));
}

// ---- one fp32 GEMM launch -----------------------------------------------------
GemmLaunch plan_linear_launch(int M, int K, int N, int act, int ncu) {
  const int tx = (M + 127) / 128, ty = N / 64;   // the tiled kernel's grid
  const int sx = (M + 31) / 32, sy = N / 32;     // 32 x 32 tiles
  if (N <= 64 && act == 0 && K % 256 == 0 && N % 32 == 0)   // the head projection, every M
    return GemmLaunch{GEMM_KSPLIT, sx, sy, 256};
  // one wave per 32 x 32 tile while the tiled grid would leave CUs without a workgroup
  if ((int64_t)tx * ty < ncu && K % 64 == 0 && N % 32 == 0) return GemmLaunch{GEMM_ONE_WAVE, sx, sy, 64};
  return GemmLaunch{GEMM_TILED, tx, ty, 256};
}

std::vector<GemmRow> plan_gemm_launches(const ForwardPlan& p, int ncu) {
  std::vector<GemmRow> rows(p.gemms, p.gemms + p.ngemms);
  for (GemmRow& r : rows)   // launch_linear_x3 and launch_cf_gemm keep their own shape choice
    r.l = r.launcher == GEMM_BY_LINEAR ? plan_linear_launch(r.M, r.K, r.N, r.act, ncu)
                                       : GemmLaunch{r.launcher == GEMM_BY_X3 ? GEMM_X3 : GEMM_CONFORMER, 0, 0, 0};
  return rows;
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
  const bool gamma = m.cfg.feature_type == SEDX_FEATURE_GAMMA;
  for (int w = 0; w < wg->n_win; ++w) {
    const int64_t len = wg->loop.len[w];
    // a gamma model's window goes through fft_gtgram like a clip (utils/features.py:356-370): un-centred frames,
    // so it needs one whole FFT of samples
    if (gamma && audio_T(m, len) < 1) {
      snprintf(wg->reject, sizeof(wg->reject), "window %d has %lld samples: shorter than the gammatone FFT", w,
               (long long)len);
      return wg->reject;
    }
    // the model raises on these windows: STFT reflect padding needs more
    // than n_fft/2 samples (stft.py:237); then what every forward refuses
    if (!gamma && len <= m.cfg.window_size / 2) {
      snprintf(wg->reject, sizeof(wg->reject), "window %d has %lld samples: too short for the STFT's reflect padding",
               w, (long long)len);
      return wg->reject;
    }
    if (wg->groups.empty() || wg->groups.back().len != len) {
      WinGroup g;
      g.w0 = w;
      g.len = len;
      g.g = geometry_from_T(m, audio_T(m, len));   // the frontend's own frame count (gamma: 1 + (len - nfft) / hop)
      char why[96];
      if (shape_refusal(m, g.g.T, why, sizeof(why))) {
        snprintf(wg->reject, sizeof(wg->reject), "window %d: %s", w, why);
        return wg->reject;
      }
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
  // a gamma model: the frontend's mag / db / mm, shared by the groups' forwards (one runs at a time)
  for (const auto& g : wg.groups) l.fe_bytes = std::max(l.fe_bytes, frontend_bytes(m, n_clips * g.nw, g.len));
  l.fe = carve(end, l.fe_bytes);
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

// ---- ragged windowed driver -----------------------------------------------------
const char* ragged_geometry(const Model& m, const int64_t* clip_len, int64_t n_clips, const sedx_window_spec* spec,
                            const double* dur, RaggedGeom* rg) {
  if (!spec) return "null window spec";
  if (!clip_len || n_clips <= 0) return "null clip lengths or no clips";
  if (spec->driver != SEDX_DRIVER_PREDICT)
    return "the ragged driver is predict.py's: main_strong pads every clip to 10 s and has no ragged form";
  if (spec->vote != 0) return "the ragged driver has no vote merge (sedx_window_spec.vote must be 0)";
  if (spec->audio_duration > 0) return "sedx_window_spec.audio_duration must be <= 0: the durations come per clip";
  if (n_clips >= INT32_MAX) return "too many clips";
  *rg = RaggedGeom{};
  rg->clip_len.assign(clip_len, clip_len + n_clips);
  rg->n_win.resize((size_t)n_clips);
  rg->plan_of.resize((size_t)n_clips);
  rg->item_off.assign((size_t)n_clips + 1, 0);
  rg->frame_off.assign((size_t)n_clips + 1, 0);
  std::vector<int32_t> plan_nw;   // the window count plans[i] was built for
  WindowLoop wl;
  WinGeom wg;
  for (int64_t c = 0; c < n_clips; ++c) {
    sedx_window_spec sp = *spec;
    sp.audio_duration = dur && dur[c] > 0 ? dur[c] : 0.0;
    const char* why = window_loop(m.cfg.sample_rate, clip_len[c], sp, &wl);
    const int32_t nw = (int32_t)wl.start.size();
    // the ragged driver's own rule: a clip holds at least one complete window.  (Alone, such a clip runs as one
    // zero-padded window, as in the reference; a directory's stray short file is refused by index instead, and
    // predict_files lists it as skipped.)
    if (!why && clip_len[c] < (int64_t)sp.sample_duration * m.cfg.sample_rate)
      why = "no complete window: the clip is shorter than sample_duration";
    size_t pi = plan_nw.size();
    if (!why) {
      // window_geometry's remaining rules (the window's samples, the model's frame limits, the merge) see a
      // clip only through its window count: one run, and one merge plan, per distinct count
      pi = (size_t)(std::find(plan_nw.begin(), plan_nw.end(), nw) - plan_nw.begin());
      if (pi == plan_nw.size()) {
        why = window_geometry(m, clip_len[c], &sp, true, &wg);
        if (!why) {
          if (wg.groups.size() != 1) why = "windows of more than one length";   // (not the predict driver's)
          else {
            rg->full_len = wg.full_len;
            rg->g = wg.groups[0].g;
            plan_nw.push_back(nw);
            rg->plans.push_back(std::move(wg.plan));
          }
        }
      }
    }
    if (why) {
      char buf[160];
      snprintf(buf, sizeof(buf), "%s", why);   // (why may point into wg.reject)
      snprintf(rg->reject, sizeof(rg->reject), "clip %lld: %s", (long long)c, buf);
      return rg->reject;
    }
    rg->n_win[c] = nw;
    rg->plan_of[c] = (int32_t)pi;
    rg->item_off[c + 1] = rg->item_off[c] + nw;
    rg->frame_off[c + 1] = rg->frame_off[c] + rg->plans[pi].N;
    rg->win_start.insert(rg->win_start.end(), wl.start.begin(), wl.start.end());
    // the tables index items and merged rows with 32 bits
    if (rg->item_off[c + 1] > INT32_MAX / 2 || rg->frame_off[c + 1] > INT32_MAX / std::max(1, m.cfg.classes_num))
      return "too many windows or merged frames for one ragged call";
  }
  return nullptr;
}

RaggedLayout ragged_layout(const Model& m, const Tuning& t, const RaggedGeom& rg, int64_t items_per_forward) {
  RaggedLayout l;
  const size_t C = m.cfg.classes_num;
  l.items = rg.item_off.back();
  l.chunk = items_per_forward > 0 ? std::min(items_per_forward, l.items) : l.items;
  // the forwards: full chunks, then the rest (a smaller batch may plan other kernels)
  ForwardPlan fp;
  plan_forward(m, t, l.chunk, rg.g.T, &fp);
  l.model_bytes = fp.total_bytes;
  if (l.chunk > 0 && l.items % l.chunk) {
    plan_forward(m, t, l.items % l.chunk, rg.g.T, &fp);
    l.model_bytes = std::max(l.model_bytes, fp.total_bytes);
  }
  size_t end = l.model_bytes;
  l.fw = take(end, (size_t)l.items * rg.g.out_frames * C).off;
  l.clipwise = take(end, (size_t)l.chunk * C).off;
  l.fe_bytes = frontend_bytes(m, l.chunk, rg.full_len);   // a gamma model: mag / db / mm of one forward's items
  l.fe = carve(end, l.fe_bytes);
  l.tables = end / 4;
  for (const MergePlan& p : rg.plans) {
    l.n_off += (size_t)p.N + 1;
    l.n_src += p.src.size();
  }
  size_t b = 0;
  l.t_item = carve(b, sizeof(ItemRow) * (size_t)l.items);
  l.t_clip = carve(b, sizeof(RaggedClipRow) * (rg.n_win.size() + 1));
  l.t_off = carve(b, 4 * l.n_off);
  l.t_src = carve(b, 8 * l.n_src);
  l.t_div = carve(b, 4 * l.n_off);
  l.table_bytes = b;
  l.total_bytes = end + b;
  return l;
}

void ragged_tables(const RaggedGeom& rg, const RaggedLayout& l, const int64_t* clip_off, std::vector<char>* blob) {
  blob->assign(l.table_bytes, 0);
  ItemRow* item = reinterpret_cast<ItemRow*>(blob->data() + l.t_item);
  RaggedClipRow* crow = reinterpret_cast<RaggedClipRow*>(blob->data() + l.t_clip);
  int32_t* off = reinterpret_cast<int32_t*>(blob->data() + l.t_off);
  int32_t* src = reinterpret_cast<int32_t*>(blob->data() + l.t_src);   // (window, frame) pairs
  int32_t* div = reinterpret_cast<int32_t*>(blob->data() + l.t_div);
  // the plans' tables back to back; off stays relative to its own plan's src entries
  std::vector<int32_t> off0(rg.plans.size()), src0(rg.plans.size());
  size_t no = 0, ns = 0;
  for (size_t pi = 0; pi < rg.plans.size(); ++pi) {
    const MergePlan& p = rg.plans[pi];
    off0[pi] = (int32_t)no;
    src0[pi] = (int32_t)ns;
    std::copy(p.off.begin(), p.off.end(), off + no);
    std::copy(p.div.begin(), p.div.end(), div + no);   // N entries of the N + 1 (the last stays 0)
    for (size_t j = 0; j < p.src.size(); ++j) {
      const int32_t id = p.src[j];
      const int w = (int)(std::upper_bound(p.win_base.begin(), p.win_base.end(), id) - p.win_base.begin()) - 1;
      src[2 * (ns + j)] = w;
      src[2 * (ns + j) + 1] = id - p.win_base[w];
    }
    no += (size_t)p.N + 1;
    ns += p.src.size();
  }
  const size_t n_clips = rg.n_win.size();
  for (size_t c = 0; c < n_clips; ++c) {
    crow[c] = RaggedClipRow{(int32_t)rg.frame_off[c], (int32_t)rg.item_off[c], off0[rg.plan_of[c]], src0[rg.plan_of[c]]};
    for (int32_t w = 0; w < rg.n_win[c]; ++w) {
      const int64_t st = rg.win_start[(size_t)rg.item_off[c] + w];
      // samples of the window backed by the clip's audio, in [0, full_len]: beyond them pad_truncate's zeros
      const int64_t av = std::min(rg.full_len, std::max<int64_t>(0, rg.clip_len[c] - st));
      // a window wholly past its clip reads nothing: its source stays inside the buffer
      item[rg.item_off[c] + w] = ItemRow{clip_off[c] + (av > 0 ? st : 0), av};
    }
  }
  crow[n_clips] = RaggedClipRow{(int32_t)rg.frame_off[n_clips], (int32_t)rg.item_off[n_clips], 0, 0};
}

}  // namespace sedx
