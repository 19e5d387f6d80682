// libsedx C ABI (include/sedx.h): handle, state_dict ingestion + packing,
// forward orchestration, windowed driver.  Host C++; kernels live in *.hip.
#include <new>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/sedx.h"
#include "rank.h"
#include "sedx_internal.h"

using namespace sedx;

// one forward's stage-boundary events: events 0..10 bound stages 0..10 (stage
// i = [i, i + 1]) except stage 0 = [0, 12] (frontend) and stage 11 = [12, 1]
// (pipeline wait): event 12 is recorded after the frontend, before the
// cross-stream wait
struct EvSet {
  hipEvent_t ev[SEDX_N_STAGES + 1] = {};
  bool rec[SEDX_N_STAGES + 1] = {};
};

// the model (cfg, seq, head, hw, nac: sedx_create, weights.h) and its state
struct sedx_handle : sedx::Model {
  int device = 0;
  std::string err;
  std::map<std::string, Tensor> params;
  std::map<std::string, std::vector<int64_t>> expected;
  bool finalized = false;
  void* blob = nullptr;      // single device allocation for all packed weights
  DevWeights w;
  F16Weights wf16;           // SEDX_PRECISION_F16's conv packs, in the same allocation
  int g_nfft = 0, g_hop = 0;   // gammatone FFT size and hop (prepare_weights)
  void* ws = nullptr;        // cached workspace
  size_t ws_bytes = 0;
  Tuning tune;               // sedx_set_precision / sedx_set_tuning / sedx_set_pipelined (plan.h)
  // sedx_set_capture: copy one stage's output of every later forward
  int cap_stage = -1;
  float* cap_buf = nullptr;
  size_t cap_bytes = 0;
  bool conv_done_recorded = false;   // sedx_set_pipelined
  hipEvent_t conv_done = nullptr;
  // host-mapped word the GRU kernel ORs a failure code into when a bounded
  // hand-off spin times out (that forward's outputs are NaN); the next
  // forward / sedx_stage_times turns it into SEDX_EHIP
  unsigned* gru_err_host = nullptr;
  unsigned* gru_err_dev = nullptr;
  // the last ragged window plan and what it was asked for (ragged_geometry_of)
  struct RaggedMemo {
    bool valid = false, has_dur = false;
    std::vector<int64_t> len;
    std::vector<double> dur;
    sedx_window_spec spec{};
    RaggedGeom rg;
  } ragged_memo;
  // optional per-stage timing (sedx_set_profiling): mark() records into
  // ev_cur, which is ev_last in mode 1.  Mode 2 (accumulate): every forward
  // takes its own set from the pool, so forwards in flight on different
  // streams time independently; sedx_stage_times folds the used sets into
  // per-stage sums and averages
  int profiling = 0;          // 0 off, 1 last forward, 2 accumulate
  EvSet ev_last;
  std::vector<EvSet> ev_pool;
  size_t ev_used = 0;
  EvSet* ev_cur = nullptr;
  double acc_ms[SEDX_N_STAGES] = {};
  int64_t acc_n[SEDX_N_STAGES] = {};
};

namespace {
// the events bounding stage i (see EvSet)
inline int stage_begin(int i) { return i == 11 ? 12 : i; }
inline int stage_end(int i) { return i == 0 ? 12 : i == 11 ? 1 : i + 1; }
static_assert(SEDX_N_STAGES == 12, "stage event map");

// elapsed ms of stage i in set e, once its end event completed; *recorded =
// false (and *ms untouched) when the set does not hold both events
hipError_t stage_ms(const EvSet& e, int i, float* ms, bool* recorded) {
  const int a = stage_begin(i), b = stage_end(i);
  *recorded = e.rec[a] && e.rec[b];
  if (!*recorded) return hipSuccess;
  const hipError_t st = hipEventSynchronize(e.ev[b]);
  return st != hipSuccess ? st : hipEventElapsedTime(ms, e.ev[a], e.ev[b]);
}

// mode 2: sums the elapsed times of every used event set, frees the pool
void fold_ev_pool(sedx_handle* h) {
  for (size_t k = 0; k < h->ev_used; ++k)
    for (int i = 0; i < SEDX_N_STAGES; ++i) {
      float v = 0.f;
      bool rec = false;
      if (stage_ms(h->ev_pool[k], i, &v, &rec) == hipSuccess && rec) {
        h->acc_ms[i] += v;
        ++h->acc_n[i];
      }
    }
  h->ev_used = 0;
  h->ev_cur = nullptr;
}

inline void mark(sedx_handle* h, int i, hipStream_t s) {
  if (!h->profiling) return;
  if (h->profiling == 2 && i == 0) {    // a forward starts: next event set
    if (h->ev_used == 4096) fold_ev_pool(h);
    if (h->ev_used == h->ev_pool.size()) {
      h->ev_pool.emplace_back();
      for (auto& e : h->ev_pool.back().ev)
        if (hipEventCreate(&e) != hipSuccess) e = nullptr;
    }
    h->ev_cur = &h->ev_pool[h->ev_used++];
    for (auto& r : h->ev_cur->rec) r = false;
  }
  EvSet* e = h->ev_cur;
  if (e && e->ev[i]) {
    (void)hipEventRecord(e->ev[i], s);
    e->rec[i] = true;
  }
}

sedx_status fail(const sedx_handle* h, sedx_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) const_cast<sedx_handle*>(h)->err = buf;   // the const queries set sedx_last_error's message too
  return st;
}

#define HIP_TRY(h, expr)                                                                \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(h, SEDX_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));         \
  } while (0)

// sedx_set_capture: stage `stage` just wrote `n` floats at `src`
void capture(sedx_handle* h, int stage, const float* src, size_t n, hipStream_t s) {
  if (h->cap_stage != stage || !h->cap_buf) return;
  const size_t bytes = std::min(n * sizeof(float), h->cap_bytes);
  if (hipMemcpyAsync(h->cap_buf, src, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
    note_launch_error(hipErrorInvalidValue);
}
// a stage held in the chunk-of-4 layout [B][C/4][T][F][4] (the F(4x4,3x3)
// layers): captured in the documented channels-last layout (a buffer short
// of the whole stage gets the raw prefix)
void capture_c4(sedx_handle* h, int stage, const float* src, int64_t B, int T, int F, int C, hipStream_t s) {
  if (h->cap_stage != stage || !h->cap_buf) return;
  const size_t n = (size_t)B * T * F * C;
  if (h->cap_bytes < n * sizeof(float)) return capture(h, stage, src, n, s);
  launch_c4_to_nhwc(src, (int)B, T, F, C, h->cap_buf, s);
}

// errors of the launches just issued: preparation failures noted by
// launch_info (sedx_internal.h) first, then the runtime's launch error
sedx_status launch_status(sedx_handle* h) {
  const hipError_t pe = take_launch_error();
  if (pe != hipSuccess) return fail(h, SEDX_EHIP, "kernel launch preparation failed: %s", hipGetErrorString(pe));
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(h, SEDX_EHIP, "kernel launch failed: %s", hipGetErrorString(le));
  return SEDX_OK;
}

// a GRU hand-off of an earlier forward timed out (its outputs were NaN)
sedx_status check_async_error(sedx_handle* h) {
  if (!h->gru_err_host) return SEDX_OK;
  const unsigned code = __atomic_exchange_n(h->gru_err_host, 0u, __ATOMIC_ACQ_REL);
  if (code)
    return fail(h, SEDX_EHIP, "a GRU recurrence hand-off of an earlier forward timed out (code %u): its "
                              "outputs were NaN", code);
  return SEDX_OK;
}

// what every forward checks before it looks at its arguments
sedx_status preflight(sedx_handle* h) {
  if (!h) return SEDX_EINVAL;
  if (!h->finalized) return fail(h, SEDX_ESTATE, "weights not finalised");
  return check_async_error(h);
}

// the geometry the size queries answer for: L_or_T = samples (logmel) or frames (gamma)
sedx_status query_geometry(const sedx_handle* h, int64_t L_or_T, Geometry* g) {
  *g = geometry_from_T(*h, h->cfg.feature_type == SEDX_FEATURE_GAMMA ? L_or_T : conv_T(*h, L_or_T));
  char buf[96];
  const char* why = shape_refusal(*h, g->T, buf, sizeof(buf));   // the queries reject what the forward rejects ...
  // ... but one: on the 9-layer trunk the size of an input too short for any forward is still reported (frames 0)
  // (Cnn_9layers_Conformer refuses it here as everywhere)
  if (why && !(h->depth == 9 && g->Ts < 1 && !h->token)) return fail(h, SEDX_EINVAL, "%s", why);
  return SEDX_OK;
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

sedx_status get_ws(sedx_handle* h, size_t need, void* user, size_t user_bytes, float** out) {
  if (user) {
    if (user_bytes < need)
      return fail(h, SEDX_EINVAL, "workspace too small: %zu < %zu bytes", user_bytes, need);
    *out = static_cast<float*>(user);
    return SEDX_OK;
  }
  if (h->ws_bytes < need) {
    if (h->ws) (void)hipFree(h->ws);
    h->ws = nullptr;
    h->ws_bytes = 0;
    HIP_TRY(h, hipMalloc(&h->ws, need));
    h->ws_bytes = need;
  }
  *out = static_cast<float*>(h->ws);
  return SEDX_OK;
}

// the log-mel frontend of plan p's items into its X0: n_win windows of
// sig_len samples per clip at win_start (device; nullptr: one, at 0); or, with
// item_tab (device, one row per item), every item's source from its row
void run_logmel(sedx_handle* h, const ForwardPlan& p, float* ws, const float* audio, const int16_t* audio_i16,
                int64_t clip_stride, int64_t n_clips, int n_win, const int64_t* win_start, int64_t clip_len,
                int64_t sig_len, hipStream_t s, const ItemRow* item_tab = nullptr) {
  const DevWeights& w = h->w;
  FrontendParams f{};
  f.item_tab = item_tab;
  f.audio = audio;
  f.audio_i16 = audio_i16;
  f.clip_stride = clip_stride;
  f.n_clips = (int32_t)n_clips;
  f.n_win = n_win;
  f.win_start = win_start;
  f.clip_len = clip_len;
  f.sig_len = sig_len;
  f.T = (int32_t)p.g.T;
  f.hop = h->cfg.hop_size;
  f.twiddle = reinterpret_cast<const float2*>(w.twiddle);
  f.window = w.window;
  f.mel_w = w.mel_w;
  f.mel_tab = w.mel_tab;
  f.mel_mt = h->tune.mel_mfma ? w.mel_mt : nullptr;   // the MFMA mel table (nullptr when the host did not build one)
  for (int j = 0; j < 4; ++j) {
    f.mt_klo[j] = w.mt_klo[j];
    f.mt_ns[j] = w.mt_ns[j];
    f.mt_off[j] = w.mt_off[j];
  }
  f.mt_floats = w.mt_floats;
  f.mel_wmax = w.mel_wmax;
  f.mel_off = w.mel_off;
  f.mel_lo = w.mel_lo;
  f.bn_scale = w.bn0_scale;
  f.bn_mean = w.bn0_mean;
  f.bn_bias = w.bn0_bias;
  f.out = ws + p.x0.off;
  launch_logmel(f, h->cfg.window_size, s);
}

// the gammatone frontend of plan p's items into its X0 (launch_gamma_items): items of sig_len samples, mapped
// onto the clips' audio as run_logmel's are; fe: the frontend's regions (gamma_layout for p.B items).
// even_bases: the host knows every item's first sample to be at an even offset
sedx_status run_gamma_items(sedx_handle* h, const ForwardPlan& p, float* ws, char* fe, const float* audio,
                            int64_t clip_stride, int n_win, const int64_t* win_start, int64_t clip_len,
                            int64_t sig_len, bool even_bases, hipStream_t s, const ItemRow* item_tab = nullptr) {
  if (p.B > 65535) return fail(h, SEDX_EINVAL, "forward too large: %lld items (the gammatone frontend runs at most 65535)",
                               (long long)p.B);
  const GammaLayout lay = gamma_layout(p.B, sig_len, h->g_nfft, h->g_hop);
  if (lay.T != p.g.T) return fail(h, SEDX_ESTATE, "the gammatone frontend's frames (%lld) are not the plan's (%lld)",
                                  (long long)lay.T, (long long)p.g.T);
  GammaItemParams g{};
  g.audio = audio;
  g.L = sig_len;
  g.B = (int32_t)p.B;
  g.T = (int32_t)lay.T;
  g.T_fill = (int32_t)lay.T_fill;
  g.hop = h->g_hop;
  g.nfft = h->g_nfft;
  g.kp = lay.kp;
  g.twiddle = reinterpret_cast<const double2*>(h->w.g_twiddle);
  g.window = h->w.g_window;
  g.weightsT = h->w.g_weightsT;
  g.mag = reinterpret_cast<double*>(fe + lay.mag_off);
  g.db = reinterpret_cast<double*>(fe + lay.db_off);
  g.mm = reinterpret_cast<unsigned long long*>(fe + lay.mm_off);
  g.out = nullptr;
  g.item_tab = item_tab;
  g.win_start = win_start;
  g.clip_stride = clip_stride;
  g.clip_len = clip_len;
  g.n_win = n_win;
  launch_gamma_items(g, even_bases, h->tune.gamma_spec, h->w.bn0_scale, h->w.bn0_mean, h->w.bn0_bias, ws + p.x0.off, s);
  return SEDX_OK;
}

// CNN + head on X0 [B][T][64] already in the workspace: every kernel choice
// and every pointer comes from the plan
sedx_status run_body(sedx_handle* h, const ForwardPlan& p, float* ws, float* d_fw, float* d_clip, float* d_emb,
                     hipStream_t s) {
  const DevWeights& w = h->w;
  const Tuning& t = h->tune;
  const Geometry& g = p.g;
  const int64_t B = p.B;
  const int iB = (int)B, M = p.M, T3 = (int)g.Ts;   // the sequence's frames (T5 on the 14-layer trunk)
  float* X0 = ws + p.x0.off;
  float* A = ws + p.A.off;
  int* sched = reinterpret_cast<int*>(ws + p.sched.off);
  // the cross-stream wait for the previous forward's conv stack comes before
  // the b1c1 stage event, so stage 1 times only this forward's work
  mark(h, 12, s);   // the frontend's end: the wait below is stage 11, not the frontend's
  // block 1's first launch (conv1 / the zero-bordered copy of X0): before
  // the pipelined wait with sedx_set_pipelined(h, 2) — an HBM-bound launch
  // that may then overlap the previous forward's compute-bound conv tail —
  // else after it (stage 1)
  auto block1_first = [&]() {
    switch (p.block1) {
      case B1_CONV1C4_F43:
        if (p.b1_planar) launch_conv1_planar(X0, iB, (int)g.T, w.c1_w, w.c1_b, A, s);
        else launch_conv1_c4(X0, iB, (int)g.T, w.c1_w, w.c1_b, A, s);
        break;
      case B1_CONV1_F23:
      case B1_CONV1_F43: launch_conv1_nhwc(X0, iB, (int)g.T, w.c1_w, w.c1_b, A, s); break;
      case B1_PAD_EXACT:
      case B1_PAD_X3:
      case B1_PAD_F16: launch_pad_x0(X0, iB, (int)g.T, A, s); break;
      case B1_F23_FUSED: break;   // conv1 inside the stage-2 launch
      case B1_VGG: launch_vgg_conv1(X0, iB, (int)g.T, w.c1_w, w.c1_b, A, s); break;   // conv1 + ReLU + max pool
    }
  };
  // the claim counters (the workspace comes from the caller): zeroed once per
  // forward, ahead of the pipelined wait — this forward's memory only
  if (p.claims) HIP_TRY(h, hipMemsetAsync(sched, 0, 7 * CONV_SCHED_INTS * sizeof(int), s));
  const bool first_early = t.pipelined && t.pipe_conv1_first;
  if (first_early) block1_first();
  if (t.pipelined && h->conv_done_recorded) HIP_TRY(h, hipStreamWaitEvent(s, h->conv_done, 0));
  mark(h, 1, s);
  capture(h, 0, X0, (size_t)B * g.T * 64, s);
  if (!first_early) block1_first();
  if (h->vgg) capture(h, 50, A, (size_t)B * g.T1 * 32 * 64, s);
  for (int i = 0; i < p.nlayers; ++i) {
    const ConvLayer& c = p.layers[i];
    const int k = i + 1;   // the layer's weights
    float* in = ws + c.in;
    float* out = ws + c.out;
    if (h->vgg) {
      // VGGish trunk: conv2 .. conv4_2 on the exact fp32 kernel in every mode (stages 2-6; captures 51-54, 8)
      mark(h, 2 + i, s);
      launch_conv3x3(in, iB, c.T, c.F, c.cin, c.cout, w.wp[k], w.cb[k], out, c.epi, w.zero, s);
      capture(h, i == 4 ? 8 : 51 + i, out, (size_t)B * c.To * c.Fo * c.cout, s);
      // capture 55, conv4_2's pooled output before the mean: the same layer once more with the pool alone,
      // straight into a buffer that holds all of it
      const size_t n55 = (size_t)B * c.To * (c.F / 2) * c.cout;
      if (i == 4 && h->cap_stage == 55 && h->cap_buf && h->cap_bytes >= n55 * sizeof(float))
        launch_conv3x3(in, iB, c.T, c.F, c.cin, c.cout, w.wp[k], w.cb[k], h->cap_buf, EPI_MAXPOOL2, w.zero, s);
      if (i == 4) mark(h, 7, s), mark(h, 8, s);   // no launches of their own: stage 6 ends here
      continue;
    }
    if (i >= p.first_deep) {
      // 14-layer trunk: block 4's pooled conv2 (stage 8, reading block 4 conv1's
      // layout) and blocks 5-6 (timed inside stage 8; captures 40..43), fp32 in every mode
      if (i < 7) mark(h, 2 + i, s);
      const int l = i - p.first_deep;   // the layer's slice of the deep pack (weights.h)
      launch_conv3x3_deep(in, iB, c.T, c.F, c.cin, c.cout, w.wp[7] + deep_w_off(l), w.cb[7] + deep_b_off(l), out,
                          c.epi, p.c4 && l == 0, s);
      capture(h, i < 7 ? 2 + i : 40 + (i - 7), out, (size_t)B * c.To * c.Fo * c.cout, s);
      continue;
    }
    int* claim = p.claims ? sched + i * CONV_SCHED_INTS : nullptr;
    mark(h, 2 + i, s);
    // block 1 as one launch: conv1 computed inside conv2's halo staging (the
    // b1c1 stage is just the zero-bordered copy of the bn0 output), or conv2
    // on conv1's activation
    WinoFamily wf;
    const bool wino = conv_launch_family(p, i, &wf);   // sedx_conv_launch_plan answers by the same call
    if (wino && wf == WINO_F23_BLOCK1)
      launch_block1_wino(in, iB, c.T, w.c1_w, w.c1_b, w.wu[k], w.cb[k], out, w.zero, w.trash, s, p.c4);
    else if (wino && wf == WINO_F23)
      launch_conv3x3_wino(in, iB, c.T, c.F, c.cin, c.cout, w.wu[k], w.cb[k], out, c.epi, w.zero, w.trash, s, c.order);
    else if (wino)   // in block 1 on conv1's activation (B1_CONV1_F43, B1_CONV1C4_F43)
      launch_conv3x3_wino43(in, iB, c.T, c.F, c.cin, c.cout, w.wu43[k], w.cb[k], out, c.epi, w.trash, s, c.order,
                            p.c4, 0, claim, i == 0 && p.b1_planar);
    else if (i == 0 && p.block1 == B1_PAD_X3)
      launch_block1_fused_x3(nullptr, iB, c.T, in, w.c1_wt, w.c1_b, w.wx3[k], w.cb[k], out, claim, s);
    else if (i == 0 && p.block1 == B1_PAD_F16)
      launch_block1_fused_f16(iB, c.T, in, w.c1_wt, w.c1_b, h->wf16.w[k], w.cb[k], out, claim, s);
    else if (i == 0)   // B1_PAD_EXACT
      launch_block1_exact(in, iB, c.T, w.c1_w, w.c1_b, w.wp[k], w.cb[k], out, w.zero, s);
    else if (p.family == CONV_X3)
      launch_conv3x3_x3(in, iB, c.T, c.F, c.cin, c.cout, w.wx3[k], w.cb[k], out, c.epi, claim, s);
    else if (p.family == CONV_F16)
      launch_conv3x3_f16(in, iB, c.T, c.F, c.cin, c.cout, h->wf16.w[k], w.cb[k], out, c.epi, claim, s);
    else
      launch_conv3x3(in, iB, c.T, c.F, c.cin, c.cout, w.wp[k], w.cb[k], out, c.epi, w.zero, s);
    if (h->token && i == 6) {
      // Cnn_9layers_Conformer: the tag token, then block 4's pixels in (frame, bin) order (inside stage 8; capture 8)
      launch_tokens(out, iB, c.To, p.c4, w.bfc, ws + p.Tok.off, s);   // bfc: the tag token (weights.h)
      capture(h, 8, ws + p.Tok.off, (size_t)M * h->sw, s);
    } else if (p.c4 && c.epi != EPI_FMEAN)
      capture_c4(h, 2 + i, out, B, c.To, c.Fo, c.cout, s);
    else
      capture(h, 2 + i, out, (size_t)B * c.To * c.Fo * c.cout, s);
  }
  mark(h, 9, s);
  if (t.pipelined) {
    HIP_TRY(h, hipEventRecord(h->conv_done, s));
    h->conv_done_recorded = true;
  }
  const bool x3 = t.precision == SEDX_PRECISION_X3;
  float* S = ws + (h->token ? p.Tok.off : p.P.off);   // [B][T3][512] (14-layer: [B][T5][2048]; tokens: [B][8 T3 + 1][512])
  float* G = ws + p.G.off;
  float* Hs = ws + p.Hs.off;
  float* O = ws + p.O.off;
  float* LG = ws + p.LG.off;
  // GEMMs: M, K, N and act of every launch from here to the head finish are the plan's next row (p.gemms, which
  // sedx_gemm_launch_plan reports); a launch the plan does not list is not issued, and is SEDX_ESTATE below
  int used = 0;
  bool drift = false;
  auto next_row = [&](bool cf) -> const GemmRow* {
    const GemmRow* r = used < p.ngemms && (p.gemms[used].launcher == GEMM_BY_CF) == cf ? &p.gemms[used] : nullptr;
    ++used, drift |= !r;
    return r;
  };
  // x3 split-bf16 MFMA or fp32 MFMA, by the row (bn: the x3 kernel's tile width)
  auto linear = [&](const float* a, const float* wf, void* wx, int bn, const float* bias, float* c) {
    const GemmRow* r = next_row(false);
    if (r && r->launcher == GEMM_BY_X3) launch_linear_x3(a, r->M, r->K, wx, r->N, bn, bias, c, r->act, s);
    else if (r) launch_linear(a, r->M, r->K, wf, r->N, bias, c, r->act, s);
  };
  auto cf_gemm = [&](const float* a, const float* wgt, const float* bias, const float* res, float* c, int epi) {
    if (const GemmRow* r = next_row(true)) launch_cf_gemm(a, r->M, r->K, wgt, r->N, bias, res, c, epi, s);
  };
  // the head's input [M][512]: the sequence layer's output, or (no sequence
  // layer: no projection, no recurrence / MHA launch) the stage-8 buffer itself
  const float* HI = h->seq == SEQ_NONE && !h->decision ? S : Hs;
  if (h->decision) {
    // Cnn14_DecisionLevelAtt: max + avg pooling over 3 sequence frames inside fc1's A staging, + ReLU: one launch
    launch_decision(S, iB, T3, w.wfc, w.bfc, Hs, s);   // fc1 in the MultiHead fc's slots (weights.h)
  } else if (h->seq == SEQ_CONFORMER) {
    // (on either trunk) fp32 in every precision mode; x is updated in place by the residual epilogues
    float* X = ws + p.X.off;
    float* Xn = ws + p.Xn.off;
    float* Hb = ws + p.Hb.off;
    float* AV = ws + p.AV.off;
    float* Rr = ws + p.Rr.off;
    float* RK = ws + p.RK.off;
    const size_t nx = (size_t)M * CF_D;
    // r and r_k = r_net(r) of every block: on device, every forward
    launch_cf_relpos(w.cf_inv_freq, T3, CF_BLOCKS, Rr, s);
    for (int b = 0; b < CF_BLOCKS; ++b)
      cf_gemm(Rr + (size_t)b * T3 * CF_D, w.cf[b].rnet, nullptr, nullptr, RK + (size_t)b * T3 * CF_D, CF_EPI_NONE);
    // input layer (conformer_encoder.py:22-28): K = the trunk's width
    cf_gemm(S, w.cf_in_w, w.cf_in_b, nullptr, Xn, CF_EPI_NONE);
    launch_cf_input_norm(Xn, iB, T3, w.cf_in_g, w.cf_in_be, w.cf_pe, X, s);
    capture(h, 20, X, nx, s);
    for (int b = 0; b < CF_BLOCKS; ++b) {
      const CfBlockWeights& c = w.cf[b];
      auto ffn = [&](int f) {              // x = 0.5 ffn(x) + x
        launch_cf_layernorm(X, M, c.ffn_g[f], c.ffn_be[f], Xn, s);
        cf_gemm(Xn, c.ffn_w1[f], c.ffn_b1[f], nullptr, Hb, CF_EPI_SWISH);
        cf_gemm(Hb, c.ffn_w2[f], c.ffn_b2[f], X, X, CF_EPI_HALF_RES);
      };
      ffn(0);
      capture(h, 21 + 4 * b, X, nx, s);
      // mhsa: x = x + o_net(attention(qkv_net(LN(x))))
      launch_cf_layernorm(X, M, c.att_g, c.att_be, Xn, s);
      cf_gemm(Xn, c.wqkv, nullptr, nullptr, Hb, CF_EPI_NONE);
      (p.attn_mx ? launch_cf_relattn_mx : launch_cf_relattn)(Hb, iB, T3, RK + (size_t)b * T3 * CF_D, c.rwb, c.rrb, AV, s);
      cf_gemm(AV, c.wo, nullptr, X, X, CF_EPI_RES);
      capture(h, 22 + 4 * b, X, nx, s);
      // conv module: x = conv(x) + x
      launch_cf_layernorm(X, M, c.cv_g, c.cv_be, Xn, s);
      cf_gemm(Xn, c.pw1_w, c.pw1_b, nullptr, Hb, CF_EPI_NONE);
      launch_cf_glu_dwconv(Hb, iB, T3, c.dw_wt, c.dw_b, AV, s);
      cf_gemm(AV, c.pw2_w, c.pw2_b, X, X, CF_EPI_RES);
      capture(h, 23 + 4 * b, X, nx, s);
      ffn(1);
      launch_cf_layernorm(X, M, c.norm_g, c.norm_be, X, s);
      capture(h, 24 + 4 * b, X, nx, s);
    }
    HI = X;
  } else if (h->seq == SEQ_GRU) {
    linear(S, w.w_ih, w.w_ih_x3, 128, w.b_ih, G);
    if (h->depth == 14)
      launch_gru1024(G, iB, T3, w.whh, w.bhh, Hs, s);
    else if (p.gru_variant < 0)
      launch_gru(G, iB, T3, w.whhT, w.bhh, Hs, s);
    else
      launch_gru_coop(G, iB, T3, w.whh, w.bhh, Hs, ws + p.gru.off, !x3, p.gru_fast, p.gru_variant, h->gru_err_dev,
                      (unsigned)t.gru_spin, s, p.gru_spread);
  } else if (h->seq == SEQ_MHA) {
    linear(S, w.wqkv, w.wqkv_x3, 128, w.bqkv, G);
    launch_mha(G, iB, T3, O, s);
    linear(O, w.wfc, w.wfc_x3, 128, w.bfc, Hs);
  }
  capture(h, 9, HI, (size_t)M * h->hw, s);
  mark(h, 10, s);
  // head projection (att|cla rows or fc rows, zero-padded to nac), then its finish
  if (h->seq == SEQ_CONFORMER) cf_gemm(HI, w.wac, w.bac, nullptr, LG, CF_EPI_NONE);
  else linear(HI, w.wac, w.wac_x3, 64, w.bac, LG);
  if (drift || used != p.ngemms)
    return fail(h, SEDX_ESTATE, "the forward's GEMM launches (%d) are not the %d its plan lists", used, p.ngemms);
  const int C = h->cfg.classes_num, frames = (int)g.out_frames;
  float* emb_cla = h->emb == EMB_CLA ? d_emb : nullptr;
  switch (h->head_launch) {
    case HEAD_LAUNCH_VGG_ATT:   // x12, padded to 1000 frames
      launch_vgg_att_head(LG, iB, T3, C, h->nac, frames, g.rep, d_fw, d_clip, emb_cla, s);
      break;
    case HEAD_LAUNCH_VGG_FC:    // x(1000 // seq_len), padded to 1000 frames, the mean over all of them
      launch_vgg_fc_head(LG, iB, T3, C, h->nac, frames, g.rep, d_fw, d_clip, s);
      break;
    case HEAD_LAUNCH_ATT_REP:   // x(1000 // seq_len), padded to 1000 or the next multiple of 100
      capture(h, 44, LG, (size_t)M * h->nac, s);
      launch_att_head_rep(LG, iB, T3, C, h->nac, frames, g.rep, d_fw, d_clip, s);
      break;
    case HEAD_LAUNCH_TOKEN:     // logits as they stand: token 0 clipwise, tokens 1.. framewise
      capture(h, 44, LG, (size_t)M * h->nac, s);
      launch_token_head(LG, iB, T3, C, h->nac, d_fw, d_clip, s);
      break;
    case HEAD_LAUNCH_ATT: launch_att_head(LG, iB, T3, C, h->nac, frames, d_fw, d_clip, emb_cla, s, g.rep); break;
    default: launch_fc_head(LG, iB, T3, C, h->nac, h->head == HEAD_FC_MAX, d_fw, d_clip, s, frames);
  }
  if (h->emb == EMB_HEAD_INPUT && d_emb) launch_transpose_btd(HI, iB, T3, h->hw, d_emb, s);
  mark(h, 11, s);
  return launch_status(h);
}

}  // namespace

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

const char* sedx_version(void) {
  return "sedx 0.6 (abi 6; gfx950: fp32 MFMA exact direct conv | fp32 Winograd F(4x4,3x3) + F(2x2,3x3) | "
         "3xbf16-split MFMA | fp16 MFMA conv stack)";
}

int32_t sedx_abi_version(void) { return SEDX_ABI_VERSION; }

sedx_status sedx_set_precision(sedx_handle* h, int32_t mode) {
  if (!h) return SEDX_EINVAL;
  if (mode != SEDX_PRECISION_EXACT && mode != SEDX_PRECISION_X3 && mode != SEDX_PRECISION_WINOGRAD &&
      mode != SEDX_PRECISION_F16)
    return fail(h, SEDX_EINVAL, "unknown precision mode %d", mode);
  h->tune.precision = mode;
  return SEDX_OK;
}

const char* sedx_last_error(const sedx_handle* h) {
  if (h) return h->err.c_str();
  // handle-free entry points: average precision (cleared by a later
  // segment-count failure, so the latest of the two is reported), segment counts
  if (const char* rank = rank_error()) return rank;
  const char* seg = segment_error();
  return seg ? seg : "null handle";
}

sedx_status sedx_set_capture(sedx_handle* h, int32_t stage, float* d_buf, size_t bytes) {
  if (!h) return SEDX_EINVAL;
  if (stage < 0 || !d_buf) {
    h->cap_stage = -1;
    h->cap_buf = nullptr;
    h->cap_bytes = 0;
    return SEDX_OK;
  }
  const bool cf_stage = h->seq == SEQ_CONFORMER && stage >= 20 && stage <= 20 + 4 * CF_BLOCKS;
  const bool deep_stage = h->depth == 14 && stage >= 40 && stage <= 43;   // blocks 5-6 of the 14-layer trunk
  const bool vgg_stage = h->vgg && stage >= 50 && stage <= 55;            // the VGGish trunk's launches
  // Cnn_14layers_Conformer_FrameAtt's and Cnn_9layers_Conformer's logits
  const bool lg_stage = (h->head_launch == HEAD_LAUNCH_ATT_REP || h->head_launch == HEAD_LAUNCH_TOKEN) && stage == 44;
  if (h->vgg && stage >= 1 && stage <= 7) return fail(h, SEDX_EINVAL, "stage %d cannot be captured", (int)stage);
  if (stage == 1 || (stage > 9 && !cf_stage && !deep_stage && !vgg_stage && !lg_stage)) return fail(h, SEDX_EINVAL, "stage %d cannot be captured", (int)stage);
  h->cap_stage = stage;
  h->cap_buf = d_buf;
  h->cap_bytes = bytes;
  return SEDX_OK;
}

sedx_status sedx_set_tuning(sedx_handle* h, int32_t knob, int32_t value) {
  if (!h) return SEDX_EINVAL;
  static const struct {
    int knob, lo, hi;   // every value in [lo, hi] is one the header names
    int Tuning::*field;
  } knobs[] = {{SEDX_TUNE_GRU_KERNEL, SEDX_GRU_KERNEL_COOP, SEDX_GRU_KERNEL_PAIR, &Tuning::gru_kernel},
               {SEDX_TUNE_GRU_HANDOFF, SEDX_GRU_HANDOFF_AUTO, SEDX_GRU_HANDOFF_LOCAL, &Tuning::gru_handoff},
               {SEDX_TUNE_WINO_BLOCK1, 0, 2, &Tuning::wino_block1},
               {SEDX_TUNE_MEL_MFMA, 0, 1, &Tuning::mel_mfma},
               {SEDX_TUNE_GRU_SPIN, 0, INT32_MAX, &Tuning::gru_spin},
               {SEDX_TUNE_WINO_ORDER, 0, 3, &Tuning::wino_order},
               {SEDX_TUNE_GAMMA_SPEC, 0, 1, &Tuning::gamma_spec},
               {SEDX_TUNE_WINO_F43, 0, 2, &Tuning::wino_f43},
               {SEDX_TUNE_CF_ATTN, 0, 2, &Tuning::cf_attn}};
  for (const auto& k : knobs) {
    if (k.knob != knob) continue;
    if (value < k.lo || value > k.hi) return fail(h, SEDX_EINVAL, "bad value %d for tuning knob %d", (int)value, (int)knob);
    h->tune.*k.field = value;
    return SEDX_OK;
  }
  return fail(h, SEDX_EINVAL, "unknown tuning knob %d", (int)knob);
}

sedx_status sedx_check_error(sedx_handle* h) {
  if (!h) return SEDX_EINVAL;
  return check_async_error(h);
}

sedx_status sedx_create(const sedx_config* cfg, int device, sedx_handle** out) {
  if (!cfg || !out) return SEDX_EINVAL;
  *out = nullptr;
  if (cfg->mel_bins != 64) return SEDX_EINVAL;
  if (cfg->window_size != 256 && cfg->window_size != 512 && cfg->window_size != 1024) return SEDX_EINVAL;
  if (cfg->hop_size <= 0 || cfg->sample_rate <= 0 || cfg->classes_num <= 0 || cfg->classes_num > DECISION_MAX_CLASSES)
    return SEDX_EINVAL;
  if (cfg->feature_type == SEDX_FEATURE_GAMMA && cfg->model_type != SEDX_MODEL_GRU_FRAMEATT &&
      cfg->model_type != SEDX_MODEL_GRU_REG)   // the same forward before the head (models.py:2846-2850)
    return SEDX_EINVAL;
  Model m;   // after the range checks: nac is computed from classes_num
  if (!make_model(*cfg, &m) || cfg->classes_num > m.max_classes) return SEDX_EINVAL;
  sedx_handle* h = new sedx_handle();
  static_cast<Model&>(*h) = m;
  h->device = device;
  h->expected = expected_params(m);
  *out = h;
  return SEDX_OK;
}

void sedx_destroy(sedx_handle* h) {
  if (!h) return;
  {
    DeviceGuard g(h->device);
    for (auto& e : h->ev_last.ev)
      if (e) (void)hipEventDestroy(e);
    for (auto& set : h->ev_pool)
      for (auto& e : set.ev)
        if (e) (void)hipEventDestroy(e);
    if (h->conv_done) (void)hipEventDestroy(h->conv_done);
    if (h->blob) (void)hipFree(h->blob);
    if (h->ws) (void)hipFree(h->ws);
    if (h->gru_err_host) (void)hipHostFree(h->gru_err_host);
  }
  delete h;
}

sedx_status sedx_load_param(sedx_handle* h, const char* key, const float* h_data,
                            const int64_t* shape, int32_t ndim) {
  if (!h || !key || !h_data || (ndim > 0 && !shape) || ndim < 0 || ndim > 8) return SEDX_EINVAL;
  auto it = h->expected.find(key);
  if (it == h->expected.end() && ignored_key(*h, key)) {
    if (!ignored_key_shape_ok(*h, key, std::vector<int64_t>(shape, shape + ndim)))
      return fail(h, SEDX_EKEY, "size mismatch for %s", key);
    return SEDX_OK;
  }
  if (it == h->expected.end()) return fail(h, SEDX_EKEY, "unexpected key in state_dict: %s", key);
  std::vector<int64_t> sh(shape, shape + ndim);
  if (sh != it->second) return fail(h, SEDX_EKEY, "size mismatch for %s", key);
  int64_t n = 1;
  for (auto d : sh) n *= d;
  Tensor t;
  t.shape = sh;
  t.data.assign(h_data, h_data + n);
  h->params[key] = std::move(t);
  h->finalized = false;
  return SEDX_OK;
}

sedx_status sedx_finalize_weights(sedx_handle* h) {
  if (!h) return SEDX_EINVAL;
  // host work first, before any device call: the key check and every packed
  // layout, as the host image of one allocation (weights.cpp)
  DevWeights w;
  WeightBlob blob;
  GammaGeom gg;
  F16Weights wf16;
  if (sedx_status st = prepare_weights(*h, h->params, &w, &blob, &gg, &h->err, &wf16)) return st;
  DeviceGuard dg(h->device);
  if (h->blob) {
    (void)hipFree(h->blob);
    h->blob = nullptr;
    h->w = DevWeights();
    h->wf16 = F16Weights();
  }
  HIP_TRY(h, hipMalloc(&h->blob, blob.image.size()));
  HIP_TRY(h, hipMemcpy(h->blob, blob.image.data(), blob.image.size(), hipMemcpyHostToDevice));
  blob.bind(h->blob);   // sets w's and wf16's pointers
  h->w = w;
  h->wf16 = wf16;
  h->g_nfft = gg.nfft;
  h->g_hop = gg.hop;
  if (!h->gru_err_host) {
    void* p = nullptr;
    HIP_TRY(h, hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent));
    h->gru_err_host = static_cast<unsigned*>(p);
    *h->gru_err_host = 0;
    void* d = nullptr;
    HIP_TRY(h, hipHostGetDevicePointer(&d, p, 0));
    h->gru_err_dev = static_cast<unsigned*>(d);
  }
  h->finalized = true;
  return SEDX_OK;
}

sedx_status sedx_set_profiling(sedx_handle* h, int32_t on) {
  if (!h) return SEDX_EINVAL;
  if (on < 0 || on > 2) return fail(h, SEDX_EINVAL, "profiling mode %d (0 off, 1 last forward, 2 accumulate)", (int)on);
  DeviceGuard dg(h->device);
  if (on && !h->ev_last.ev[0])
    for (auto& e : h->ev_last.ev) HIP_TRY(h, hipEventCreate(&e));
  if (h->profiling == 2) fold_ev_pool(h);
  // mode 2: event sets for the first 64 forwards up front, so a timed loop
  // does not create events on the host while it issues work
  while (on == 2 && h->ev_pool.size() < 64) {
    h->ev_pool.emplace_back();
    for (auto& e : h->ev_pool.back().ev) HIP_TRY(h, hipEventCreate(&e));
  }
  h->profiling = on;
  for (auto& r : h->ev_last.rec) r = false;
  h->ev_used = 0;
  h->ev_cur = on == 1 ? &h->ev_last : nullptr;   // mode 2: mark() takes a set per forward
  for (int i = 0; i < SEDX_N_STAGES; ++i) {
    h->acc_ms[i] = 0.0;
    h->acc_n[i] = 0;
  }
  return SEDX_OK;
}

sedx_status sedx_set_pipelined(sedx_handle* h, int32_t on) {
  if (!h) return SEDX_EINVAL;
  if (on < 0 || on > 2) return fail(h, SEDX_EINVAL, "sedx_set_pipelined: on must be 0, 1 or 2");
  DeviceGuard dg(h->device);
  if (on && !h->conv_done) HIP_TRY(h, hipEventCreateWithFlags(&h->conv_done, hipEventDisableTiming));
  h->tune.pipelined = on != 0;
  h->tune.pipe_conv1_first = on == 2;
  h->conv_done_recorded = false;
  return SEDX_OK;
}

sedx_status sedx_stage_times(sedx_handle* h, float* ms, int32_t capacity, int32_t* n_stages) {
  if (!h || !n_stages) return SEDX_EINVAL;
  *n_stages = SEDX_N_STAGES;
  if (!h->profiling) return fail(h, SEDX_ESTATE, "profiling is off");
  DeviceGuard dg(h->device);
  if (sedx_status e = check_async_error(h)) return e;
  if (h->profiling == 2) fold_ev_pool(h);
  for (int i = 0; i < SEDX_N_STAGES; ++i) {
    float v = 0.f;
    bool rec = false;
    if (h->profiling == 2) {
      v = h->acc_n[i] ? (float)(h->acc_ms[i] / (double)h->acc_n[i]) : 0.f;
      h->acc_ms[i] = 0.0;
      h->acc_n[i] = 0;
    } else if (i < capacity) {
      HIP_TRY(h, stage_ms(h->ev_last, i, &v, &rec));
    }
    if (i < capacity) ms[i] = v;
  }
  return SEDX_OK;
}

sedx_status sedx_output_geometry(const sedx_handle* h, int64_t L_or_T, int64_t* out_frames,
                                 int64_t* seq_len) {
  if (!h || !out_frames || !seq_len) return SEDX_EINVAL;
  Geometry g;
  if (sedx_status st = query_geometry(h, L_or_T, &g)) return st;
  *out_frames = g.out_frames;
  *seq_len = g.Ts;
  return SEDX_OK;
}

sedx_status sedx_workspace_size(const sedx_handle* h, int64_t B, int64_t L_or_T, size_t* bytes) {
  if (!h || !bytes || B <= 0) return SEDX_EINVAL;
  Geometry g;
  if (sedx_status st = query_geometry(h, L_or_T, &g)) return st;
  ForwardPlan p;
  plan_forward(*h, h->tune, B, g.T, &p);   // the size of a shape no forward runs is still answered
  *bytes = p.total_bytes;
  return SEDX_OK;
}

sedx_status sedx_conv_launch_plan(const sedx_handle* h, int64_t B, int64_t L_or_T, int32_t ncu,
                                  sedx_conv_launch* rows, int32_t capacity, int32_t* n_rows) {
  if (!h || !n_rows || B <= 0 || capacity < 0 || (capacity && !rows)) return SEDX_EINVAL;
  *n_rows = 0;
  Geometry g;
  if (sedx_status st = query_geometry(h, L_or_T, &g)) return st;
  ForwardPlan p;
  if (const char* why = plan_forward(*h, h->tune, B, g.T, &p)) return fail(h, SEDX_EINVAL, "%s", why);
  if (ncu <= 0) {
    DeviceGuard dg(h->device);
    ncu = device_cus();
  }
  int n = 0;
  for (int i = 0; i < std::min(7, p.first_deep); ++i) {   // the launches of the 9-layer families (not conv_deep.hip's)
    const ConvLayer& c = p.layers[i];
    sedx_conv_launch r{};
    r.stage = 2 + i;
    r.family = p.family == CONV_X3 ? SEDX_CONV_X3 : p.family == CONV_F16 ? SEDX_CONV_F16 : SEDX_CONV_EXACT;
    r.T = c.T, r.F = c.F, r.cin = c.cin, r.cout = c.cout, r.epi = c.epi;
    WinoFamily wf;
    const bool wino = conv_launch_family(p, i, &wf);
    // run_body's arguments: the F(2x2) launchers take no layout flag and no counters
    const bool c4 = p.c4 && (!wino || wf != WINO_F23);
    int64_t b0 = 0;
    do {   // the launchers' loop over whole clips
      if (wino) {
        const ConvLaunch l = plan_conv_launch(wf, ncu, B - b0, c.T, c.F, c.cin, c.cout, c.epi, c.order, c4, 0,
                                              p.claims && wf == WINO_F43);
        if (l.reject) return fail(h, SEDX_EINVAL, "stage %d: %s", r.stage, l.reject);
        r.family = wf;
        r.clips = l.clips, r.tg = l.TG, r.nt = l.NT, r.c4 = c4;
        r.tb_per_clip = l.tb_per_clip, r.ngroups = l.ngroups, r.nitems = l.nitems, r.nwg = l.nwg;
        r.claim = l.claim, r.order2d = l.order2d;
        r.clips_per_launch = l.clips_per_launch;
      }
      if (n < capacity) rows[n] = r;
      ++n;
      b0 += wino ? r.clips : B;
    } while (b0 < B);
  }
  *n_rows = n;
  if (n > capacity) return fail(h, SEDX_EINVAL, "%d conv launches: capacity %d", n, capacity);
  return SEDX_OK;
}

sedx_status sedx_gemm_launch_plan(const sedx_handle* h, int64_t B, int64_t L_or_T, int32_t ncu,
                                  sedx_gemm_launch* rows, int32_t capacity, int32_t* n_rows) {
  if (!h || !n_rows || B <= 0 || capacity < 0 || (capacity && !rows)) return SEDX_EINVAL;
  *n_rows = 0;
  Geometry g;
  if (sedx_status st = query_geometry(h, L_or_T, &g)) return st;
  ForwardPlan p;
  if (const char* why = plan_forward(*h, h->tune, B, g.T, &p)) return fail(h, SEDX_EINVAL, "%s", why);
  if (ncu <= 0) {
    DeviceGuard dg(h->device);
    ncu = device_cus();
  }
  int n = 0;
  for (const GemmRow& r : plan_gemm_launches(p, ncu)) {   // run_body's launch order
    if (n < capacity) rows[n] = sedx_gemm_launch{r.stage, r.M, r.K, r.N, r.act, r.l.kernel, r.l.grid_x, r.l.grid_y};
    ++n;
  }
  *n_rows = n;
  if (n > capacity) return fail(h, SEDX_EINVAL, "%d GEMM launches: capacity %d", n, capacity);
  return SEDX_OK;
}

// the plan of B items of T frames (or why the forward refuses them) and its workspace
static sedx_status plan_and_workspace(sedx_handle* h, int64_t B, int64_t T, void* d_workspace,
                                      size_t workspace_bytes, ForwardPlan* p, float** ws) {
  if (const char* why = plan_forward(*h, h->tune, B, T, p)) return fail(h, SEDX_EINVAL, "%s", why);
  return get_ws(h, p->total_bytes, d_workspace, workspace_bytes, ws);
}

static sedx_status forward_wave(sedx_handle* h, const float* d_wave, const int16_t* d_wave16, int64_t B,
                                int64_t L, float* d_framewise, float* d_clipwise, float* d_embedding,
                                void* d_workspace, size_t workspace_bytes, void* stream) {
  if (sedx_status e = preflight(h)) return e;
  if (h->cfg.feature_type != SEDX_FEATURE_LOGMEL)
    return fail(h, SEDX_EINVAL, "gamma models take features: use sedx_forward_features");
  if ((!d_wave && !d_wave16) || !d_framewise || !d_clipwise || B <= 0)
    return fail(h, SEDX_EINVAL, "null pointer or empty batch");
  const int n2 = h->cfg.window_size / 2;
  if (L <= n2)
    return fail(h, SEDX_EINVAL, "input of %lld samples is too short for reflect padding of %d",
                (long long)L, n2);
  DeviceGuard dg(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ForwardPlan p;
  float* ws = nullptr;
  if (sedx_status st = plan_and_workspace(h, B, conv_T(*h, L), d_workspace, workspace_bytes, &p, &ws)) return st;
  mark(h, 0, s);
  run_logmel(h, p, ws, d_wave, d_wave16, L, B, 1, nullptr, L, L, s);
  return run_body(h, p, ws, d_framewise, d_clipwise, d_embedding, s);
}

sedx_status sedx_forward(sedx_handle* h, const float* d_wave, int64_t B, int64_t L,
                         float* d_framewise, float* d_clipwise, float* d_embedding,
                         void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_wave) return fail(h, SEDX_EINVAL, "null waveform pointer");
  return forward_wave(h, d_wave, nullptr, B, L, d_framewise, d_clipwise, d_embedding, d_workspace,
                      workspace_bytes, stream);
}

sedx_status sedx_forward_i16(sedx_handle* h, const int16_t* d_wave, int64_t B, int64_t L,
                             float* d_framewise, float* d_clipwise, float* d_embedding,
                             void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_wave) return fail(h, SEDX_EINVAL, "null waveform pointer");
  return forward_wave(h, nullptr, d_wave, B, L, d_framewise, d_clipwise, d_embedding, d_workspace,
                      workspace_bytes, stream);
}

sedx_status sedx_forward_features(sedx_handle* h, const float* d_feat, int64_t B, int64_t T,
                                  float* d_framewise, float* d_clipwise, float* d_embedding,
                                  void* d_workspace, size_t workspace_bytes, void* stream) {
  if (sedx_status e = preflight(h)) return e;
  if (!d_feat || !d_framewise || !d_clipwise || B <= 0 || T <= 0)
    return fail(h, SEDX_EINVAL, "null pointer or empty batch");
  DeviceGuard dg(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ForwardPlan p;
  float* ws = nullptr;
  if (sedx_status st = plan_and_workspace(h, B, T, d_workspace, workspace_bytes, &p, &ws)) return st;
  mark(h, 0, s);
  launch_features_bn0(d_feat, (int)B, (int)T, h->w.bn0_scale, h->w.bn0_mean, h->w.bn0_bias, ws + p.x0.off, s);
  return run_body(h, p, ws, d_framewise, d_clipwise, d_embedding, s);
}

sedx_status sedx_gamma_features(sedx_handle* h, const float* d_audio, int64_t B, int64_t L,
                                float* d_feat, int64_t* T_out, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
  if (sedx_status e = preflight(h)) return e;
  if (h->cfg.feature_type != SEDX_FEATURE_GAMMA)
    return fail(h, SEDX_EINVAL, "handle was not created with feature_type=gamma");
  if (L < h->g_nfft) return fail(h, SEDX_EINVAL, "clip shorter than the gammatone FFT");
  const GammaLayout lay = gamma_layout(B > 0 ? B : 1, L, h->g_nfft, h->g_hop);
  const int64_t T = lay.T;
  if (T_out) *T_out = T;
  if (!d_feat) return SEDX_OK;   // geometry query
  if (!d_audio || B <= 0) return fail(h, SEDX_EINVAL, "null pointer or empty batch");
  if (B > INT32_MAX / 64 || B * T > INT32_MAX / 64) return fail(h, SEDX_EINVAL, "batch too large");
  DeviceGuard dg(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* ws = nullptr;
  sedx_status st = get_ws(h, lay.total_bytes, d_workspace, workspace_bytes, &ws);
  if (st != SEDX_OK) return st;
  char* base = reinterpret_cast<char*>(ws);
  GammaParams p{};
  p.audio = d_audio;
  p.L = L;
  p.B = (int32_t)B;
  p.T = (int32_t)T;
  p.T_fill = (int32_t)lay.T_fill;
  p.hop = h->g_hop;
  p.nfft = h->g_nfft;
  p.kp = lay.kp;
  p.twiddle = reinterpret_cast<const double2*>(h->w.g_twiddle);
  p.window = h->w.g_window;
  p.weightsT = h->w.g_weightsT;
  p.mag = reinterpret_cast<double*>(base + lay.mag_off);
  p.db = reinterpret_cast<double*>(base + lay.db_off);
  p.mm = reinterpret_cast<unsigned long long*>(base + lay.mm_off);
  p.out = d_feat;
  launch_gamma(p, s, h->tune.gamma_spec);
  return launch_status(h);
}

sedx_status sedx_gamma_workspace_size(const sedx_handle* h, int64_t B, int64_t L, size_t* bytes) {
  if (!h) return SEDX_EINVAL;
  if (!bytes || B <= 0) return fail(h, SEDX_EINVAL, "null size pointer or empty batch");
  if (h->cfg.feature_type != SEDX_FEATURE_GAMMA)
    return fail(h, SEDX_EINVAL, "handle was not created with feature_type=gamma");
  if (!h->finalized) return fail(h, SEDX_ESTATE, "weights not finalised");
  if (L < h->g_nfft) return fail(h, SEDX_EINVAL, "clip shorter than the gammatone FFT");
  *bytes = gamma_layout(B, L, h->g_nfft, h->g_hop).total_bytes;
  return SEDX_OK;
}

sedx_status sedx_gamma_workspace_layout(const sedx_handle* h, int64_t B, int64_t L, sedx_gamma_layout* out) {
  if (!h) return SEDX_EINVAL;
  if (!out || B <= 0) return fail(h, SEDX_EINVAL, "null layout pointer or empty batch");
  if (h->cfg.feature_type != SEDX_FEATURE_GAMMA)
    return fail(h, SEDX_EINVAL, "handle was not created with feature_type=gamma");
  // the sizes follow from the configuration alone: no weights, no device
  GammaGeom gg;
  if (!gamma_geometry(h->cfg.sample_rate, h->cfg.window_size, h->cfg.hop_size, &gg))
    return fail(h, SEDX_EINVAL, "gammatone nfft %d unsupported", gg.nfft);
  if (L < gg.nfft) return fail(h, SEDX_EINVAL, "clip shorter than the gammatone FFT");
  const GammaLayout lay = gamma_layout(B, L, gg.nfft, gg.hop);
  out->T = lay.T;
  out->T_fill = lay.T_fill;
  out->nfft = gg.nfft;
  out->hop = gg.hop;
  out->kp = lay.kp;
  out->reserved = 0;
  out->mag_offset = lay.mag_off;
  out->db_offset = lay.db_off;
  out->mm_offset = lay.mm_off;
  out->total_bytes = lay.total_bytes;
  return SEDX_OK;
}

// ---- one call from audio, whatever the model's features -------------------------
// the geometry of B clips of L samples through the model's own frontend (what sedx_forward_audio runs)
static sedx_status audio_query(const sedx_handle* h, int64_t L, Geometry* g) {
  char buf[96];
  if (const char* why = audio_refusal(*h, L, buf, sizeof(buf))) return fail(h, SEDX_EINVAL, "%s", why);
  *g = geometry_from_T(*h, audio_T(*h, L));
  if (const char* why = shape_refusal(*h, g->T, buf, sizeof(buf))) return fail(h, SEDX_EINVAL, "%s", why);
  return SEDX_OK;
}

sedx_status sedx_audio_geometry(const sedx_handle* h, int64_t L, int64_t* T, int64_t* out_frames, int64_t* seq_len) {
  if (!h) return SEDX_EINVAL;
  Geometry g;
  if (sedx_status st = audio_query(h, L, &g)) return st;
  if (T) *T = g.T;
  if (out_frames) *out_frames = g.out_frames;
  if (seq_len) *seq_len = g.Ts;
  return SEDX_OK;
}

sedx_status sedx_audio_workspace_size(const sedx_handle* h, int64_t B, int64_t L, size_t* bytes) {
  if (!h) return SEDX_EINVAL;
  if (!bytes || B <= 0) return fail(h, SEDX_EINVAL, "null size pointer or empty batch");
  Geometry g;
  if (sedx_status st = audio_query(h, L, &g)) return st;
  if (h->cfg.feature_type == SEDX_FEATURE_GAMMA && B > 65535)
    return fail(h, SEDX_EINVAL, "forward too large: %lld items (the gammatone frontend runs at most 65535)", (long long)B);
  *bytes = audio_layout(*h, h->tune, B, L).total_bytes;
  return SEDX_OK;
}

sedx_status sedx_forward_audio(sedx_handle* h, const float* d_audio, int64_t B, int64_t L, float* d_framewise,
                               float* d_clipwise, float* d_embedding, void* d_workspace, size_t workspace_bytes,
                               void* stream) {
  if (!h) return SEDX_EINVAL;
  if (h->cfg.feature_type != SEDX_FEATURE_GAMMA)
    return sedx_forward(h, d_audio, B, L, d_framewise, d_clipwise, d_embedding, d_workspace, workspace_bytes, stream);
  if (sedx_status e = preflight(h)) return e;
  if (!d_audio || !d_framewise || !d_clipwise || B <= 0) return fail(h, SEDX_EINVAL, "null pointer or empty batch");
  Geometry g;
  if (sedx_status st = audio_query(h, L, &g)) return st;
  if (B > 65535 || B * g.T > INT32_MAX / 64) return fail(h, SEDX_EINVAL, "batch too large");
  DeviceGuard dg(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const AudioLayout al = audio_layout(*h, h->tune, B, L);
  ForwardPlan p;
  if (const char* why = plan_forward(*h, h->tune, B, g.T, &p)) return fail(h, SEDX_EINVAL, "%s", why);
  float* ws = nullptr;
  if (sedx_status st = get_ws(h, al.total_bytes, d_workspace, workspace_bytes, &ws)) return st;
  mark(h, 0, s);
  // B items of one window each: clip b's L samples at b * L (all backed); every base is even when L is
  if (sedx_status st = run_gamma_items(h, p, ws, reinterpret_cast<char*>(ws) + al.fe, d_audio, L, 1, nullptr, L, L,
                                       L % 2 == 0, s))
    return st;
  return run_body(h, p, ws, d_framewise, d_clipwise, d_embedding, s);
}

// host-side failures of the window entry points (plan vectors) become
// status codes instead of exceptions crossing the C ABI
#define SEDX_HOST_TRY(h, body)                                                              \
  try {                                                                                     \
    body                                                                                    \
  } catch (const std::bad_alloc&) {                                                         \
    return fail(h, SEDX_ENOMEM, "host allocation failed (merge plan)");                     \
  } catch (...) {                                                                           \
    return fail(h, SEDX_EINVAL, "host-side failure building the window plan");              \
  }

sedx_status sedx_window_geometry(const sedx_handle* h, int64_t L_clip, const sedx_window_spec* spec,
                                 int64_t* n_windows, int64_t* window_samples, int64_t* merged_frames) {
  if (!h) return SEDX_EINVAL;
  SEDX_HOST_TRY(h, {
    WinGeom wg;
    // the plan of the forward the spec names: avg_merge rejects a zero step
    if (const char* why = window_geometry(*h, L_clip, spec, spec && spec->vote == 0, &wg))
      return fail(h, SEDX_EINVAL, "%s", why);
    if (n_windows) *n_windows = wg.n_win;
    if (window_samples) *window_samples = wg.full_len;
    if (merged_frames) *merged_frames = wg.plan.N;
    return SEDX_OK;
  })
}

// every window of every clip through the model (one batch per window group),
// then the merge by the host's plan (avg or vote)
static sedx_status forward_windows_impl(sedx_handle* h, const float* d_audio, int64_t n_clips, int64_t L_clip,
                                        const sedx_window_spec* spec, const double* h_vote_thres, float* d_merged,
                                        void* d_workspace, size_t workspace_bytes, void* stream) {
  if (sedx_status e = preflight(h)) return e;
  const bool gamma = h->cfg.feature_type == SEDX_FEATURE_GAMMA;   // its windows go through the gammatone frontend
  if (!d_audio || !d_merged || n_clips <= 0) return fail(h, SEDX_EINVAL, "null pointer or empty batch");
  if (spec && spec->vote != 0 && h_vote_thres == nullptr)
    return fail(h, SEDX_EINVAL, "spec.vote = 1: call sedx_forward_windows_vote");
  WinGeom wg;
  if (const char* why = window_geometry(*h, L_clip, spec, h_vote_thres == nullptr, &wg))
    return fail(h, SEDX_EINVAL, "%s", why);
  // the frontend and conv launches index items with 32-bit sizes (as forward_wave)
  for (const auto& g : wg.groups)
    if (n_clips > INT32_MAX / g.nw || n_clips * g.nw * g.g.T > INT32_MAX / 64)
      return fail(h, SEDX_EINVAL, "batch too large: %lld clips x %d windows", (long long)n_clips, g.nw);
  if (n_clips * wg.plan.N > INT32_MAX / h->cfg.classes_num)
    return fail(h, SEDX_EINVAL, "merged output too large");
  DeviceGuard dg(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const WinLayout wl = win_layout(*h, h->tune, n_clips, wg);
  float* ws = nullptr;
  if (sedx_status st = get_ws(h, wl.total_bytes, d_workspace, workspace_bytes, &ws)) return st;
  const int C = h->cfg.classes_num;
  // tables: built on the host, one copy (the host vector is consumed by the
  // call: pageable-source hipMemcpyAsync stages it before returning)
  std::vector<char> blob(wl.table_bytes, 0);
  int64_t* t_start = reinterpret_cast<int64_t*>(blob.data() + wl.t_start);
  int64_t* t_wb = reinterpret_cast<int64_t*>(blob.data() + wl.t_wb);
  int64_t* t_wcs = reinterpret_cast<int64_t*>(blob.data() + wl.t_wcs);
  int32_t* t_off = reinterpret_cast<int32_t*>(blob.data() + wl.t_off);
  int2* t_src = reinterpret_cast<int2*>(blob.data() + wl.t_src);
  int32_t* t_div = reinterpret_cast<int32_t*>(blob.data() + wl.t_div);
  std::copy(wg.loop.start.begin(), wg.loop.start.end(), t_start);
  for (size_t gi = 0; gi < wg.groups.size(); ++gi) {
    const WinGroup& g = wg.groups[gi];
    for (int i = 0; i < g.nw; ++i) {
      t_wb[g.w0 + i] = (int64_t)(wl.fw_off[gi] - wl.model_bytes / sizeof(float)) + (int64_t)i * g.g.out_frames * C;
      t_wcs[g.w0 + i] = (int64_t)g.nw * g.g.out_frames * C;
    }
  }
  std::copy(wg.plan.off.begin(), wg.plan.off.end(), t_off);
  for (size_t j = 0; j < wg.plan.src.size(); ++j) {
    const int32_t id = wg.plan.src[j];
    const int w = (int)(std::upper_bound(wg.plan.win_base.begin(), wg.plan.win_base.end(), id) -
                        wg.plan.win_base.begin()) - 1;
    t_src[j] = make_int2(w, id - wg.plan.win_base[w]);
  }
  std::copy(wg.plan.div.begin(), wg.plan.div.end(), t_div);
  char* d_tables = reinterpret_cast<char*>(ws + wl.tables);
  HIP_TRY(h, hipMemcpyAsync(d_tables, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
  double* vthr = reinterpret_cast<double*>(ws + wl.vthr);
  if (h_vote_thres) HIP_TRY(h, hipMemcpyAsync(vthr, h_vote_thres, C * sizeof(double), hipMemcpyHostToDevice, s));
  const int64_t* d_start = reinterpret_cast<const int64_t*>(d_tables + wl.t_start);
  mark(h, 0, s);
  for (size_t gi = 0; gi < wg.groups.size(); ++gi) {
    const WinGroup& g = wg.groups[gi];
    ForwardPlan p;
    if (const char* why = plan_forward(*h, h->tune, n_clips * g.nw, g.g.T, &p)) return fail(h, SEDX_EINVAL, "%s", why);
    if (gamma) {
      // the one-wave spectrum kernel's 8-byte loads: clip c's window i starts at c * L_clip + start[i]
      bool even = L_clip % 2 == 0;
      for (int i = 0; i < g.nw; ++i) even = even && wg.loop.start[g.w0 + i] % 2 == 0;
      if (sedx_status st = run_gamma_items(h, p, ws, reinterpret_cast<char*>(ws) + wl.fe, d_audio, L_clip, g.nw,
                                           d_start + g.w0, wg.clip_len, g.len, even, s))
        return st;
    } else
      run_logmel(h, p, ws, d_audio, nullptr, L_clip, n_clips, g.nw, d_start + g.w0, wg.clip_len, g.len, s);
    if (sedx_status st = run_body(h, p, ws, ws + wl.fw_off[gi], ws + wl.clip_off[gi], nullptr, s)) return st;
  }
  MergeArgs a{};
  a.fw = ws + wl.model_bytes / sizeof(float);
  a.wb = reinterpret_cast<const int64_t*>(d_tables + wl.t_wb);
  a.wcs = reinterpret_cast<const int64_t*>(d_tables + wl.t_wcs);
  a.off = reinterpret_cast<const int32_t*>(d_tables + wl.t_off);
  a.src = reinterpret_cast<const int2*>(d_tables + wl.t_src);
  a.div = reinterpret_cast<const int32_t*>(d_tables + wl.t_div);
  a.vote_thr = h_vote_thres ? vthr : nullptr;
  a.n_clips = (int32_t)n_clips;
  a.N = (int32_t)wg.plan.N;
  a.C = C;
  a.merged = d_merged;
  launch_merge_plan(a, s);
  return launch_status(h);
}

sedx_status sedx_window_workspace_size(const sedx_handle* h, int64_t n_clips, int64_t L_clip,
                                       const sedx_window_spec* spec, size_t* bytes) {
  if (!h || !bytes || n_clips <= 0) return SEDX_EINVAL;
  SEDX_HOST_TRY(h, {
    WinGeom wg;
    if (const char* why = window_geometry(*h, L_clip, spec, spec && spec->vote == 0, &wg))
      return fail(h, SEDX_EINVAL, "%s", why);
    *bytes = win_layout(*h, h->tune, n_clips, wg).total_bytes;
    return SEDX_OK;
  })
}

sedx_status sedx_forward_windows(sedx_handle* h, const float* d_audio, int64_t n_clips, int64_t L_clip,
                                 const sedx_window_spec* spec, float* d_merged, void* d_workspace,
                                 size_t workspace_bytes, void* stream) {
  if (!h) return SEDX_EINVAL;
  SEDX_HOST_TRY(h, {
    return forward_windows_impl(h, d_audio, n_clips, L_clip, spec, nullptr, d_merged, d_workspace, workspace_bytes,
                                stream);
  })
}

sedx_status sedx_forward_windows_vote(sedx_handle* h, const float* d_audio, int64_t n_clips, int64_t L_clip,
                                      const sedx_window_spec* spec, const double* bin_thres, float* d_votes,
                                      void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!h) return SEDX_EINVAL;
  if (!bin_thres) return fail(h, SEDX_EINVAL, "vote mode needs the per-class binarisation thresholds");
  SEDX_HOST_TRY(h, {
    return forward_windows_impl(h, d_audio, n_clips, L_clip, spec, bin_thres, d_votes, d_workspace, workspace_bytes,
                                stream);
  })
}
// ---- the ragged form of the predict driver: clips of different lengths in one call ----
// One inference asks for the same plan three times (geometry, workspace size, forward), and a clip's merge plan
// costs about a millisecond of host time to build: the handle keeps the last accepted plan with its question.
static const char* ragged_geometry_of(const sedx_handle* hc, const int64_t* len, int64_t n,
                                      const sedx_window_spec* spec, const double* dur, const RaggedGeom** out) {
  sedx_handle::RaggedMemo& m = const_cast<sedx_handle*>(hc)->ragged_memo;
  if (m.valid && spec && len && n > 0 && (size_t)n == m.len.size() && std::equal(len, len + n, m.len.begin()) &&
      m.has_dur == (dur != nullptr) && (!dur || std::equal(dur, dur + n, m.dur.begin())) &&
      spec->driver == m.spec.driver && spec->overlap == m.spec.overlap && spec->vote == m.spec.vote &&
      spec->sample_duration == m.spec.sample_duration && spec->overlap_value == m.spec.overlap_value &&
      spec->audio_duration == m.spec.audio_duration) {
    *out = &m.rg;
    return nullptr;
  }
  m.valid = false;
  if (const char* why = ragged_geometry(*hc, len, n, spec, dur, &m.rg)) return why;   // (why points into m.rg)
  m.len.assign(len, len + n);
  m.has_dur = dur != nullptr;
  if (dur) m.dur.assign(dur, dur + n);
  m.spec = *spec;
  m.valid = true;
  *out = &m.rg;
  return nullptr;
}

sedx_status sedx_ragged_window_geometry(const sedx_handle* h, const int64_t* h_clip_len, int64_t n_clips,
                                        const sedx_window_spec* spec, const double* h_audio_duration,
                                        int64_t* h_n_windows, int64_t* h_frame_off, int64_t* window_samples,
                                        int64_t* total_windows) {
  if (!h) return SEDX_EINVAL;
  SEDX_HOST_TRY(h, {
    const RaggedGeom* prg = nullptr;
    if (const char* why = ragged_geometry_of(h, h_clip_len, n_clips, spec, h_audio_duration, &prg))
      return fail(h, SEDX_EINVAL, "%s", why);
    const RaggedGeom& rg = *prg;
    if (h_n_windows) std::copy(rg.n_win.begin(), rg.n_win.end(), h_n_windows);
    if (h_frame_off) std::copy(rg.frame_off.begin(), rg.frame_off.end(), h_frame_off);
    if (window_samples) *window_samples = rg.full_len;
    if (total_windows) *total_windows = rg.item_off.back();
    return SEDX_OK;
  })
}

sedx_status sedx_ragged_window_workspace_size(const sedx_handle* h, const int64_t* h_clip_len, int64_t n_clips,
                                              const sedx_window_spec* spec, const double* h_audio_duration,
                                              int64_t items_per_forward, size_t* bytes) {
  if (!h) return SEDX_EINVAL;
  if (!bytes) return fail(h, SEDX_EINVAL, "null size pointer");
  SEDX_HOST_TRY(h, {
    const RaggedGeom* prg = nullptr;
    if (const char* why = ragged_geometry_of(h, h_clip_len, n_clips, spec, h_audio_duration, &prg))
      return fail(h, SEDX_EINVAL, "%s", why);
    const RaggedGeom& rg = *prg;
    *bytes = ragged_layout(*h, h->tune, rg, items_per_forward).total_bytes;
    return SEDX_OK;
  })
}

// every window of every clip as one item list through the model, in forwards
// of at most items_per_forward items, then every clip's own merge
static sedx_status forward_windows_ragged_impl(sedx_handle* h, const float* d_audio, const int64_t* h_clip_off,
                                               int64_t n_clips, const sedx_window_spec* spec,
                                               const double* h_audio_duration, int64_t items_per_forward,
                                               float* d_merged, void* d_workspace, size_t workspace_bytes,
                                               void* stream) {
  if (sedx_status e = preflight(h)) return e;
  const bool gamma = h->cfg.feature_type == SEDX_FEATURE_GAMMA;   // its windows go through the gammatone frontend
  if (!d_audio || !d_merged || !h_clip_off || n_clips <= 0)
    return fail(h, SEDX_EINVAL, "null pointer or empty batch");
  std::vector<int64_t> len((size_t)n_clips);
  for (int64_t c = 0; c < n_clips; ++c) {
    len[c] = h_clip_off[c + 1] - h_clip_off[c];
    if (h_clip_off[c] < 0 || len[c] < 0)
      return fail(h, SEDX_EINVAL, "clip %lld: the clip offsets must be non-negative and non-decreasing", (long long)c);
  }
  const RaggedGeom* prg = nullptr;
  if (const char* why = ragged_geometry_of(h, len.data(), n_clips, spec, h_audio_duration, &prg))
    return fail(h, SEDX_EINVAL, "%s", why);
  const RaggedGeom& rg = *prg;
  const RaggedLayout rl = ragged_layout(*h, h->tune, rg, items_per_forward);
  // the frontend and conv launches index items with 32-bit sizes (as forward_wave)
  if (rl.chunk > INT32_MAX || rl.chunk * rg.g.T > INT32_MAX / 64)
    return fail(h, SEDX_EINVAL, "forward too large: %lld windows (lower items_per_forward)", (long long)rl.chunk);
  DeviceGuard dg(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* ws = nullptr;
  if (sedx_status st = get_ws(h, rl.total_bytes, d_workspace, workspace_bytes, &ws)) return st;
  const int C = h->cfg.classes_num;
  // tables: built on the host, one copy (consumed by the call, as in forward_windows_impl)
  std::vector<char> blob;
  ragged_tables(rg, rl, h_clip_off, &blob);
  char* d_tables = reinterpret_cast<char*>(ws + rl.tables);
  HIP_TRY(h, hipMemcpyAsync(d_tables, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
  const ItemRow* d_item = reinterpret_cast<const ItemRow*>(d_tables + rl.t_item);
  const int64_t item_floats = rg.g.out_frames * C;
  // (gamma) the one-wave spectrum kernel's 8-byte loads want every item's first sample at an even offset:
  // clips of odd lengths put the clips after them at odd ones, and those calls keep the Stockham kernel
  bool even_bases = true;
  if (gamma) {
    const ItemRow* rows = reinterpret_cast<const ItemRow*>(blob.data() + rl.t_item);
    for (int64_t i = 0; i < rl.items; ++i) even_bases = even_bases && rows[i].src % 2 == 0;
  }
  mark(h, 0, s);
  for (int64_t i0 = 0; i0 < rl.items; i0 += rl.chunk) {
    const int64_t n = std::min(rl.chunk, rl.items - i0);
    ForwardPlan p;
    if (const char* why = plan_forward(*h, h->tune, n, rg.g.T, &p)) return fail(h, SEDX_EINVAL, "%s", why);
    // n items of one window each, their sources from the item table at i0
    if (gamma) {
      if (sedx_status st = run_gamma_items(h, p, ws, reinterpret_cast<char*>(ws) + rl.fe, d_audio, 0, 1, nullptr,
                                           rg.full_len, rg.full_len, even_bases, s, d_item + i0))
        return st;
    } else
      run_logmel(h, p, ws, d_audio, nullptr, 0, n, 1, nullptr, rg.full_len, rg.full_len, s, d_item + i0);
    if (sedx_status st = run_body(h, p, ws, ws + rl.fw + i0 * item_floats, ws + rl.clipwise, nullptr, s)) return st;
  }
  RaggedMergeArgs a{};
  a.fw = ws + rl.fw;
  a.item_floats = item_floats;
  a.crow = reinterpret_cast<const RaggedClipRow*>(d_tables + rl.t_clip);
  a.off = reinterpret_cast<const int32_t*>(d_tables + rl.t_off);
  a.src = reinterpret_cast<const int2*>(d_tables + rl.t_src);
  a.div = reinterpret_cast<const int32_t*>(d_tables + rl.t_div);
  a.n_clips = (int32_t)n_clips;
  a.rows = (int32_t)rg.frame_off.back();
  a.C = C;
  a.merged = d_merged;
  launch_merge_ragged(a, s);
  return launch_status(h);
}

sedx_status sedx_forward_windows_ragged(sedx_handle* h, const float* d_audio, const int64_t* h_clip_off,
                                        int64_t n_clips, const sedx_window_spec* spec,
                                        const double* h_audio_duration, int64_t items_per_forward, float* d_merged,
                                        void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!h) return SEDX_EINVAL;
  SEDX_HOST_TRY(h, {
    return forward_windows_ragged_impl(h, d_audio, h_clip_off, n_clips, spec, h_audio_duration, items_per_forward,
                                       d_merged, d_workspace, workspace_bytes, stream);
  })
}
#undef SEDX_HOST_TRY

sedx_status sedx_events_ragged_workspace_size(const int64_t* h_frame_off, int64_t n_clips, int64_t C, size_t* bytes) {
  if (!bytes || !h_frame_off || n_clips < 0 || C <= 0) return SEDX_EINVAL;
  int64_t tmax = 0;
  for (int64_t c = 0; c < n_clips; ++c) {
    if (h_frame_off[c + 1] < h_frame_off[c]) return SEDX_EINVAL;
    tmax = std::max(tmax, h_frame_off[c + 1] - h_frame_off[c]);
  }
  *bytes = events_workspace_bytes(n_clips * C, tmax, C) + align256((size_t)(n_clips + 1) * 8);
  return SEDX_OK;
}

sedx_status sedx_events_device_ragged(const float* d_x, const int64_t* h_frame_off, int64_t n_clips, int64_t C,
                                      const double* high_thres, const double* low_thres, int32_t use_low_thres,
                                      const int64_t* n_smooth, const int64_t* n_salt, int32_t* d_events,
                                      int64_t capacity, int64_t* d_info, void* d_workspace, size_t workspace_bytes,
                                      void* stream) {
  if (n_clips < 0 || C <= 0 || !h_frame_off || !d_info || !n_smooth || !n_salt || !high_thres ||
      (capacity > 0 && !d_events) || capacity < 0 || (use_low_thres && !low_thres))
    return SEDX_EINVAL;
  size_t need = 0;
  if (sedx_events_ragged_workspace_size(h_frame_off, n_clips, C, &need) != SEDX_OK) return SEDX_EINVAL;
  int64_t tmax = 0;
  for (int64_t c = 0; c < n_clips; ++c) tmax = std::max(tmax, h_frame_off[c + 1] - h_frame_off[c]);
  if (n_clips > 0 && h_frame_off[n_clips] > h_frame_off[0] && !d_x) return SEDX_EINVAL;
  if (tmax > events_max_frames()) return SEDX_EINVAL;   // a series' two bitmaps live in LDS
  if (!d_workspace || workspace_bytes < need) return SEDX_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // counts, slots, then one packed block: the per-class parameters (as sedx_events_device) and the frame offsets
  char* p = static_cast<char*>(d_workspace);
  int64_t* counts = reinterpret_cast<int64_t*>(p);
  p += align256(n_clips * C * 8);
  int64_t* slots = reinterpret_cast<int64_t*>(p);
  p += align256(n_clips * C * events_slot_cap(tmax) * 8);
  const size_t o_hi = 0, o_lo = align256(C * 4), o_ns = o_lo + align256(C * 8), o_salt = o_ns + align256(C * 8);
  const size_t o_foff = o_salt + align256(C * 8);
  std::vector<char> blob(o_foff + (size_t)(n_clips + 1) * 8, 0);
  for (int64_t k = 0; k < C; ++k) {
    reinterpret_cast<float*>(blob.data() + o_hi)[k] = (float)high_thres[k];
    reinterpret_cast<double*>(blob.data() + o_lo)[k] = use_low_thres ? low_thres[k] : 0.0;
    reinterpret_cast<int64_t*>(blob.data() + o_ns)[k] = n_smooth[k];
    reinterpret_cast<int64_t*>(blob.data() + o_salt)[k] = n_salt[k];
  }
  std::memcpy(blob.data() + o_foff, h_frame_off, (size_t)(n_clips + 1) * 8);
  if (hipMemcpyAsync(p, blob.data(), blob.size(), hipMemcpyHostToDevice, s) != hipSuccess) return SEDX_EHIP;
  EventArgs a{d_x, n_clips, tmax, C, reinterpret_cast<const float*>(p + o_hi),
              reinterpret_cast<const double*>(p + o_lo), reinterpret_cast<const int64_t*>(p + o_ns),
              reinterpret_cast<const int64_t*>(p + o_salt), use_low_thres, 0, 0, counts, slots,
              events_slot_cap(tmax), d_info, d_events, capacity};
  launch_events_ragged(a, reinterpret_cast<const int64_t*>(p + o_foff), s);
  if (take_launch_error() != hipSuccess) return SEDX_EHIP;
  return hipGetLastError() == hipSuccess ? SEDX_OK : SEDX_EHIP;
}

sedx_status sedx_events_workspace_size(int64_t n_clips, int64_t T, int64_t C, size_t* bytes) {
  if (!bytes || n_clips < 0 || T < 0 || C <= 0) return SEDX_EINVAL;
  *bytes = events_workspace_bytes(n_clips * C, T, C);
  return SEDX_OK;
}

sedx_status sedx_events_device(const float* d_x, int64_t n_clips, int64_t T, int64_t C,
                               const double* high_thres, const double* low_thres,
                               int32_t use_low_thres, const int64_t* n_smooth, const int64_t* n_salt,
                               int32_t mode, double overlap_value, int32_t sample_duration,
                               int32_t* d_events, int64_t capacity, int64_t* d_info,
                               void* d_workspace, size_t workspace_bytes, void* stream) {
  if (n_clips < 0 || T < 0 || C <= 0 || !d_info || !n_smooth || !n_salt || (mode != 0 && mode != 1) ||
      (n_clips > 0 && !d_x) || (capacity > 0 && !d_events) || capacity < 0 ||
      (use_low_thres && !low_thres) || (mode == 0 && !high_thres))
    return SEDX_EINVAL;
  // int(100 * overlap_value) in float64 (vad.py:63)
  if (mode == 1 && !(std::fabs(100.0 * overlap_value) < 1e9)) return SEDX_EINVAL;
  const int64_t step = mode == 1 ? (int64_t)(100.0 * overlap_value) : 0;
  // step 0: range(0, N - 0, 0) raises; step < 0: the range is empty, no
  // frame is ever a candidate and the reference returns no events
  if (mode == 1 && (step == 0 || sample_duration <= 0)) return SEDX_EINVAL;
  if (T > events_max_frames()) return SEDX_EINVAL;   // a series' two bitmaps live in LDS
  const size_t need = events_workspace_bytes(n_clips * C, T, C);
  if (!d_workspace || workspace_bytes < need) return SEDX_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // per-class parameters -> one packed block in the workspace, one copy
  // (f32 high: the mode-0 compare is float32)
  char* p = static_cast<char*>(d_workspace);
  int64_t* counts = reinterpret_cast<int64_t*>(p);
  p += align256(n_clips * C * 8);
  int64_t* slots = reinterpret_cast<int64_t*>(p);
  p += align256(n_clips * C * events_slot_cap(T) * 8);
  const size_t o_hi = 0, o_lo = align256(C * 4), o_ns = o_lo + align256(C * 8), o_salt = o_ns + align256(C * 8);
  std::vector<char> blob(o_salt + C * 8, 0);
  for (int64_t k = 0; k < C; ++k) {
    reinterpret_cast<float*>(blob.data() + o_hi)[k] = high_thres ? (float)high_thres[k] : 0.f;
    reinterpret_cast<double*>(blob.data() + o_lo)[k] = use_low_thres ? low_thres[k] : 0.0;
    reinterpret_cast<int64_t*>(blob.data() + o_ns)[k] = n_smooth[k];
    reinterpret_cast<int64_t*>(blob.data() + o_salt)[k] = n_salt[k];
  }
  if (hipMemcpyAsync(p, blob.data(), blob.size(), hipMemcpyHostToDevice, s) != hipSuccess) return SEDX_EHIP;
  const float* d_hi = reinterpret_cast<const float*>(p + o_hi);
  const double* d_lo = reinterpret_cast<const double*>(p + o_lo);
  const int64_t* d_ns = reinterpret_cast<const int64_t*>(p + o_ns);
  const int64_t* d_nsalt = reinterpret_cast<const int64_t*>(p + o_salt);
  EventArgs a{d_x, n_clips, T, C, d_hi, d_lo, d_ns, d_nsalt, use_low_thres,
              step, (int64_t)sample_duration, counts, slots, events_slot_cap(T), d_info, d_events,
              capacity};
  launch_events(a, mode, s);
  if (take_launch_error() != hipSuccess) return SEDX_EHIP;
  return hipGetLastError() == hipSuccess ? SEDX_OK : SEDX_EHIP;
}

sedx_status sedx_segment_counts_workspace_size(int64_t n_clips, int64_t T, int64_t C, int64_t V, size_t* bytes) {
  if (!bytes || n_clips < 0 || T < 0 || C <= 0 || V < 1 || V > 64) return SEDX_EINVAL;
  *bytes = calib_workspace_bytes(C, V);
  return SEDX_OK;
}

sedx_status sedx_segment_counts_device(const float* d_x, int64_t n_clips, int64_t T, int64_t C,
                                       const uint64_t* d_target, int64_t segment_frames, int64_t V,
                                       const double* high, const double* low, const int64_t* n_smooth,
                                       const int64_t* n_salt, int64_t* d_counts, void* d_workspace,
                                       size_t workspace_bytes, void* stream) {
  const sedx_status chk = segment_counts_check(n_clips, T, C, segment_frames, V);
  if (chk != SEDX_OK) return chk;
  if (!high || !low || !n_smooth || !n_salt || !d_counts || (n_clips > 0 && (!d_x || !d_target)))
    return segment_fail("segment counts: null argument");
  if (T > calib_max_frames())                       // a series' two bitmaps live in LDS
    return segment_fail("segment counts: T = %lld frames, the device path holds at most %lld", (long long)T,
                        (long long)calib_max_frames());
  if (n_clips * C >= (int64_t(1) << 31)) return segment_fail("segment counts: too many series for one launch");
  const size_t need = calib_workspace_bytes(C, V);
  if (!d_workspace || workspace_bytes < need)
    return segment_fail("segment counts: workspace too small: %zu < %zu bytes", workspace_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // thresholds and per-class parameters -> one packed block in the workspace, one copy
  const size_t o_hi = 0, o_lo = align256(V * C * 8), o_ns = 2 * o_lo, o_salt = o_ns + align256(C * 8);
  std::vector<char> blob(o_salt + C * 8, 0);
  std::memcpy(blob.data() + o_hi, high, V * C * 8);
  std::memcpy(blob.data() + o_lo, low, V * C * 8);
  std::memcpy(blob.data() + o_ns, n_smooth, C * 8);
  std::memcpy(blob.data() + o_salt, n_salt, C * 8);
  char* p = static_cast<char*>(d_workspace);
  if (hipMemcpyAsync(p, blob.data(), blob.size(), hipMemcpyHostToDevice, s) != hipSuccess) return SEDX_EHIP;
  CalibArgs a{d_x, n_clips, T, C, d_target, segment_frames, V,
              reinterpret_cast<const double*>(p + o_hi), reinterpret_cast<const double*>(p + o_lo),
              reinterpret_cast<const int64_t*>(p + o_ns), reinterpret_cast<const int64_t*>(p + o_salt), d_counts};
  launch_segment_counts(a, s);
  if (take_launch_error() != hipSuccess) return SEDX_EHIP;
  return hipGetLastError() == hipSuccess ? SEDX_OK : SEDX_EHIP;
}

}  // extern "C"
