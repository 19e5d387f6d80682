// Host side of windowed inference and the one-call forward on a gamma handle under AddressSanitizer + UBSan
// (make asan-gamma-windows): window_geometry / win_layout over both drivers and the vote merge, ragged_geometry /
// ragged_layout over chunk sizes, audio_layout over batches and clip lengths.  Every group's frame count is the
// gammatone one; the frontend's regions (gamma_layout's mag / db / mm for one forward's items) are 256-byte
// aligned, large enough for every forward that uses them, and disjoint from the model workspace, the stored
// outputs and the tables; a log-mel model's layouts carry no such region.  No GPU, no preload.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "host_check.h"

using namespace sedx;

static Model gamma_model(int type, int sr, int feature = SEDX_FEATURE_GAMMA) {
  sedx_config cfg{};
  cfg.model_type = type;
  cfg.feature_type = feature;
  cfg.sample_rate = sr, cfg.window_size = sr / 125 * 4, cfg.hop_size = sr / 100;   // 256 / 512 / 1024
  cfg.mel_bins = 64, cfg.fmin = sr / 640.f, cfg.fmax = sr * 0.4375f, cfg.classes_num = 25;
  Model m;
  if (!make_model(cfg, &m)) {
    std::printf("FAIL make_model(%d)\n", type);
    std::exit(1);
  }
  return m;
}

// gamma_layout's regions hold B items of L samples and fit in `bytes`
static void check_frontend(const Model& m, int64_t B, int64_t L, size_t bytes, const char* what) {
  GammaGeom gg;
  CHECK(gamma_geometry(m.cfg.sample_rate, m.cfg.window_size, m.cfg.hop_size, &gg), "%s: gamma_geometry", what);
  const GammaLayout g = gamma_layout(B, L, gg.nfft, gg.hop);
  CHECK(g.T == audio_T(m, L) && g.T >= 1 && g.T_fill >= g.T - 1 && g.T_fill <= g.T, "%s: T %lld", what, (long long)g.T);
  CHECK(g.mag_off % 256 == 0 && g.db_off % 256 == 0 && g.mm_off % 256 == 0 && g.total_bytes % 256 == 0, "%s: alignment", what);
  CHECK(g.db_off - g.mag_off >= (size_t)B * g.T * g.kp * 8 && g.mm_off - g.db_off >= (size_t)B * 64 * g.T * 8 &&
            g.total_bytes - g.mm_off >= (size_t)B * 16, "%s: a frontend region is too small", what);
  CHECK(g.total_bytes <= bytes, "%s: the frontend needs %zu of %zu bytes", what, g.total_bytes, bytes);
  CHECK(frontend_bytes(m, B, L) == g.total_bytes, "%s: frontend_bytes", what);
}

static void check_windows(const Model& m, const Model& logmel, int64_t L_clip, int64_t n_clips, const sedx_window_spec& sp) {
  WinGeom wg, wl_g;
  const bool avg = sp.vote == 0;
  const char* why = window_geometry(m, L_clip, &sp, avg, &wg);
  if (why) {
    CHECK(why[0] != 0, "an empty refusal");
    return;
  }
  const int C = m.cfg.classes_num;
  GammaGeom gg;
  gamma_geometry(m.cfg.sample_rate, m.cfg.window_size, m.cfg.hop_size, &gg);
  int nw = 0;
  for (const WinGroup& g : wg.groups) {
    CHECK(g.len >= gg.nfft && g.g.T == 1 + (g.len - gg.nfft) / gg.hop, "group of %lld samples: T %lld", (long long)g.len,
          (long long)g.g.T);
    char buf[96];
    CHECK(!shape_refusal(m, g.g.T, buf, sizeof(buf)), "an accepted group the model refuses");
    nw += g.nw;
  }
  CHECK(nw == wg.n_win, "groups cover the windows");
  const WinLayout l = win_layout(m, Tuning{}, n_clips, wg);
  std::vector<Span> spans;
  spans.push_back(Span{"model", 0, l.model_bytes / 4});
  for (size_t gi = 0; gi < wg.groups.size(); ++gi) {
    const WinGroup& g = wg.groups[gi];
    spans.push_back(Span{"framewise", l.fw_off[gi], (size_t)n_clips * g.nw * g.g.out_frames * C});
    spans.push_back(Span{"clipwise", l.clip_off[gi], (size_t)n_clips * g.nw * C});
    check_frontend(m, n_clips * g.nw, g.len, l.fe_bytes, "window group");
    ForwardPlan fp;
    CHECK(!plan_forward(m, Tuning{}, n_clips * g.nw, g.g.T, &fp) && fp.total_bytes <= l.model_bytes, "a group's plan");
  }
  spans.push_back(Span{"vote thresholds", l.vthr, (size_t)2 * C});
  CHECK(l.fe % 4 == 0 && l.fe_bytes > 0, "frontend region");
  spans.push_back(Span{"frontend", l.fe / 4, l.fe_bytes / 4});
  spans.push_back(Span{"tables", l.tables, l.table_bytes / 4});
  check_spans(spans, 0, l.total_bytes / 4, "win_layout");
  CHECK(l.total_bytes == l.tables * 4 + l.table_bytes, "the tables close the area");
  // the log-mel twin: no frontend region, the tables straight after the vote thresholds
  if (!window_geometry(logmel, L_clip, &sp, avg, &wl_g)) {
    const WinLayout ll = win_layout(logmel, Tuning{}, n_clips, wl_g);
    CHECK(ll.fe_bytes == 0 && ll.tables * 4 == ll.vthr * 4 + align256((size_t)2 * C * 4), "a log-mel layout changed");
  }
}

static void check_ragged(const Model& m, const std::vector<int64_t>& len, const sedx_window_spec& sp, int64_t per) {
  RaggedGeom rg;
  if (ragged_geometry(m, len.data(), (int64_t)len.size(), &sp, nullptr, &rg)) return;
  const int C = m.cfg.classes_num;
  CHECK(rg.g.T == audio_T(m, rg.full_len), "ragged item frames");
  const RaggedLayout l = ragged_layout(m, Tuning{}, rg, per);
  std::vector<Span> spans;
  spans.push_back(Span{"model", 0, l.model_bytes / 4});
  spans.push_back(Span{"framewise", l.fw, (size_t)l.items * rg.g.out_frames * C});
  spans.push_back(Span{"clipwise", l.clipwise, (size_t)l.chunk * C});
  spans.push_back(Span{"frontend", l.fe / 4, l.fe_bytes / 4});
  spans.push_back(Span{"tables", l.tables, l.table_bytes / 4});
  check_spans(spans, 0, l.total_bytes / 4, "ragged_layout");
  CHECK(l.fe % 4 == 0 && l.total_bytes == l.tables * 4 + l.table_bytes, "the tables close the area");
  // every forward of the call: full chunks, then the rest
  for (int64_t i0 = 0; i0 < l.items; i0 += l.chunk)
    check_frontend(m, std::min(l.chunk, l.items - i0), rg.full_len, l.fe_bytes, "ragged forward");
}

static void check_audio(const Model& m, int64_t B, int64_t L) {
  char buf[96];
  GammaGeom gg;
  gamma_geometry(m.cfg.sample_rate, m.cfg.window_size, m.cfg.hop_size, &gg);
  const char* why = audio_refusal(m, L, buf, sizeof(buf));
  CHECK((why != nullptr) == (L < gg.nfft), "audio_refusal at %lld samples", (long long)L);
  CHECK((audio_T(m, L) >= 1) == (L >= gg.nfft), "audio_T at %lld samples", (long long)L);
  if (why) {
    CHECK(frontend_bytes(m, B, L) == 0, "frontend_bytes of a refused clip");
    return;
  }
  const AudioLayout a = audio_layout(m, Tuning{}, B, L);
  ForwardPlan fp;
  plan_forward(m, Tuning{}, B, audio_T(m, L), &fp);
  CHECK(a.model_bytes == fp.total_bytes && a.fe % 256 == 0 && a.fe >= a.model_bytes && a.total_bytes == a.fe + a.fe_bytes,
        "audio_layout's order");
  check_frontend(m, B, L, a.fe_bytes, "audio forward");
}

static void check_refusals(const Model& m16) {
  WinGeom wg;
  sedx_window_spec sp{};
  sp.driver = SEDX_DRIVER_MAIN_STRONG, sp.sample_duration = 1, sp.overlap_value = 1.99, sp.audio_duration = 11.0;
  const char* why = window_geometry(m16, 176000, &sp, true, &wg);
  CHECK(why && !std::strcmp(why, "window 5 has 800 samples: shorter than the gammatone FFT"), "tail window: %s",
        why ? why : "accepted");
  sp.overlap_value = 1.98;   // 1600 samples: 4 frames
  why = window_geometry(m16, 176000, &sp, true, &wg);
  CHECK(why && std::strstr(why, "window 5: ") == why, "a 4-frame tail window: %s", why ? why : "accepted");
}

int main() {
  std::mt19937_64 rng(20240917);
  const int rates[3] = {8000, 16000, 32000};
  check_refusals(gamma_model(SEDX_MODEL_GRU_FRAMEATT, 16000));
  const double ovs[5] = {1.0, 0.5, 2.0, 0.37, 1.99};
  for (int it = 0; it < 240; ++it) {
    const int sr = rates[it % 3];
    const int type = it % 5 == 4 ? SEDX_MODEL_GRU_REG : SEDX_MODEL_GRU_FRAMEATT;
    const Model m = gamma_model(type, sr), lm = gamma_model(type, sr, SEDX_FEATURE_LOGMEL);
    const int sd = 1 + (int)(rng() % 6);
    sedx_window_spec sp{};
    sp.driver = rng() % 2 ? SEDX_DRIVER_PREDICT : SEDX_DRIVER_MAIN_STRONG;
    sp.overlap = (int)(rng() % 2), sp.sample_duration = sd;
    sp.vote = sp.driver == SEDX_DRIVER_MAIN_STRONG && rng() % 2;
    sp.overlap_value = ovs[rng() % 5];
    const int64_t L = (int64_t)(rng() % ((uint64_t)14 * sr)) + 1;
    // loop bounds a little off the decoded length, some running past the samples (main_strong: past 10 s)
    sp.audio_duration = rng() % 3 ? 0.0 : (double)L / sr + ((double)(rng() % 3000) - 1000.0) / 1000.0;
    check_windows(m, lm, L, 1 + (int64_t)(rng() % 5), sp);
    // ragged: the predict driver over clips of odd lengths, chunked
    sedx_window_spec rs{};
    rs.driver = SEDX_DRIVER_PREDICT, rs.overlap = (int)(rng() % 2), rs.sample_duration = sd, rs.overlap_value = ovs[rng() % 2];
    std::vector<int64_t> len(1 + rng() % 6);
    for (auto& v : len) v = (int64_t)sd * sr + (int64_t)(rng() % ((uint64_t)9 * sr));
    check_ragged(m, len, rs, (int64_t)(rng() % 4 == 0 ? 0 : 1 + rng() % 9));
    // the one-call forward: around the FFT length, and clips of seconds
    GammaGeom gg;
    gamma_geometry(m.cfg.sample_rate, m.cfg.window_size, m.cfg.hop_size, &gg);
    check_audio(m, 1 + (int64_t)(rng() % 40), gg.nfft - 2 + (int64_t)(rng() % 5));
    check_audio(m, 1 + (int64_t)(rng() % 40), gg.nfft + 7 * gg.hop + (int64_t)(rng() % ((uint64_t)10 * sr)));
  }
  return host_check::finish("gamma_windows_driver");
}
