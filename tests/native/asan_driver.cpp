// AddressSanitizer / UBSan driver for libsedx's host code that consumes
// untrusted input (built by `make -C sound-event-detection_amd asan`, run by
// tests/test_asan_cpu.py):
//  * sedx_wav_parse over a malformed-RIFF corpus: every truncation of valid
//    PCM16 / float32 / WAVE_FORMAT_EXTENSIBLE images, oversized and odd chunk
//    sizes, zero / huge channel counts, unknown formats, zero bits per sample,
//    and seeded random byte flips of the valid images;
//  * sedx_events (the quirk-exact vad of utils/vad.py) over random and edge
//    series: all-on, all-off, single frames at both ends, negative low
//    thresholds, capacity too small;
//  * the weight packing (csrc/weights.cpp): every packed layout read back the
//    way its kernel addresses it (the staging copy into LDS, then the lane's
//    fragment read), the split-bf16 bit patterns, the Winograd U values, and
//    prepare_weights whole for every model on a synthetic state_dict;
//  * the forward and window plans (csrc/plan.cpp): over models, precisions,
//    knobs, batch sizes and lengths, every workspace region aligned, disjoint
//    and large enough for what its launch writes by the contracts of
//    sedx_internal.h, and the kernel choices against literal tables;
//  * the Winograd conv launch plan (plan_conv_launch): over families, layers,
//    batch sizes, lengths, CU counts and knobs, every launch of a split batch
//    inside the kernels' 32-bit offsets, the grid and the item order within
//    what the item decode assumes, and every refusal an expected one;
//  * the fp32 GEMM launch plan (plan_linear_launch): over the sequence and head
//    GEMMs, row counts at every kernel switch and CU counts, the grid covering
//    the output exactly in the chosen kernel's tiles.
// Any memory error or undefined behaviour aborts the process; a failed check is
// printed and counted (host_check.h): non-zero exit either way.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/sedx.h"
#include "host_check.h"

namespace {

void put16(std::vector<uint8_t>& v, uint32_t x) {
  v.push_back(x & 0xff);
  v.push_back((x >> 8) & 0xff);
}
void put32(std::vector<uint8_t>& v, uint32_t x) {
  put16(v, x & 0xffff);
  put16(v, x >> 16);
}
void tag(std::vector<uint8_t>& v, const char* t) { v.insert(v.end(), t, t + 4); }

// RIFF image: fmt chunk (tag, channels, rate, bits; extensible adds the
// 24-byte extension), an odd-sized LIST chunk, then data of n_bytes.
std::vector<uint8_t> wav(uint32_t fmt_tag, uint32_t ch, uint32_t rate, uint32_t bits, uint32_t n_data,
                         bool extensible, uint32_t data_size_field) {
  std::vector<uint8_t> v;
  tag(v, "RIFF");
  put32(v, 0);
  tag(v, "WAVE");
  tag(v, "fmt ");
  put32(v, extensible ? 40 : 16);
  put16(v, extensible ? 0xFFFE : fmt_tag);
  put16(v, ch);
  put32(v, rate);
  put32(v, rate * ch * (bits / 8));
  put16(v, ch * (bits / 8));
  put16(v, bits);
  if (extensible) {
    put16(v, 22);
    put16(v, bits);
    put32(v, 0);
    put16(v, fmt_tag);
    for (int i = 0; i < 14; ++i) v.push_back(0);
  }
  tag(v, "LIST");
  put32(v, 3);
  v.push_back('a');
  v.push_back('b');
  v.push_back('c');
  v.push_back(0);   // pad byte of the odd chunk
  tag(v, "data");
  put32(v, data_size_field);
  for (uint32_t i = 0; i < n_data; ++i) v.push_back((uint8_t)(i * 37));
  const uint32_t riff = (uint32_t)v.size() - 8;
  std::memcpy(v.data() + 4, &riff, 4);
  return v;
}

int parse_all_prefixes(const std::vector<uint8_t>& img, int* ok) {
  int n = 0;
  for (size_t len = 0; len <= img.size(); ++len) {
    // exact-size heap copy so a read past `len` is caught
    std::vector<uint8_t> buf(img.begin(), img.begin() + len);
    sedx_wav_info info;
    const sedx_status st = sedx_wav_parse(len ? buf.data() : nullptr, len, &info);
    if (st == SEDX_OK) {
      ++*ok;
      if (info.data_offset + info.data_bytes > (int64_t)len || info.frames < 0) {
        std::fprintf(stderr, "parse accepted an inconsistent image (len %zu)\n", len);
        std::abort();
      }
    }
    ++n;
  }
  return n;
}

// ---- weight packing (csrc/weights.cpp) ---------------------------------------

using namespace sedx;

std::vector<double> random_wf(int Cin, int Cout, std::mt19937& rng) {
  std::normal_distribution<double> nd(0.0, 0.1);
  std::vector<double> wf((size_t)Cout * Cin * 9);
  for (auto& v : wf) v = nd(rng);
  return wf;
}
// every element of a pack was read exactly once: the pack holds nothing else
void all_once(const std::vector<uint8_t>& seen, const char* what) {
  for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "%s: element %zu read %d times", what, i, seen[i]);
}

// conv.hip (conv3x3_kernel): chunk c of channel block n0 is staged by 16-byte
// DMAs, LDS float L = 256 u + 4 lane <- wp[9 KC Cout c + 2 n0 + 2 Cout row + 4
// (lane % LPR)], row = L / (2 BN); the 32x32x2 MFMA's B fragment of a lane
// (khalf, n) at tap t is the float2 at t KC BN + (khalf BN + n) 2: (.x, .y) =
// k-steps 0, 1, and the A side pairs k-step ks with channel 2 ks + khalf
void check_exact(int Cin, int Cout, std::mt19937& rng) {
  const int KC = 4, BN = Cout % 128 == 0 ? 128 : Cout % 64 == 0 ? 64 : Cout;
  const std::vector<double> wf = random_wf(Cin, Cout, rng);
  std::vector<float> pk((size_t)Cin * 9 * Cout);
  pack_conv_exact(wf.data(), Cin, Cout, pk.data());
  std::vector<uint8_t> seen(pk.size(), 0);
  for (int o = 0; o < Cout; ++o)
    for (int i = 0; i < Cin; ++i)
      for (int t = 0; t < 9; ++t) {
        const int chunk = i / KC, ks = (i % KC) / 2, khalf = (i % KC) % 2, n0 = o / BN * BN, n = o % BN;
        const int L = t * KC * BN + (khalf * BN + n) * 2 + ks;
        const int row = L / (2 * BN), col = L % (2 * BN);
        const size_t g = (size_t)9 * KC * Cout * chunk + 2 * n0 + (size_t)row * 2 * Cout + col;
        CHECK(g < pk.size(), "exact %dx%d", Cin, Cout);
        CHECK(pk[g] == (float)wf[((size_t)o * Cin + i) * 9 + t], "exact %dx%d o %d i %d t %d", Cin, Cout, o, i, t);
        ++seen[g];
      }
  all_once(seen, "exact pack");
}

// round-to-nearest-even bf16 of a finite float, by the remainder
uint16_t bf16_rne(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  uint32_t hi = u >> 16;
  const uint32_t rem = u & 0xFFFFu;
  if (rem > 0x8000u || (rem == 0x8000u && (hi & 1u))) ++hi;
  return (uint16_t)hi;
}
float bf16_value(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// conv_x3.hip: stage (nb, chunk, ky) = 3 BN 4 uint4 copied as they lie from
// wp[((nb nchunks + chunk) 3 + ky) 3 BN 4 ..]; the fragment of lane (h, n) at
// tap (ky, kx) is uint4 kx BN 4 + n 4 + (h ^ s) (hi) and + ((2 + h) ^ s) (lo),
// s = (n >> 2) & 3; its 8 bf16 are input channels 16 chunk + 8 h + e.
// linear_x3.hip: chunk kc (32 k) = 2 BN 4 uint4 from Wp[nb (K / 16) BN 4 + kc
// 2 BN 4 ..]; the fragment of k-step ks is uint4 (ks BN + n) 4 + (h ^ s) / + ((2 + h) ^ s).
void check_x3(int N, int K, int taps, int BN, std::mt19937& rng) {
  std::normal_distribution<float> nd(0.f, 0.1f);
  std::vector<float> w((size_t)N * K * taps);
  for (auto& v : w) v = nd(rng);
  // edges: zero, bf16-exact (lo == 0), exact ties (to even: down, then up), a negative tie
  const float edges[] = {0.f, -0.f, 1.5f, from_bits(0x3F808000u), from_bits(0x3F818000u), from_bits(0xBF808000u),
                         from_bits(0x3F80FFFFu)};
  for (size_t e = 0; e < sizeof(edges) / sizeof(edges[0]); ++e) {
    w[e] = edges[e];                          // first output channel
    w[w.size() - 1 - 13 * e] = edges[e];      // last ones: the other swizzles and halves
    w[(w.size() / 2 + 29 * e) % w.size()] = edges[e];
  }
  CHECK(bf16_rne(edges[3]) == 0x3F80 && bf16_rne(edges[4]) == 0x3F82 && bf16_rne(edges[2]) == 0x3FC0, "tie rule");
  const std::vector<uint16_t> px = pack_x3(w.data(), N, K, taps, BN);
  CHECK(px.size() == w.size() * 2, "x3 size");
  std::vector<uint8_t> seen(px.size(), 0);
  int sw_seen = 0;
  for (int o = 0; o < N; ++o)
    for (int i = 0; i < K; ++i)
      for (int t = 0; t < taps; ++t) {
        const int nb = o / BN, n = o % BN, s = (n >> 2) & 3, h = (i % 16) / 8, e = i % 8;
        size_t u4;
        if (taps == 9) {
          const int nchunks = K / 16, chunk = i / 16, ky = t / 3, kx = t % 3;
          u4 = (((size_t)nb * nchunks + chunk) * 3 + ky) * (3 * BN * 4) + (size_t)kx * BN * 4 + n * 4;
        } else {
          const int kc = i / 32, ks = (i % 32) / 16;
          u4 = (size_t)nb * (K / 16) * BN * 4 + (size_t)kc * (2 * BN * 4) + (size_t)(ks * BN + n) * 4;
        }
        const size_t ihi = 8 * (u4 + (h ^ s)) + e, ilo = 8 * (u4 + ((2 + h) ^ s)) + e;
        CHECK(ihi < px.size() && ilo < px.size(), "x3 index");
        const float x = w[((size_t)o * K + i) * taps + t];
        const uint16_t hi = bf16_rne(x), lo = bf16_rne(x - bf16_value(hi));
        CHECK(px[ihi] == hi && px[ilo] == lo, "x3 N %d K %d taps %d o %d i %d t %d: %04x %04x vs %04x %04x", N, K,
              taps, o, i, t, px[ihi], px[ilo], hi, lo);
        ++seen[ihi];
        ++seen[ilo];
        sw_seen |= 1 << s;
      }
  CHECK(sw_seen == 15, "x3: all four swizzles");
  all_once(seen, "x3 pack");
}

// (G g G^T)[a][c] in float64, rounded once to fp32: g [3][3] row-major, G [n][3]
void ggt(const double* g, const double (*G)[3], int n, float* out) {
  double tmp[6][3];
  for (int a = 0; a < n; ++a)
    for (int y = 0; y < 3; ++y) tmp[a][y] = G[a][0] * g[0 * 3 + y] + G[a][1] * g[1 * 3 + y] + G[a][2] * g[2 * 3 + y];
  for (int a = 0; a < n; ++a)
    for (int c = 0; c < n; ++c) out[a * n + c] = (float)(tmp[a][0] * G[c][0] + tmp[a][1] * G[c][1] + tmp[a][2] * G[c][2]);
}
const double G22[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
const double G43[6][3] = {{1.0 / 4, 0, 0},          {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                          {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6},  {0, 0, 1}};

// conv_wino.hip: chunk c of channel group n0 (NCH = 32 or 64 channels) is
// staged like the exact slab, LDS float L <- U[64 Cout c + 2 n0 + 2 Cout row +
// col], row = L / (2 NCH); the fragment of lane (khalf, n) at position p is
// the float2 at 4 NCH p + 2 NCH khalf + 2 n, (.x, .y) = k-steps 0, 1 = input
// channels 2 khalf, 2 khalf + 1 of the chunk (the halo's float2 of that lane)
void check_wino(int Cin, int Cout, int NCH, std::mt19937& rng) {
  const std::vector<double> wf = random_wf(Cin, Cout, rng);
  std::vector<float> U((size_t)Cin * Cout * 16);
  pack_conv_wino(wf.data(), Cin, Cout, U.data());
  std::vector<uint8_t> seen(U.size(), 0);
  for (int o = 0; o < Cout; ++o)
    for (int i = 0; i < Cin; ++i) {
      float want[16];
      ggt(&wf[((size_t)o * Cin + i) * 9], G22, 4, want);
      const int chunk = i / 4, khalf = (i % 4) / 2, ks = i % 2, n0 = o / NCH * NCH, n = o % NCH;
      for (int p = 0; p < 16; ++p) {
        const int L = 4 * NCH * p + 2 * NCH * khalf + 2 * n + ks;
        const int row = L / (2 * NCH), col = L % (2 * NCH);
        const size_t g = (size_t)64 * Cout * chunk + 2 * n0 + (size_t)row * 2 * Cout + col;
        CHECK(g < U.size(), "wino index");
        CHECK(U[g] == want[p], "wino %dx%d o %d i %d p %d", Cin, Cout, o, i, p);
        ++seen[g];
      }
    }
  all_once(seen, "F(2x2) pack");
}

// conv_wino43.hip: the slab of (64-channel group g, chunk c) = 36 x 4 x 64
// floats copied as they lie from U[(g nch + c) 9216 ..]; lane l = 16 k + m
// reads position p as the 4 floats at 256 p + 4 l: output channels 64 g + 16 nt
// + m, nt = 0..3, input channel 4 c + k.  The 16-channel items read the second
// pack, at Cin Cout 36 floats: slab (g16, c) at (g16 nch + c) 2304, the lane's
// float at 64 p + l.
void check_wino43(int Cin, int Cout, std::mt19937& rng) {
  const std::vector<double> wf = random_wf(Cin, Cout, rng);
  std::vector<float> U((size_t)2 * Cin * Cout * 36);
  pack_conv_wino43(wf.data(), Cin, Cout, U.data());
  std::vector<uint8_t> seen(U.size(), 0);
  const int nch = Cin / 4;
  int nt_seen = 0;
  for (int o = 0; o < Cout; ++o)
    for (int i = 0; i < Cin; ++i) {
      float want[36];
      ggt(&wf[((size_t)o * Cin + i) * 9], G43, 6, want);
      const int c = i / 4, k = i % 4, m = o % 16, lane = 16 * k + m, nt = o % 64 / 16;
      for (int p = 0; p < 36; ++p) {
        const size_t g4 = ((size_t)(o / 64) * nch + c) * 9216 + 256 * p + 4 * lane + nt;
        const size_t g1 = (size_t)Cin * Cout * 36 + ((size_t)(o / 16) * nch + c) * 2304 + 64 * p + lane;
        CHECK(g4 < (size_t)Cin * Cout * 36 && g1 < U.size(), "wino43 index");
        CHECK(U[g4] == want[p] && U[g1] == want[p], "wino43 %dx%d o %d i %d p %d", Cin, Cout, o, i, p);
        ++seen[g4];
        ++seen[g1];
      }
      nt_seen |= 1 << nt;
    }
  CHECK(nt_seen == 15, "wino43: nt 0..3");
  all_once(seen, "F(4x4) packs");
}

// a synthetic state_dict of the model's expected shapes: random tensors
// (positive variances), a Hann-window DFT for the STFT, a triangular mel
// matrix.  only: a key prefix to keep (nullptr: every key)
Params synth_params(const Model& m, uint32_t seed, const char* only = nullptr, const char* only2 = nullptr) {
  Params P;
  std::mt19937 rng(seed);
  std::normal_distribution<float> nd(0.f, 0.1f);
  for (const auto& kv : expected_params(m)) {
    const std::string& key = kv.first;
    if (only && key.rfind(only, 0) != 0 && key.rfind(only2, 0) != 0) continue;
    Tensor t;
    t.shape = kv.second;
    size_t n = 1;
    for (int64_t d : t.shape) n *= (size_t)d;
    t.data.resize(n);
    const bool var = key.size() > 11 && key.compare(key.size() - 11, 11, "running_var") == 0;
    for (auto& v : t.data) v = var ? std::fabs(nd(rng)) + 0.5f : nd(rng);
    P[key] = std::move(t);
  }
  if (only) return P;
  const int N = m.cfg.window_size, K = N / 2 + 1;
  auto& wr = P.at("spectrogram_extractor.stft.conv_real.weight").data;
  auto& wi = P.at("spectrogram_extractor.stft.conv_imag.weight").data;
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) {
      const double win = 0.5 - 0.5 * std::cos(2.0 * M_PI * n / N), ang = 2.0 * M_PI * ((int64_t)k * n % N) / N;
      wr[(size_t)k * N + n] = (float)(std::cos(ang) * win);
      wi[(size_t)k * N + n] = (float)(-std::sin(ang) * win);
    }
  auto& mel = P.at("logmel_extractor.melW").data;   // [K][64]: band m a triangle around bin (m + 1) (K - 1) / 65
  const double step = (K - 1) / 65.0;
  for (int k = 0; k < K; ++k)
    for (int b = 0; b < 64; ++b) {
      const double v = 1.0 - std::fabs(k - (b + 1) * step) / step;
      mel[(size_t)k * 64 + b] = v > 0 ? (float)v : 0.f;
    }
  return P;
}

struct PtrWant {
  const char* name;
  const void* p;
  bool want;
};
// every pointer of the table, with whether this model's forward reads it
std::vector<PtrWant> pointer_table(const Model& m, const DevWeights& W) {
  const bool gru = m.seq == SEQ_GRU, mha = m.seq == SEQ_MHA, cf = m.seq == SEQ_CONFORMER;
  const bool gam = m.cfg.feature_type == SEDX_FEATURE_GAMMA;
  std::vector<PtrWant> t = {
      {"twiddle", W.twiddle, true},     {"window", W.window, true},       {"mel_w", W.mel_w, true},
      {"mel_tab", W.mel_tab, true},     {"mel_mt", W.mel_mt, m.cfg.window_size == 512},
      {"mel_off", W.mel_off, true},     {"mel_lo", W.mel_lo, true},       {"bn0_scale", W.bn0_scale, true},
      {"bn0_mean", W.bn0_mean, true},   {"bn0_bias", W.bn0_bias, true},   {"c1_w", W.c1_w, true},
      {"c1_wt", W.c1_wt, true},         {"c1_b", W.c1_b, true},           {"zero", W.zero, true},
      {"trash", W.trash, true},         {"w_ih", W.w_ih, gru},            {"b_ih", W.b_ih, gru},
      {"whhT", W.whhT, gru},            {"whh", W.whh, gru},              {"bhh", W.bhh, gru},
      {"wqkv", W.wqkv, mha},            {"bqkv", W.bqkv, mha},            {"wfc", W.wfc, mha},
      {"bfc", W.bfc, mha},              {"wac", W.wac, true},             {"bac", W.bac, true},
      {"cf_in_w", W.cf_in_w, cf},       {"cf_in_b", W.cf_in_b, cf},       {"cf_in_g", W.cf_in_g, cf},
      {"cf_in_be", W.cf_in_be, cf},     {"cf_pe", W.cf_pe, cf},           {"cf_inv_freq", W.cf_inv_freq, cf},
      {"w_ih_x3", W.w_ih_x3, gru},      {"wqkv_x3", W.wqkv_x3, mha},      {"wfc_x3", W.wfc_x3, mha},
      {"wac_x3", W.wac_x3, !cf},        {"g_twiddle", W.g_twiddle, gam},  {"g_window", W.g_window, gam},
      {"g_weightsT", W.g_weightsT, gam},
  };
  for (int i = 0; i < 8; ++i) {
    t.push_back({"wp", W.wp[i], i > 0});
    t.push_back({"cb", W.cb[i], i > 0});
    t.push_back({"wx3", W.wx3[i], i > 0});
    t.push_back({"wu", W.wu[i], i > 0});
    t.push_back({"wu43", W.wu43[i], i > 0});
  }
  for (const CfBlockWeights& c : W.cf) {
    for (int f = 0; f < 2; ++f)
      for (const float* p : {c.ffn_g[f], c.ffn_be[f], c.ffn_w1[f], c.ffn_b1[f], c.ffn_w2[f], c.ffn_b2[f]})
        t.push_back({"cf.ffn", p, cf});
    for (const float* p : {c.att_g, c.att_be, c.wqkv, c.wo, c.rnet, c.rwb, c.rrb, c.cv_g, c.cv_be, c.pw1_w, c.pw1_b,
                           c.dw_wt, c.dw_b, c.pw2_w, c.pw2_b, c.norm_g, c.norm_be})
      t.push_back({"cf", p, cf});
  }
  return t;
}
// the table above names every pointer member: a member added to DevWeights
// without a row here changes this size
static_assert(sizeof(DevWeights) == sizeof(void*) * (39 + 5 * 8 + CF_BLOCKS * 29) + 14 * sizeof(int32_t),
              "pointer_table lists every DevWeights pointer");

// rows of the head projection against the state_dict: att row c at c, cla row
// c at C + c (fc: row c at c), zeros after
void check_head_rows(const Model& m, const Params& P, const float* wac, const float* bac) {
  const int C = m.cfg.classes_num;
  const bool att = m.head == HEAD_ATT;
  for (int r = 0; r < m.nac; ++r) {
    const Tensor* w = nullptr;
    const Tensor* b = nullptr;
    int c = r;
    if (att && r < 2 * C) {
      w = &P.at(r < C ? "att_block.att.weight" : "att_block.cla.weight");
      b = &P.at(r < C ? "att_block.att.bias" : "att_block.cla.bias");
      c = r < C ? r : r - C;
    } else if (!att && r < C) {
      w = &P.at("fc.weight");
      b = &P.at("fc.bias");
    }
    CHECK(bac[r] == (b ? b->data[c] : 0.f), "head bias row %d", r);
    for (int j = 0; j < m.hw; ++j)
      CHECK(wac[(size_t)r * m.hw + j] == (w ? w->data[(size_t)c * m.hw + j] : 0.f), "head row %d col %d", r, j);
  }
}

// prepare_weights on a whole synthetic state_dict
void check_prepare(int model_type, int window, int feature, int classes = 25) {
  const Model m = model_of(model_type, classes, window, feature);
  const Params P = synth_params(m, 100 + model_type);
  DevWeights W;
  WeightBlob blob;
  GammaGeom gg;
  std::string err;
  const sedx_status st = prepare_weights(m, P, &W, &blob, &gg, &err);
  CHECK(st == SEDX_OK, "model %d window %d: %s", model_type, window, err.c_str());
  // regions: 256-byte aligned, disjoint, inside the image, one per pointer
  size_t end = 0;
  for (const auto& r : blob.regions) {
    CHECK(r.off % 256 == 0 && r.off >= end && r.bytes > 0 && r.off + r.bytes <= blob.image.size(), "region at %zu", r.off);
    end = r.off + r.bytes;
  }
  for (const PtrWant& e : pointer_table(m, W)) CHECK(e.p == nullptr, "%s set before bind", e.name);
  blob.bind(blob.image.data());   // the image stands in for the device allocation
  size_t set = 0;
  for (const PtrWant& e : pointer_table(m, W)) {
    CHECK((e.p != nullptr) == e.want, "model %d window %d: pointer %s", model_type, window, e.name);
    set += e.p != nullptr;
  }
  CHECK(set == blob.regions.size(), "%zu pointers, %zu regions", set, blob.regions.size());
  for (const auto& r : blob.regions) CHECK(*r.dst == blob.image.data() + r.off, "bind");
  CHECK((W.mt_floats != 0) == (window == 512), "mt_floats %d at window %d", W.mt_floats, window);
  CHECK((gg.nfft != 0) == (feature == SEDX_FEATURE_GAMMA), "gamma geometry");
  // through the table, as block 1's conv2 reads it (check_exact's addressing
  // at BN = 64): the BN-folded weight and bias
  const auto& wt = P.at("conv_block1.conv2.weight").data;
  for (int o = 0; o < 64; ++o) {
    const double sc = (double)P.at("conv_block1.bn2.weight").data[o] /
                      std::sqrt((double)P.at("conv_block1.bn2.running_var").data[o] + 1e-5);
    CHECK(W.cb[1][o] == (float)((double)P.at("conv_block1.bn2.bias").data[o] -
                                (double)P.at("conv_block1.bn2.running_mean").data[o] * sc), "bias %d", o);
    for (int i = 0; i < 64; ++i)
      for (int t = 0; t < 9; ++t) {
        const int L = t * 4 * 64 + ((i % 2) * 64 + o) * 2 + (i % 4) / 2;
        CHECK(W.wp[1][(size_t)9 * 4 * 64 * (i / 4) + L] == (float)(wt[((size_t)o * 64 + i) * 9 + t] * sc), "wp[1]");
      }
  }
  // the head in the image, and its x3 pack as linear_x3.hip reads it at N =
  // nac, BN = 64 (check_x3's addressing)
  check_head_rows(m, P, W.wac, W.bac);
  if (W.wac_x3) {
    const uint16_t* px = static_cast<const uint16_t*>(W.wac_x3);
    for (int o = 0; o < m.nac; ++o)
      for (int i = 0; i < 512; ++i) {
        const int nb = o / 64, n = o % 64, s = (n >> 2) & 3, h = (i % 16) / 8, e = i % 8, kc = i / 32, ks = (i % 32) / 16;
        const size_t u4 = (size_t)nb * 32 * 64 * 4 + (size_t)kc * (2 * 64 * 4) + (size_t)(ks * 64 + n) * 4;
        const float x = W.wac[(size_t)o * 512 + i];
        const uint16_t hi = bf16_rne(x), lo = bf16_rne(x - bf16_value(hi));
        CHECK(px[8 * (u4 + (h ^ s)) + e] == hi && px[8 * (u4 + ((2 + h) ^ s)) + e] == lo, "wac_x3 row %d col %d", o, i);
      }
  }
}

// head rows over the class counts at which nac steps (one trunk: heads only)
void check_heads() {
  for (int model_type : {SEDX_MODEL_CNN_FRAMEATT, SEDX_MODEL_CNN_FRAMEAVG, SEDX_MODEL_CONFORMER_FRAMEATT})
    for (int C : {1, 32, 33, 64, 65, 256}) {
      const Model m = model_of(model_type, C, 512, SEDX_FEATURE_LOGMEL);
      const bool att = m.head == HEAD_ATT;
      const int rows = att ? 2 * C : C;
      CHECK(m.nac == (rows + 63) / 64 * 64 && m.nac >= rows && m.nac % 64 == 0, "nac %d for %d rows", m.nac, rows);
      if (att) CHECK(m.nac == (C <= 32 ? 64 : C <= 64 ? 128 : C <= 96 ? 192 : 512), "AttBlock nac %d at C %d", m.nac, C);
      else CHECK(m.nac == (C <= 64 ? 64 : C <= 128 ? 128 : 256), "fc nac %d at C %d", m.nac, C);
      const Params P = synth_params(m, 7 * C, "att_block.", "fc.");
      std::vector<float> wac, bac;
      pack_head(m, P, &wac, &bac);
      CHECK(wac.size() == (size_t)m.nac * m.hw && bac.size() == (size_t)m.nac, "head size");
      check_head_rows(m, P, wac.data(), bac.data());
    }
}

void check_errors() {
  const Model m = model_of(SEDX_MODEL_GRU_FRAMEATT, 25, 512, SEDX_FEATURE_LOGMEL);
  Params P = synth_params(m, 5);
  DevWeights W;
  WeightBlob blob;
  GammaGeom gg;
  std::string err;
  Params Q = P;
  Q.erase("gru.bias_hh_l0_reverse");
  CHECK(prepare_weights(m, Q, &W, &blob, &gg, &err) == SEDX_EKEY, "missing key status");
  CHECK(err == "missing key in state_dict: gru.bias_hh_l0_reverse", "missing key message: %s", err.c_str());
  P.at("spectrogram_extractor.stft.conv_imag.weight").data[2 * 512 + 7] += 1e-3f;
  CHECK(prepare_weights(m, P, &W, &blob, &gg, &err) == SEDX_EINVAL, "perturbed STFT status");
  CHECK(err.rfind("STFT conv weights are not a windowed DFT (max err ", 0) == 0 &&
            err.find("the FFT frontend cannot reproduce them") != std::string::npos, "STFT message: %s", err.c_str());
}

int check_weights() {
  std::mt19937 rng(4321);
  int n = 0;
  check_exact(4, 2, rng), ++n;
  check_exact(8, 128, rng), ++n;
  check_exact(64, 64, rng), ++n;
  check_x3(64, 16, 1, 64, rng), ++n;
  check_x3(128, 32, 1, 128, rng), ++n;
  check_x3(64, 16, 9, 64, rng), ++n;
  check_x3(256, 32, 9, 128, rng), ++n;
  check_wino(4, 32, 32, rng), ++n;
  check_wino(8, 64, 32, rng), ++n;
  check_wino(8, 64, 64, rng), ++n;
  check_wino43(8, 64, rng), ++n;
  check_wino43(16, 128, rng), ++n;
  for (int model_type = 0; model_type <= 8; ++model_type) check_prepare(model_type, 512, SEDX_FEATURE_LOGMEL), ++n;
  check_prepare(SEDX_MODEL_GRU_FRAMEATT, 512, SEDX_FEATURE_GAMMA), ++n;
  check_prepare(SEDX_MODEL_CNN_FRAMEAVG, 256, SEDX_FEATURE_LOGMEL), ++n;
  check_prepare(SEDX_MODEL_CNN_FRAMEAVG, 1024, SEDX_FEATURE_LOGMEL), ++n;
  // nac 128 through the whole path (the head's x3 pack at two column blocks)
  check_prepare(SEDX_MODEL_CNN_FRAMEATT, 512, SEDX_FEATURE_LOGMEL, 33), ++n;
  check_prepare(SEDX_MODEL_CNN_FRAMEAVG, 512, SEDX_FEATURE_LOGMEL, 65), ++n;
  check_heads(), ++n;
  check_errors(), n += 2;
  return n;
}

// ---- forward and window plans (csrc/plan.cpp) ---------------------------------
// the conv launches after block 1's first, by trunk: the layer's T is T >> pools; its F, channels and epilogue
struct LayerRow { int pools, F, cin, cout, epi; };
const LayerRow ROWS9[7] = {{0, 64, 64, 64, EPI_POOL2},    {1, 32, 64, 128, EPI_STORE},  {1, 32, 128, 128, EPI_POOL2},
                           {2, 16, 128, 256, EPI_STORE}, {2, 16, 256, 256, EPI_POOL2}, {3, 8, 256, 512, EPI_STORE},
                           {3, 8, 512, 512, EPI_FMEAN}};
const LayerRow ROWS14[11] = {{0, 64, 64, 64, EPI_POOL2},    {1, 32, 64, 128, EPI_STORE},   {1, 32, 128, 128, EPI_POOL2},
                             {2, 16, 128, 256, EPI_STORE}, {2, 16, 256, 256, EPI_POOL2},  {3, 8, 256, 512, EPI_STORE},
                             {3, 8, 512, 512, EPI_POOL2},  {4, 4, 512, 1024, EPI_STORE},  {4, 4, 1024, 1024, EPI_POOL2},
                             {5, 2, 1024, 2048, EPI_STORE}, {5, 2, 2048, 2048, EPI_FMEAN}};
const LayerRow ROWSVGG[5] = {{1, 32, 64, 128, EPI_MAXPOOL2},   {2, 16, 128, 256, EPI_STORE}, {2, 16, 256, 256, EPI_MAXPOOL2},
                             {3, 8, 256, 512, EPI_STORE},     {3, 8, 512, 512, EPI_MAXPOOL2_FMEAN}};

// one plan of any model against the launch contracts of sedx_internal.h: the extents below are what the kernels
// write, restated here, not what plan.cpp reserved.  Top-level regions aligned, disjoint and inside the total; the
// conv chain by the trunk's layer table, each launch reading what the previous one wrote, in the other buffer.
// Returns plan_forward's reason.
const char* check_plan_regions(const Model& m, const Tuning& t, int64_t B, int64_t T, ForwardPlan* plan) {
  ForwardPlan& p = *plan;
  const char* why = plan_forward(m, t, B, T, &p);
  const bool deep = m.depth == 14;
  const LayerRow* rows = m.vgg ? ROWSVGG : deep ? ROWS14 : ROWS9;
  const int nlayers = m.vgg ? 5 : deep ? 11 : 7, pools = m.vgg ? 4 : deep ? 5 : 3;
  const int64_t Ts = T >> pools;
  CHECK(p.g.T == T && p.g.T1 == T / 2 && p.g.T2 == T / 4 && p.g.T3 == T / 8 && p.g.Ts == Ts && p.B == B && p.M == (int)(B * Ts),
        "geometry of model %d at T %lld", m.cfg.model_type, (long long)T);
  CHECK(p.nlayers == nlayers && p.first_deep == (m.vgg ? 5 : deep ? 6 : 7), "model %d: layer list", m.cfg.model_type);
  const size_t total = p.total_bytes / 4, uB = (size_t)B;
  CHECK(p.total_bytes % 256 == 0, "total");
  check_spans({span("x0", p.x0), span("A", p.A), span("P", p.P), span("sched", p.sched)}, 0, total, "workspace");
  CHECK(p.x0.floats >= uB * T * 64, "x0");                                   // launch_logmel / launch_features_bn0
  CHECK(p.sched.floats >= 7 * 256, "sched");                                 // 7 launches x CONV_SCHED_INTS
  for (int i = 0; i < nlayers; ++i) {
    const ConvLayer& c = p.layers[i];
    const LayerRow& r = rows[i];
    const int64_t Tl = T >> r.pools;
    CHECK(c.T == Tl && c.F == r.F && c.cin == r.cin && c.cout == r.cout && c.epi == r.epi, "model %d layer %d", m.cfg.model_type, i);
    const Region& out = i % 2 ? p.A : p.P;
    CHECK(c.out == out.off && c.in == (i % 2 ? p.P.off : i == 0 && p.block1 == B1_F23_FUSED ? p.x0.off : p.A.off),
          "layer %d buffers", i);
    const bool pool = r.epi == EPI_POOL2 || r.epi == EPI_MAXPOOL2, mean = r.epi == EPI_FMEAN || r.epi == EPI_MAXPOOL2_FMEAN;
    const int64_t To = pool || r.epi == EPI_MAXPOOL2_FMEAN ? Tl / 2 : Tl, Fo = mean ? 1 : pool ? r.F / 2 : r.F;
    CHECK(c.To == To && c.Fo == Fo, "layer %d output %d x %d", i, c.To, c.Fo);
    const size_t ext = uB * To * Fo * r.cout;   // [B][To][Fo][Cout]; the frequency means: [B][To][Cout]
    CHECK(ext <= out.floats, "layer %d writes %zu floats into %zu", i, ext, out.floats);
    if (i > 0) {
      const ConvLayer& q = p.layers[i - 1];
      CHECK(c.in == q.out && c.T == q.To && c.F == q.Fo && c.cin == q.cout, "layer %d does not read layer %d", i, i - 1);
      CHECK(uB * c.T * c.F * c.cin <= (i % 2 ? p.P : p.A).floats, "layer %d reads outside its buffer", i);
    }
    if (i >= p.first_deep) CHECK(c.cin % DEEP_CK == 0 && c.cout % DEEP_BN == 0, "deep layer %d", i);   // conv_deep.hip's tiles
  }
  // the last launch writes the sequence input [B][Ts][sw] into P; the logits live in A
  const ConvLayer& last = p.layers[nlayers - 1];
  CHECK(last.To == Ts && last.Fo == 1 && last.cout == m.sw && last.out == p.P.off, "the sequence input is not P");
  CHECK(inside(p.LG, p.A) && p.LG.floats >= uB * Ts * m.nac, "logits");
  return why;
}

// a 9-layer plan: the refusals, the kernel choices against literal tables and the head / encoder scratch
void check_plan(const Model& m, const Tuning& t, int64_t B, int64_t T) {
  ForwardPlan p;
  const char* why = check_plan_regions(m, t, B, T, &p);
  const int64_t T3 = T / 8;
  const bool cf = m.seq == SEQ_CONFORMER;
  const char* want_why = T3 < 1 ? "input too short" : cf && T3 > 5000 ? "the Conformer encoder holds 5000" : B * T > INT32_MAX / 64 ? "batch too large" : nullptr;
  CHECK((why == nullptr) == (want_why == nullptr), "B %lld T %lld: %s", (long long)B, (long long)T, why ? why : "accepted");
  if (why && want_why) CHECK(std::strstr(why, want_why) != nullptr, "B %lld T %lld: reason '%s'", (long long)B, (long long)T, why);
  // the block-1 form, the layout flag and the family for (precision, SEDX_TUNE_WINO_BLOCK1, SEDX_TUNE_WINO_F43)
  static const Block1Form wino_form[3][3] = {{B1_PAD_EXACT, B1_PAD_EXACT, B1_PAD_EXACT},
                                            {B1_CONV1_F23, B1_CONV1_F23, B1_CONV1_F43},
                                            {B1_F23_FUSED, B1_F23_FUSED, B1_CONV1C4_F43}};
  static const bool wino_c4[3][3] = {{false, false, false}, {false, false, false}, {false, true, true}};
  static const ConvFamily wino_family[3] = {CONV_WINO, CONV_WINO43, CONV_WINO43};
  const bool wino = t.precision == SEDX_PRECISION_WINOGRAD, x3 = t.precision == SEDX_PRECISION_X3;
  const Block1Form form = wino ? wino_form[t.wino_block1][t.wino_f43] : x3 ? B1_PAD_X3 : B1_PAD_EXACT;
  const ConvFamily family = wino ? wino_family[t.wino_f43] : x3 ? CONV_X3 : CONV_EXACT;
  CHECK(p.block1 == form && p.c4 == (wino && wino_c4[t.wino_block1][t.wino_f43]) && p.family == family,
        "precision %d block1 %d f43 %d: form %d c4 %d family %d", t.precision, t.wino_block1, t.wino_f43, p.block1, p.c4, p.family);
  CHECK(p.claims == (x3 || (family == CONV_WINO43 && B >= 8)), "claims at B %lld", (long long)B);
  const size_t uB = (size_t)B, M = uB * T3;
  const size_t first = form == B1_F23_FUSED ? 0 : form == B1_PAD_EXACT || form == B1_PAD_X3 ? uB * (T + 2) * 66 : uB * T * 64 * 64;
  CHECK(first <= p.A.floats, "block 1's first launch: %zu floats into A of %zu", first, p.A.floats);
  // after the conv stack, inside A (P still holds the stage-8 output)
  const size_t a0 = p.A.off, a1 = p.A.off + p.A.floats;
  if (cf) {
    check_spans({span("X", p.X), span("Xn", p.Xn), span("Hb", p.Hb), span("AV", p.AV), span("Rr", p.Rr), span("RK", p.RK),
                 span("LG", p.LG)}, a0, a1, "Conformer scratch");
    CHECK(p.X.floats >= M * 144 && p.Xn.floats >= M * 144 && p.AV.floats >= M * 144, "encoder activations");
    CHECK(p.Hb.floats >= M * 576, "hidden: the widest of ffn 576, qkv 432, pw1 288");
    CHECK(p.Rr.floats >= (size_t)3 * T3 * 144 && p.RK.floats >= (size_t)3 * T3 * 144, "r, r_k");
  } else {
    check_spans({span("G", p.G), span("Hs", p.Hs), span("O", p.O), span("LG", p.LG), span("gru", p.gru)}, a0, a1, "head scratch");
    CHECK(p.G.floats >= M * 1536 && p.Hs.floats >= M * 512 && p.O.floats >= M * 512, "G, H, O");
    // gru.hip: the sync block rounded up to 256 B (10,056 -> 10,240), then 8 x 2 x 32 x 256 floats
    CHECK(p.gru.floats * 4 >= 10240 + (size_t)8 * 2 * 32 * 256 * 4, "recurrence scratch");
  }
  // launch_gru_coop's arguments
  static const int variant[8] = {2, -1, 0, 1, 3, 3, 4, 5};   // COOP, SIMPLE, TAG16, TAG8, COOP16, AUTO, KSPLIT, PAIR
  static const bool fast[4] = {true, false, false, true};    // AUTO, GLOBAL, SPREAD, LOCAL
  const bool spread = t.gru_handoff == SEDX_GRU_HANDOFF_SPREAD || (t.gru_handoff == SEDX_GRU_HANDOFF_AUTO && t.pipelined);
  CHECK(p.gru_variant == variant[t.gru_kernel] && p.gru_fast == fast[t.gru_handoff] && p.gru_spread == spread,
        "gru kernel %d handoff %d pipelined %d: variant %d fast %d spread %d", t.gru_kernel, t.gru_handoff, t.pipelined,
        p.gru_variant, p.gru_fast, p.gru_spread);
}

// the windowed drivers' device area for tests/test_host_cpu.py's DRIVER_CASES
// (false: utilities.merge itself raises on the spec's windows, as numpy does)
bool check_window_plan(const Model& m, const Tuning& t, int driver, bool overlap, int sd, double ov, double secs, int64_t n_clips) {
  sedx_window_spec spec{};
  spec.driver = driver;
  spec.overlap = overlap;
  spec.sample_duration = sd;
  spec.overlap_value = ov;
  WinGeom wg;
  const char* why = window_geometry(m, (int64_t)std::llround(secs * 16000), &spec, true, &wg);
  if (why && std::strncmp(why, "merge: operands could not be broadcast", 38) == 0) return false;
  CHECK(!why, "window spec sd %d ov %g %g s: %s", sd, ov, secs, why);
  const WinLayout l = win_layout(m, t, n_clips, wg);
  CHECK(l.fw_off.size() == wg.groups.size() && l.clip_off.size() == wg.groups.size() && !wg.groups.empty(), "groups");
  const size_t C = m.cfg.classes_num;
  std::vector<Span> area;
  int n_win = 0;
  for (size_t g = 0; g < wg.groups.size(); ++g) {
    const size_t items = (size_t)n_clips * wg.groups[g].nw;
    ForwardPlan p;
    CHECK(!plan_forward(m, t, (int64_t)items, wg.groups[g].g.T, &p) && p.total_bytes <= l.model_bytes, "group %zu's plan", g);
    area.push_back(Span{"framewise", l.fw_off[g], items * (size_t)wg.groups[g].g.out_frames * C});   // att / fc head
    area.push_back(Span{"clipwise", l.clip_off[g], items * C});
    n_win += wg.groups[g].nw;
  }
  CHECK(n_win == wg.n_win, "windows in groups");
  area.push_back(Span{"vote thresholds", l.vthr, 2 * C});                                            // [C] f64
  area.push_back(Span{"tables", l.tables, l.table_bytes / 4});
  CHECK(l.total_bytes % 256 == 0 && l.table_bytes % 256 == 0, "window totals");
  check_spans(area, l.model_bytes / 4, l.total_bytes / 4, "window area");
  // the tables, in floats of the table block: starts, bases, strides [n_win] i64; off [N + 1] i32; src int2; div [N] i32
  const size_t N = (size_t)wg.plan.N;
  check_spans({Span{"start", l.t_start / 4, 2 * (size_t)n_win}, Span{"wb", l.t_wb / 4, 2 * (size_t)n_win},
               Span{"wcs", l.t_wcs / 4, 2 * (size_t)n_win}, Span{"off", l.t_off / 4, N + 1},
               Span{"src", l.t_src / 4, 2 * wg.plan.src.size()}, Span{"div", l.t_div / 4, N}},
              0, l.table_bytes / 4, "window tables");
  for (size_t b : {l.t_start, l.t_wb, l.t_wcs, l.t_off, l.t_src, l.t_div}) CHECK(b % 256 == 0, "table offset %zu", b);
  return true;
}

int check_plans() {
  int n = 0;
  for (int model_type : {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 13, 15, 16, 17, 19}) {   // every sedx_model_type
    const Model m = model_of(model_type, 25, 512, SEDX_FEATURE_LOGMEL);
    Tuning t;
    for (t.precision = 0; t.precision < 3; ++t.precision)
      for (t.wino_block1 = 0; t.wino_block1 < 3; ++t.wino_block1)
        for (t.wino_f43 = 0; t.wino_f43 < 3; ++t.wino_f43)
          for (int pipe = 0; pipe < 2; ++pipe)
            for (int64_t B : {1, 7, 8, 32, 530})
              for (int64_t T : {8, 9, 34, 64, 734, 1001, 6131}) {
                t.pipelined = pipe != 0;
                ForwardPlan p;   // the other trunks: the generic checks; their drivers hold what is theirs alone
                if (m.depth == 9) check_plan(m, t, B, T);
                else check_plan_regions(m, t, B, T, &p);
                ++n;
              }
  }
  // every model at the shapes the family drivers plan: both sides of each trunk's and each frame rule's limits
  const int64_t shapes[21][2] = {{1, 16},   {3, 17},    {2, 31},    {1, 32},    {1, 33},     {3, 63},     {33, 64},
                                 {5, 66},   {3, 112},   {33, 161},  {3, 200},   {5, 501},    {32, 1001},  {1, 1001},
                                 {3, 1343}, {1, 4127},  {2, 16015}, {2, 16032}, {1, 32000},  {1, 32031},  {1, 32032}};
  for (int model_type : {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 13, 15, 16, 17, 19})
    for (int precision = 0; precision < 3; ++precision)
      for (const auto& sh : shapes) {
        Tuning t;
        t.precision = precision;
        ForwardPlan p;
        check_plan_regions(model_of(model_type), t, sh[0], sh[1], &p), ++n;
      }
  const Model gru = model_of(SEDX_MODEL_GRU_FRAMEATT, 25, 512, SEDX_FEATURE_LOGMEL);
  for (int kernel = 0; kernel < 8; ++kernel)
    for (int handoff = 0; handoff < 4; ++handoff)
      for (int pipe = 0; pipe < 2; ++pipe) {
        Tuning t;
        t.gru_kernel = kernel;
        t.gru_handoff = handoff;
        t.pipelined = pipe != 0;
        check_plan(gru, t, 32, 1001), ++n;
      }
  // rejections: no frame left after the third pool; a sequence past the
  // Conformer's positional table; item counts past the launches' 32-bit sizes
  const Model cf = model_of(SEDX_MODEL_CONFORMER_FRAMEATT, 25, 512, SEDX_FEATURE_LOGMEL);
  check_plan(gru, Tuning(), 1, 7), ++n;
  check_plan(cf, Tuning(), 1, 8 * 5001), ++n;
  check_plan(cf, Tuning(), 1, 8 * 5000), ++n;
  check_plan(gru, Tuning(), 530, 63310), ++n;      // 530 x 63,310 > INT32_MAX / 64 = 33,554,431
  check_plan(gru, Tuning(), 530, 63309), ++n;      // the largest that fits
  struct Case { int driver; bool overlap; int sd; double ov, secs; };
  const Case cases[15] = {{0, true, 5, 1.0, 10.0}, {0, true, 5, 0.5, 23.0}, {0, false, 5, 1.0, 23.0}, {0, false, 5, 0.7, 17.3},
                          {0, true, 6, 0.5, 71.3}, {0, true, 5, 1.0, 187.37}, {0, true, 5, 1.0, 3.2}, {1, true, 5, 0.7, 10.0},
                          {1, true, 6, 0.9, 10.0}, {1, true, 7, 1.3, 10.0}, {1, true, 5, 0.1, 10.0}, {1, true, 5, 0.3, 9.9},
                          {1, true, 5, 1.0, 12.3}, {1, true, 6, 0.5, 8.7}, {1, true, 7, 0.9, 14.1}};
  for (const Case& c : cases)
    for (int64_t n_clips : {1, 3})
      for (const Model* m : {&gru, &cf}) {
        const bool planned = check_window_plan(*m, Tuning(), c.driver, c.overlap, c.sd, c.ov, c.secs, n_clips);
        // 7 s windows every 0.9 s over 14.1 s: the one case whose averaged merge numpy refuses
        CHECK(planned || (c.sd == 7 && c.secs == 14.1), "window case sd %d ov %g %g s: the merge raises", c.sd, c.ov, c.secs);
        n += planned;
      }
  return n;
}

// plan_conv_launch walked the way the launchers walk it (one plan per launch
// of whole clips), against what the kernels' item decode and 32-bit offsets assume
int check_launch_plans() {
  struct Layer { int F, cin, cout, epi; };
  static const Layer layers[7] = {{64, 64, 64, EPI_POOL2},   {32, 64, 128, EPI_STORE},  {32, 128, 128, EPI_POOL2},
                                  {16, 128, 256, EPI_STORE}, {16, 256, 256, EPI_POOL2}, {8, 256, 512, EPI_STORE},
                                  {8, 512, 512, EPI_FMEAN}};
  int n = 0;
  for (WinoFamily fam : {WINO_F23, WINO_F23_BLOCK1, WINO_F43})
    for (int li = 0; li < (fam == WINO_F23_BLOCK1 ? 1 : 7); ++li)
      for (int64_t B : {1, 2, 3, 7, 8, 9, 31, 32, 130, 131, 523, 524, 600})
        for (int T : {1, 2, 3, 8, 9, 64, 136, 1001})
          for (int ncu : {1, 7, 8, 64, 256, 304})
            for (int order = 0; order < 3; ++order)
              for (int c4 = 0; c4 < 2; ++c4)
                for (int ntf : {0, 1, 2, 4}) {
                  const Layer& l = layers[li];
                  const bool f43 = fam == WINO_F43, sched = B >= 8;
                  const char* want = fam == WINO_F23_BLOCK1 && T < 2                              ? "empty batch or clip"
                                     : f43 && ntf == 2 && !(c4 && (l.F == 16 || l.F == 8))       ? "16-tile items"
                                     : l.epi == EPI_POOL2 && T < 2                                ? "no tile row"
                                                                                                  : nullptr;
                  int64_t b0 = 0;
                  do {
                    const ConvLaunch p = plan_conv_launch(fam, ncu, B - b0, T, l.F, l.cin, l.cout, l.epi, order, c4 != 0, ntf, sched);
                    CHECK((p.reject == nullptr) == (want == nullptr), "family %d layer %d B %lld T %d ncu %d: %s", fam, li,
                          (long long)B, T, ncu, p.reject ? p.reject : "accepted");
                    if (p.reject) {
                      CHECK(std::strstr(p.reject, want) != nullptr && b0 == 0, "reason '%s' at clip %lld", p.reject, (long long)b0);
                      break;
                    }
                    CHECK(p.clips_per_launch >= 1 && p.clips >= 1 && p.clips == std::min(B - b0, p.clips_per_launch), "clips %d", p.clips);
                    const int64_t in = (int64_t)p.clips * T * (fam == WINO_F23_BLOCK1 ? 64 : l.F * l.cin);
                    CHECK(p.in_clip * p.clips == in && (f43 ? 4 * in : in) < INT32_MAX, "family %d: %lld input floats in one launch", fam, (long long)in);
                    CHECK(p.nwg >= 1 && p.nwg <= p.nitems && p.nwg % 8 == 0, "nwg %d of %d items", p.nwg, p.nitems);
                    CHECK(p.order2d == 0 || p.order2d == -1 || (p.order2d > 0 && p.ngroups % p.order2d == 0), "order2d %d of %d groups", p.order2d, p.ngroups);
                    CHECK(!p.claim || (f43 && sched && p.nwg == ncu / 8 * 8), "claim with %d workgroups on %d CUs", p.nwg, ncu);
                    CHECK(f43 ? (p.NT == 4 && p.TG == 2) || (p.NT == 1 && (p.TG == 2 || (p.TG == 1 && c4 && l.F <= 16)))
                              : p.TG >= 1 && p.TG <= 4 && (p.NT == 1 || p.NT == 2), "item %d x %d", p.TG, p.NT);
                    CHECK(p.tb_per_clip >= 1 && p.ngroups >= 1 && (int64_t)p.nitems >= (int64_t)p.clips * p.tb_per_clip * p.ngroups, "items");
                    b0 += p.clips;
                    ++n;
                  } while (b0 < B);
                }
  return n;
}

// plan_linear_launch over the sequence and head GEMMs at both sides of every
// kernel switch: the grid covers C [M][N] exactly once in the kernel's tiles,
// and the kernel's own conditions on K and N hold
int check_gemm_plans() {
  struct Gemm { int K, N, act; };
  static const Gemm gemms[7] = {{2048, 6144, 0}, {2048, 1536, 0}, {512, 2048, 1}, {2048, 64, 0},
                                {512, 1536, 0},  {512, 512, 1},   {512, 128, 0}};
  int n = 0;
  for (const Gemm& g : gemms)
    for (int M : {1, 128, 256, 257, 896, 897, 1280, 1281, 1408})
      for (int ncu : {1, 7, 8, 64, 256, 304}) {
        const GemmLaunch p = plan_linear_launch(M, g.K, g.N, g.act, ncu);
        const bool tiled = p.kernel == GEMM_TILED;
        CHECK(tiled || p.kernel == GEMM_ONE_WAVE || p.kernel == GEMM_KSPLIT, "kernel %d", p.kernel);
        const int tm = tiled ? 128 : 32, tn = tiled ? 64 : 32;
        CHECK(p.grid_x >= 1 && (int64_t)p.grid_x * tm >= M && (int64_t)(p.grid_x - 1) * tm < M, "M %d: %d row tiles of %d", M, p.grid_x, tm);
        CHECK(p.grid_y * tn == g.N, "N %d: %d column tiles of %d", g.N, p.grid_y, tn);
        CHECK(p.threads == (p.kernel == GEMM_ONE_WAVE ? 64 : 256), "threads %d", p.threads);
        CHECK(g.K % (tiled ? 16 : p.kernel == GEMM_KSPLIT ? 256 : 64) == 0, "K %d in kernel %d", g.K, p.kernel);
        CHECK((p.kernel == GEMM_KSPLIT) == (g.N <= 64 && g.act == 0), "K-split at N %d act %d", g.N, g.act);
        CHECK(p.kernel == GEMM_KSPLIT || tiled == ((int64_t)((M + 127) / 128) * (g.N / 64) >= ncu), "M %d N %d on %d CUs: kernel %d", M, g.N, ncu, p.kernel);
        ++n;
      }
  return n;
}
}  // namespace

int main() {
  int cases = 0, ok = 0;
  std::vector<std::vector<uint8_t>> good = {
      wav(1, 1, 16000, 16, 64, false, 64),      wav(1, 2, 44100, 24, 96, false, 96),
      wav(3, 1, 32000, 32, 128, false, 128),    wav(3, 2, 8000, 64, 160, true, 160),
      wav(1, 1, 16000, 8, 33, false, 0),        wav(1, 1, 16000, 16, 40, false, 0xFFFFFFFFu),
      wav(1, 3, 16000, 16, 50, false, 1u << 31),
  };
  std::vector<std::vector<uint8_t>> bad = {
      wav(1, 0, 16000, 16, 64, false, 64),      wav(1, 65535, 16000, 16, 64, false, 64),
      wav(2, 1, 16000, 16, 64, false, 64),      wav(1, 1, 0, 16, 64, false, 64),
      wav(1, 1, 16000, 0, 64, false, 64),       wav(1, 1, 16000, 12, 64, false, 64),
      wav(3, 1, 16000, 16, 64, true, 64),
  };
  for (auto& g : good) cases += parse_all_prefixes(g, &ok);
  for (auto& g : bad) cases += parse_all_prefixes(g, &ok);
  // chunk sizes that run past the buffer or wrap
  for (uint32_t sz : {0u, 1u, 15u, 17u, 39u, 0x7FFFFFFFu, 0xFFFFFFF0u, 0xFFFFFFFFu}) {
    std::vector<uint8_t> v = good[0];
    std::memcpy(v.data() + 16, &sz, 4);   // fmt chunk size
    cases += parse_all_prefixes(v, &ok);
  }
  std::mt19937 rng(1234);
  for (int it = 0; it < 4000; ++it) {
    std::vector<uint8_t> v = good[it % good.size()];
    const int flips = 1 + (int)(rng() % 6);
    for (int f = 0; f < flips; ++f) v[rng() % v.size()] = (uint8_t)rng();
    std::vector<uint8_t> buf(v);
    sedx_wav_info info;
    if (sedx_wav_parse(buf.data(), buf.size(), &info) == SEDX_OK) {
      ++ok;
      if (info.data_offset + info.data_bytes > (int64_t)buf.size()) std::abort();
    }
    ++cases;
  }

  // ---- vad (sedx_events) ----
  const int64_t C = 3;
  std::vector<double> hi = {0.5, 0.5, 0.9}, lo = {0.3, -0.1, 0.95};
  std::vector<int64_t> ns = {10, 0, 3}, nsalt = {10, 0, 1};
  int vad_cases = 0;
  for (int64_t T : {1, 2, 3, 17, 100, 1000}) {
    for (int pattern = 0; pattern < 6; ++pattern) {
      std::vector<float> x((size_t)2 * T * C);
      for (size_t i = 0; i < x.size(); ++i) {
        const int64_t t = (int64_t)(i / C) % T;
        switch (pattern) {
          case 0: x[i] = 1.0f; break;
          case 1: x[i] = 0.0f; break;
          case 2: x[i] = (t == 0 || t == T - 1) ? 0.8f : 0.1f; break;
          case 3: x[i] = (t % 2) ? 0.8f : 0.35f; break;
          default: x[i] = (float)(rng() % 1000) / 1000.0f; break;
        }
      }
      for (int use_lo = 0; use_lo < 2; ++use_lo)
        for (int64_t cap : {0, 1, 4096}) {
          std::vector<int32_t> ev((size_t)(cap > 0 ? cap : 1) * 4);
          int64_t n = 0;
          (void)sedx_events(x.data(), 2, T, C, hi.data(), lo.data(), use_lo, ns.data(), nsalt.data(),
                            cap > 0 ? ev.data() : nullptr, cap, &n);
          ++vad_cases;
        }
    }
  }
  const int weight_checks = check_weights();
  const int plan_checks = check_plans();
  const int launch_checks = check_launch_plans();
  const int gemm_checks = check_gemm_plans();
  std::printf("asan_driver: %d wav_parse cases (%d accepted), %d vad cases, %d weight-pack checks, %d plan checks, "
              "%d conv launch plans, %d GEMM launch plans\n", cases, ok, vad_cases, weight_checks, plan_checks,
              launch_checks, gemm_checks);
  return host_check::finish("asan_driver");
}
