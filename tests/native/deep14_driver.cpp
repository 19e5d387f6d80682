// Host side of the 14-layer models under AddressSanitizer + UBSan (make
// asan-deep14): the forward plan (regions inside the workspace, disjoint where
// they are live together), expected_params of both key sets and the deep conv
// weight pack read back by a direct index computation.  No GPU, no preload.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../sound-event-detection_amd/csrc/plan.h"
#include "../../sound-event-detection_amd/csrc/weights.h"

using namespace sedx;

static int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      ++failures;                             \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
    }                                         \
  } while (0)

static Model model_of(int type) {
  sedx_config cfg{};
  cfg.model_type = type;
  cfg.feature_type = SEDX_FEATURE_LOGMEL;
  cfg.sample_rate = 16000, cfg.window_size = 512, cfg.hop_size = 160, cfg.mel_bins = 64;
  cfg.fmin = 25, cfg.fmax = 7000, cfg.classes_num = 25;
  Model m;
  if (!make_model(cfg, &m)) {
    std::printf("FAIL make_model(%d)\n", type);
    std::exit(1);
  }
  return m;
}

static bool disjoint(const Region& a, const Region& b) {
  return a.floats == 0 || b.floats == 0 || a.off + a.floats <= b.off || b.off + b.floats <= a.off;
}
static bool inside(const Region& a, const Region& outer) { return a.off >= outer.off && a.off + a.floats <= outer.off + outer.floats; }

static void check_params(int type, bool gru) {
  const Model m = model_of(type);
  CHECK(m.depth == 14 && m.hw == 2048 && m.nac == 64 && m.head == HEAD_ATT, "model %d", type);
  const auto e = expected_params(m);
  auto has = [&](const std::string& k, std::vector<int64_t> sh) {
    auto it = e.find(k);
    CHECK(it != e.end() && it->second == sh, "expected_params(%d): %s", type, k.c_str());
  };
  has("conv_block4.conv2.weight", {512, 512, 3, 3});
  has("conv_block5.conv1.weight", {1024, 512, 3, 3});
  has("conv_block5.conv2.weight", {1024, 1024, 3, 3});
  has("conv_block6.conv1.weight", {2048, 1024, 3, 3});
  has("conv_block6.conv2.weight", {2048, 2048, 3, 3});
  has("conv_block6.bn2.running_var", {2048});
  has("att_block.att.weight", {25, 2048, 1});
  has("att_block.bn_att.weight", {25});
  if (gru) {
    has("gru.weight_ih_l0", {3072, 2048});
    has("gru.weight_hh_l0_reverse", {3072, 1024});
    has("gru.bias_hh_l0", {3072});
    CHECK(!e.count("multihead.fc.weight"), "GRU model expects MultiHead keys");
  } else {
    has("multihead.w_qs.weight", {512, 2048});
    has("multihead.fc.weight", {2048, 512});
    has("multihead.fc.bias", {2048});
    has("multihead.layer_norm.weight", {2048});
    CHECK(!e.count("gru.weight_ih_l0"), "Transformer model expects GRU keys");
  }
  // 3 frontend + 4 bn0 + 6 x (2 conv + 8 bn) + 4 att/cla + 4 bn_att, then the sequence layer's
  CHECK(e.size() == size_t(3 + 4 + 60 + 8 + (gru ? 8 : 10)), "expected_params(%d): %zu keys", type, e.size());
}

static void check_plan(int type, int precision, int64_t B, int64_t T) {
  const Model m = model_of(type);
  Tuning t;
  t.precision = precision;
  ForwardPlan p;
  const char* why = plan_forward(m, t, B, T, &p);
  const int64_t T5 = T / 32;
  CHECK((why != nullptr) == (T5 < 1), "plan_forward(%d, B %lld, T %lld): %s", type, (long long)B, (long long)T, why ? why : "accepted");
  CHECK(p.g.Ts == T5 && p.g.rep == 32 && p.g.fw_len == 32 * T5, "geometry of T %lld", (long long)T);
  const int64_t n = 32 * T5, padded = n == 1000 || n % 100 == 0 ? n : n + 100 - n % 100;
  CHECK(p.g.out_frames == padded, "out_frames %lld of T %lld", (long long)p.g.out_frames, (long long)T);
  if (why) return;
  CHECK(p.nlayers == 11 && p.first_deep == 6 && p.M == B * T5, "layer list");
  const Region all{0, p.total_bytes / 4};
  const Region* top[4] = {&p.x0, &p.A, &p.P, &p.sched};
  for (int i = 0; i < 4; ++i) {
    CHECK(inside(*top[i], all), "region %d outside the workspace", i);
    for (int j = i + 1; j < 4; ++j) CHECK(disjoint(*top[i], *top[j]), "regions %d and %d overlap", i, j);
  }
  const Region* head[4] = {&p.G, &p.Hs, &p.O, &p.LG};
  for (int i = 0; i < 4; ++i) {
    CHECK(inside(*head[i], p.A), "head region %d outside A", i);
    for (int j = i + 1; j < 4; ++j) CHECK(disjoint(*head[i], *head[j]), "head regions %d and %d overlap", i, j);
  }
  const bool gru = m.seq == SEQ_GRU;
  CHECK(p.G.floats >= (size_t)p.M * (gru ? 6144 : 1536) && p.Hs.floats >= (size_t)p.M * 2048 &&
            p.O.floats >= (size_t)p.M * 512 && p.LG.floats >= (size_t)p.M * 64,
        "head region sizes");
  // the conv chain: each launch reads what the previous one wrote, in the other buffer, inside it
  static const int cin[11] = {64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024, 2048};
  static const int cout[11] = {64, 128, 128, 256, 256, 512, 512, 1024, 1024, 2048, 2048};
  for (int i = 0; i < p.nlayers; ++i) {
    const ConvLayer& c = p.layers[i];
    CHECK(c.cin == cin[i] && c.cout == cout[i], "layer %d channels %d -> %d", i, c.cin, c.cout);
    const Region& dst = i % 2 ? p.A : p.P;
    const Region out{c.out, (size_t)B * c.To * c.Fo * c.cout};
    CHECK(inside(out, dst), "layer %d output outside its buffer", i);
    if (i > 0) {
      const ConvLayer& q = p.layers[i - 1];
      CHECK(c.in == q.out && c.T == q.To && c.F == q.Fo && c.cin == q.cout, "layer %d does not read layer %d", i, i - 1);
    }
    if (i >= 6) {
      const int F = i == 6 ? 8 : i < 9 ? 4 : 2;
      const int epi = i == 10 ? EPI_FMEAN : i % 2 == 0 ? EPI_POOL2 : EPI_STORE;
      CHECK(c.F == F && c.epi == epi && c.cin % DEEP_CK == 0 && c.cout % DEEP_BN == 0, "deep layer %d", i);
    }
  }
  CHECK(p.layers[10].To == T5 && p.layers[10].Fo == 1 && p.layers[10].out == p.P.off, "the sequence input is not P");
}

static void check_pack(int Cin, int Cout) {
  std::vector<double> wf((size_t)Cout * Cin * 9);
  for (size_t i = 0; i < wf.size(); ++i) wf[i] = (double)(float)(1.0 + (double)i * 0.5);
  std::vector<float> out(wf.size(), NAN);
  pack_conv_deep(wf.data(), Cin, Cout, out.data());
  size_t bad = 0;
  for (int o = 0; o < Cout; ++o)
    for (int i = 0; i < Cin; ++i)
      for (int t = 0; t < 9; ++t) {
        // conv_deep_kernel: wave's group g = o / 32 at float4 index (((g nchunk + chunk) 9 + tap) 4 + q) 32 + n, element c
        const size_t g = o / 32, n = o % 32, chunk = i / 16, q = (i % 16) / 4, c = i % 4;
        const size_t f4 = (((g * (Cin / 16) + chunk) * 9 + t) * 4 + q) * 32 + n;
        if (out[f4 * 4 + c] != (float)wf[((size_t)o * Cin + i) * 9 + t]) ++bad;
      }
  for (float v : out)
    if (std::isnan(v)) ++bad;
  CHECK(bad == 0, "pack_conv_deep(%d, %d): %zu wrong slots", Cin, Cout, bad);
}

int main() {
  check_params(SEDX_MODEL_GRU14_FRAMEATT, true);
  check_params(SEDX_MODEL_TRANSFORMER14_FRAMEATT, false);
  const int precisions[3] = {SEDX_PRECISION_WINOGRAD, SEDX_PRECISION_EXACT, SEDX_PRECISION_X3};
  const int64_t shapes[6][2] = {{1, 32}, {3, 112}, {33, 64}, {32, 1001}, {2, 31}, {5, 501}};
  for (int type : {SEDX_MODEL_GRU14_FRAMEATT, SEDX_MODEL_TRANSFORMER14_FRAMEATT})
    for (int pr : precisions)
      for (const auto& s : shapes) check_plan(type, pr, s[0], s[1]);
  // a 9-layer plan keeps its seven launches
  {
    const Model m = model_of(SEDX_MODEL_GRU_FRAMEATT);
    ForwardPlan p;
    CHECK(plan_forward(m, Tuning(), 4, 1001, &p) == nullptr && p.nlayers == 7 && p.first_deep == 7 && p.g.Ts == 125 &&
              p.g.rep == 8,
          "9-layer plan");
  }
  check_pack(16, 128);
  check_pack(48, 256);
  check_pack(512, 1024);
  if (failures) {
    std::printf("deep14_driver: %d failures\n", failures);
    return 1;
  }
  std::printf("deep14_driver: clean\n");
  return 0;
}
