// Host side of Cnn14_DecisionLevelAtt under AddressSanitizer + UBSan (make
// asan-cnn14): the model's settings at 25 and 527 classes, expected_params, the
// geometry closed form with its two refusals, the forward plan (regions inside
// the workspace, disjoint where they are live together) and the 527-class head
// pack read back row by row.  No GPU, no preload.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_check.h"

using namespace sedx;

static void check_params(int classes, bool k32) {
  const Model m = model_of(SEDX_MODEL_CNN14_DECISIONLEVELATT, classes, 512, SEDX_FEATURE_LOGMEL, k32);
  const int nac = (2 * classes + 63) / 64 * 64;
  CHECK(m.decision && m.depth == 14 && m.hw == 2048 && m.nac == nac && m.head == HEAD_ATT && m.seq == SEQ_NONE,
        "model settings at %d classes (nac %d)", classes, m.nac);
  const auto e = expected_params(m);
  auto has = [&](const std::string& k, std::vector<int64_t> sh) {
    auto it = e.find(k);
    CHECK(it != e.end() && it->second == sh, "expected_params(%d classes): %s", classes, k.c_str());
  };
  const int64_t W = k32 ? 1024 : 512;
  has("spectrogram_extractor.stft.conv_real.weight", {W / 2 + 1, 1, W});
  has("logmel_extractor.melW", {W / 2 + 1, 64});
  has("conv_block6.conv2.weight", {2048, 2048, 3, 3});
  has("fc1.weight", {2048, 2048});
  has("fc1.bias", {2048});
  has("att_block.att.weight", {classes, 2048, 1});
  has("att_block.cla.bias", {classes});
  has("att_block.bn_att.running_var", {classes});
  for (const char* k : {"gru.weight_ih_l0", "multihead.fc.weight", "fc.weight", "encoder.input_layer.0.weight"})
    CHECK(!e.count(k), "the model expects another family's key %s", k);
  // 3 frontend + 4 bn0 + 6 x (2 conv + 8 bn) + 2 fc1 + 4 att/cla + 4 bn_att
  CHECK(e.size() == size_t(3 + 4 + 60 + 2 + 8), "expected_params: %zu keys", e.size());
  // the other 14-layer models do not take fc1
  CHECK(!expected_params(model_of(SEDX_MODEL_GRU14_FRAMEATT, 25)).count("fc1.weight"), "fc1 on the GRU model");
  CHECK(!model_of(SEDX_MODEL_GRU14_FRAMEATT, 25).decision && !model_of(SEDX_MODEL_CNN_FRAMEATT, 25).decision, "decision flag");
}

// T = L / hop + 1 frames: T / 32 sequence frames, T - 1 framewise frames; T < 32 and T % 32 == 0 refused
static void check_geometry() {
  const Model m = model_of(SEDX_MODEL_CNN14_DECISIONLEVELATT, 25);
  Tuning t;
  for (int64_t T = 1; T <= 2100; ++T) {
    ForwardPlan p;
    const char* why = plan_forward(m, t, 1, T, &p);
    const bool refuse = T < 32 || T % 32 == 0;
    CHECK((why != nullptr) == refuse, "T %lld: %s", (long long)T, why ? why : "accepted");
    char buf[96];
    CHECK((shape_refusal(m, T, buf, sizeof(buf)) != nullptr) == refuse, "shape_refusal(%lld)", (long long)T);
    if (why) {
      CHECK(std::strlen(why) > 10, "a refusal without a reason at T %lld", (long long)T);
      continue;
    }
    const Geometry g = geometry_from_T(m, T);
    CHECK(g.Ts == T / 32 && g.rep == 32 && g.fw_len == 32 * (T / 32) && g.out_frames == T - 1 &&
              g.out_frames - g.fw_len == T % 32 - 1,
          "geometry of T %lld: %lld frames, %lld sequence frames", (long long)T, (long long)g.out_frames, (long long)g.Ts);
  }
  // the other 14-layer models keep their multiple-of-100 rule and take T % 32 == 0
  const Model g14 = model_of(SEDX_MODEL_GRU14_FRAMEATT, 25);
  ForwardPlan p;
  CHECK(plan_forward(g14, t, 1, 64, &p) == nullptr && p.g.out_frames == 100, "GRU14 at T 64");
  CHECK(geometry_from_T(g14, 1001).out_frames == 1000 && geometry_from_T(g14, 501).out_frames == 500, "GRU14 frames");
}

static void check_plan(int classes, int precision, int64_t B, int64_t T) {
  const Model m = model_of(SEDX_MODEL_CNN14_DECISIONLEVELATT, classes);
  Tuning t;
  t.precision = precision;
  ForwardPlan p;
  const char* why = plan_forward(m, t, B, T, &p);
  CHECK(why == nullptr, "plan_forward(B %lld, T %lld): %s", (long long)B, (long long)T, why ? why : "");
  if (why) return;
  const int64_t T5 = T / 32;
  // S = P (block 6's frequency mean), H and the logits inside A, no G / O
  CHECK(p.G.floats == 0 && p.O.floats == 0, "the model has no G / O region");
  CHECK(inside(p.Hs, p.A) && inside(p.LG, p.A) && disjoint(p.Hs, p.LG), "H / LG placement");
  CHECK(p.Hs.floats >= (size_t)p.M * 2048 && p.LG.floats >= (size_t)p.M * m.nac, "H / LG sizes");
  CHECK(p.P.floats >= (size_t)p.M * 2048, "the decision stage's input is not P");
}

// pack_head at 527 classes: row c = att, row C + c = cla, rows 2C .. nac - 1 zero
static void check_head_pack(int classes) {
  const Model m = model_of(SEDX_MODEL_CNN14_DECISIONLEVELATT, classes);
  Params P;
  auto fill = [&](const char* k, std::vector<int64_t> sh, float base) {
    Tensor t;
    t.shape = sh;
    size_t n = 1;
    for (auto d : sh) n *= (size_t)d;
    t.data.resize(n);
    for (size_t i = 0; i < n; ++i) t.data[i] = base + (float)(i % 4093);
    P[k] = t;
  };
  fill("att_block.att.weight", {classes, 2048, 1}, 1.f);
  fill("att_block.cla.weight", {classes, 2048, 1}, 5001.f);
  fill("att_block.att.bias", {classes}, 10001.f);
  fill("att_block.cla.bias", {classes}, 15001.f);
  std::vector<float> wac, bac;
  pack_head(m, P, &wac, &bac);
  CHECK(wac.size() == (size_t)m.nac * 2048 && bac.size() == (size_t)m.nac, "head pack sizes");
  size_t bad = 0;
  for (int r = 0; r < m.nac; ++r) {
    const bool att = r < classes, cla = !att && r < 2 * classes;
    const int c = att ? r : r - classes;
    for (int k = 0; k < 2048; ++k) {
      const float want = att   ? P["att_block.att.weight"].data[(size_t)c * 2048 + k]
                         : cla ? P["att_block.cla.weight"].data[(size_t)c * 2048 + k]
                               : 0.f;
      if (wac[(size_t)r * 2048 + k] != want) ++bad;
    }
    const float wb = att ? P["att_block.att.bias"].data[c] : cla ? P["att_block.cla.bias"].data[c] : 0.f;
    if (bac[r] != wb) ++bad;
  }
  CHECK(bad == 0, "pack_head(%d classes): %zu wrong slots", classes, bad);
}

int main() {
  check_params(25, false);
  check_params(527, true);
  check_params(33, false);
  check_geometry();
  const int precisions[3] = {SEDX_PRECISION_WINOGRAD, SEDX_PRECISION_EXACT, SEDX_PRECISION_X3};
  const int64_t shapes[7][2] = {{1, 33}, {3, 63}, {33, 161}, {32, 1001}, {1, 1001}, {5, 501}, {3, 200}};
  for (int classes : {25, 527})
    for (int pr : precisions)
      for (const auto& s : shapes) check_plan(classes, pr, s[0], s[1]);
  check_head_pack(25);
  check_head_pack(527);
  return host_check::finish("cnn14_driver");
}
