// Host side of the 14-layer models under AddressSanitizer + UBSan (make
// asan-deep14): the geometry and the head regions of the forward plan (its
// top-level regions and conv chain: asan_driver's check_plans, over every
// model), expected_params of both key sets and the deep conv weight pack read
// back by a direct index computation.  No GPU, no preload.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_check.h"

using namespace sedx;

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
  const Region* head[4] = {&p.G, &p.Hs, &p.O, &p.LG};
  for (int i = 0; i < 4; ++i) {
    CHECK(inside(*head[i], p.A), "head region %d outside A", i);
    for (int j = i + 1; j < 4; ++j) CHECK(disjoint(*head[i], *head[j]), "head regions %d and %d overlap", i, j);
  }
  const bool gru = m.seq == SEQ_GRU;
  CHECK(p.G.floats >= (size_t)p.M * (gru ? 6144 : 1536) && p.Hs.floats >= (size_t)p.M * 2048 &&
            p.O.floats >= (size_t)p.M * 512 && p.LG.floats >= (size_t)p.M * 64,
        "head region sizes");
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
  return host_check::finish("deep14_driver");
}
