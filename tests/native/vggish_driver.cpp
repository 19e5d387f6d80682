// Host side of the three VGGish models under AddressSanitizer + UBSan (make
// asan-vggish): the models' settings, expected_params and the ignored gru.*
// keys, the geometry with its refusals, the forward plan (six launches, the new
// epilogue values, regions inside the workspace and disjoint where they are
// live together), the conv pack read back the way the kernel addresses it and
// the slots prepare_weights fills.  No GPU, no preload.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_check.h"

using namespace sedx;

static const int IDS[3] = {SEDX_MODEL_VGGISH_FRAMEATT, SEDX_MODEL_VGGISH_GRU_FRAMEATT, SEDX_MODEL_VGGISH_FRAMEAVG};

static void check_params() {
  CHECK(IDS[0] == 15 && IDS[1] == 16 && IDS[2] == 17, "model ids");
  sedx_config cfg{};
  cfg.model_type = 14;
  Model none;
  CHECK(!make_model(cfg, &none), "model id 14 is assigned");
  for (int id : IDS) {
    const Model m = model_of(id);
    const bool gru = id == SEDX_MODEL_VGGISH_GRU_FRAMEATT, avg = id == SEDX_MODEL_VGGISH_FRAMEAVG;
    CHECK(m.vgg && !m.decision && m.depth == VGG_LAYERS && m.hw == 512 && m.nac == 64 &&
              m.head == (avg ? HEAD_FC_AVG : HEAD_ATT) && m.seq == (gru ? SEQ_GRU : SEQ_NONE),
          "model settings of %d", id);
    const auto e = expected_params(m);
    auto has = [&](const std::string& k, std::vector<int64_t> sh) {
      auto it = e.find(k);
      CHECK(it != e.end() && it->second == sh, "expected_params(%d): %s", id, k.c_str());
    };
    has("spectrogram_extractor.stft.conv_real.weight", {257, 1, 512});
    has("logmel_extractor.melW", {257, 64});
    has("bn0.running_var", {64});
    for (int l = 0; l < VGG_LAYERS; ++l) {
      const std::string p = "vggish.0." + std::to_string(VGG_SEQ_INDEX[l]);
      has(p + ".weight", {VGG_COUT[l], VGG_CIN[l], 3, 3});
      has(p + ".bias", {VGG_COUT[l]});
    }
    CHECK(VGG_SEQ_INDEX[0] == 0 && VGG_SEQ_INDEX[1] == 3 && VGG_SEQ_INDEX[2] == 6 && VGG_SEQ_INDEX[3] == 8 &&
              VGG_SEQ_INDEX[4] == 11 && VGG_SEQ_INDEX[5] == 13, "Sequential indices");
    if (avg) has("fc.weight", {25, 512}), has("fc.bias", {25});
    else has("att_block.att.weight", {25, 512, 1}), has("att_block.cla.bias", {25}), has("att_block.bn_att.running_var", {25});
    CHECK(e.count("gru.weight_hh_l0_reverse") == (gru ? 1u : 0u), "gru keys of %d", id);
    // every class builds the GRU: the two that never call it accept and drop its keys
    CHECK(ignored_key(m, "gru.weight_ih_l0") == !gru && !ignored_key(m, "conv_block1.conv1.weight") &&
              !ignored_key(m, "multihead.fc.weight") && !ignored_key(m, "vggish.0.0.weight"),
          "ignored keys of %d", id);
    for (const char* k : {"conv_block1.conv1.weight", "conv_block4.bn2.weight", "multihead.fc.weight", "fc1.weight",
                          "encoder.input_layer.0.weight", avg ? "att_block.att.weight" : "fc.weight"})
      CHECK(!e.count(k), "model %d expects another family's key %s", id, k);
    // 3 frontend + 4 bn0 + 12 trunk + (8 gru) + (2 fc | 4 att/cla + 4 bn_att)
    CHECK(e.size() == size_t(3 + 4 + 12 + (gru ? 8 : 0) + (avg ? 2 : 8)), "expected_params(%d): %zu keys", id, e.size());
  }
  CHECK(!model_of(SEDX_MODEL_GRU_FRAMEATT).vgg && !model_of(SEDX_MODEL_CNN14_DECISIONLEVELATT).vgg, "vgg flag");
  CHECK(!ignored_key(model_of(SEDX_MODEL_CNN_FRAMEATT), "gru.weight_ih_l0"), "a 9-layer CNN model drops gru keys");
}

// T frames: four flooring pools, always 1000 output frames; refusals as the header lists them
static void check_geometry() {
  Tuning t;
  for (int id : IDS) {
    const Model m = model_of(id);
    const bool att = m.head == HEAD_ATT;
    for (int64_t T = 1; T <= 16100; T = T < 1400 ? T + 1 : T + 97) {
      ForwardPlan p;
      const char* why = plan_forward(m, t, 1, T, &p);
      const int64_t seq = T / 2 / 2 / 2 / 2;
      const bool refuse = seq < 1 || (att ? seq > 83 : seq > 1000);
      CHECK((why != nullptr) == refuse, "model %d T %lld: %s", id, (long long)T, why ? why : "accepted");
      char buf[96];
      const char* vr = shape_refusal(m, T, buf, sizeof(buf));
      CHECK((vr != nullptr) == refuse && (!vr || std::strlen(vr) > 10), "shape_refusal(%d, %lld)", id, (long long)T);
      if (why) {
        CHECK(std::strlen(why) > 10 && (!vr || std::strcmp(why, vr) == 0), "the plan's reason at T %lld", (long long)T);
        continue;
      }
      const Geometry g = geometry_from_T(m, T);
      const int rep = att ? 12 : (int)(1000 / seq);
      CHECK(g.Ts == seq && g.T1 == T / 2 && g.T2 == T / 4 && g.T3 == T / 8 && g.T4 == seq && g.rep == rep &&
                g.fw_len == rep * seq && g.fw_len <= 1000 && g.out_frames == 1000,
            "geometry of model %d at T %lld", id, (long long)T);
    }
    ForwardPlan p;
    const int64_t edges[6] = {15, 16, 1343, 1344, 16015, 16016};   // seq 0, 1, 83, 84, 1000, 1001
    const bool ok_att[6] = {false, true, true, false, false, false}, ok_avg[6] = {false, true, true, true, true, false};
    for (int i = 0; i < 6; ++i)
      CHECK((plan_forward(m, t, 2, edges[i], &p) == nullptr) == (att ? ok_att[i] : ok_avg[i]), "model %d edge T %lld", id,
            (long long)edges[i]);
  }
  char buf[96];
  CHECK(shape_refusal(model_of(SEDX_MODEL_GRU_FRAMEATT), 1344, buf, sizeof(buf)) == nullptr, "the VGGish limits on a 9-layer model");
}

static void check_plan(int id, int precision, int64_t B, int64_t T) {
  const Model m = model_of(id);
  Tuning t;
  t.precision = precision;
  ForwardPlan p;
  const char* why = plan_forward(m, t, B, T, &p);
  CHECK(why == nullptr, "plan_forward(%d, B %lld, T %lld): %s", id, (long long)B, (long long)T, why ? why : "");
  if (why) return;
  const int64_t T1 = T / 2, T2 = T1 / 2, T3 = T2 / 2, T4 = T3 / 2;
  CHECK(p.nlayers == 5 && p.first_deep == 5 && p.M == B * T4 && p.block1 == B1_VGG && p.family == CONV_EXACT && !p.c4 &&
            !p.claims,
        "launch list");
  WinoFamily wf;
  for (int i = 0; i < 5; ++i) CHECK(!conv_launch_family(p, i, &wf), "layer %d on a Winograd launcher", i);
  CHECK(EPI_MAXPOOL2 == 3 && EPI_MAXPOOL2_FMEAN == 4, "ConvEpi values");
  const Region all{0, p.total_bytes / 4};
  for (int i = 0; i < 5; ++i) {   // the layer table and the chain: asan_driver's check_plans
    const ConvLayer& c = p.layers[i];
    const Region in{c.in, (size_t)B * c.T * c.F * c.cin}, out{c.out, (size_t)B * c.To * c.Fo * c.cout};
    CHECK(inside(in, all) && inside(out, all) && disjoint(in, out), "layer %d reads what it writes", i);
  }
  // conv1's pooled output [B][T1][32][64] is layer 0's input, inside A
  CHECK(p.A.floats >= (size_t)B * T1 * 32 * 64 && p.layers[0].in == p.A.off, "conv1's output");
  // the sequence input S = P; G, H, O, the logits and the recurrence's scratch inside A, pairwise disjoint
  const Region* head[5] = {&p.G, &p.Hs, &p.O, &p.LG, &p.gru};
  for (int i = 0; i < 5; ++i) {
    CHECK(inside(*head[i], p.A), "head region %d outside A", i);
    for (int j = i + 1; j < 5; ++j) CHECK(disjoint(*head[i], *head[j]), "head regions %d and %d overlap", i, j);
  }
  CHECK(p.layers[4].out == p.P.off && p.P.floats >= (size_t)p.M * 512 && p.Hs.floats >= (size_t)p.M * 512 &&
            p.LG.floats >= (size_t)p.M * m.nac && p.G.floats >= (size_t)p.M * 1536,
        "sequence / head sizes");
  const auto rows = plan_gemm_launches(p, 256);
  CHECK(rows.size() == (m.seq == SEQ_GRU ? 2u : 1u) && rows.back().stage == 10 && rows.back().N == 64 && rows.back().K == 512,
        "GEMM rows");
}

// pack_vgg_conv: weight (o, i, tap) at exact_pack_index, the value unchanged, every slot written once
static void check_pack(int l) {
  const int cin = VGG_CIN[l], cout = VGG_COUT[l];
  std::vector<float> w((size_t)cout * cin * 9);
  for (size_t i = 0; i < w.size(); ++i) w[i] = 0.25f + (float)(i % 65521) * 0.5f;
  const std::vector<float> pk = pack_vgg_conv(w.data(), cin, cout);
  CHECK(pk.size() == w.size(), "pack size of layer %d", l);
  size_t bad = 0;
  std::vector<unsigned char> seen(pk.size(), 0);
  for (int o = 0; o < cout; ++o)
    for (int i = 0; i < cin; ++i)
      for (int t = 0; t < 9; ++t) {
        const size_t at = exact_pack_index(cout, o, i, t);
        if (at >= pk.size() || seen[at]++ || pk[at] != w[((size_t)o * cin + i) * 9 + t]) ++bad;
      }
  CHECK(bad == 0, "pack_vgg_conv(layer %d): %zu wrong slots", l, bad);
}

// prepare_weights: a missing key is named; with every key, the six packs sit in c1_w / c1_b and wp[1..5] / cb[1..5],
// bn0 is the identity whatever was loaded, and nothing lands in another conv slot
static void check_prepare(int id) {
  const Model m = model_of(id);
  Params P;
  for (const auto& kv : expected_params(m)) {
    Tensor t;
    t.shape = kv.second;
    size_t n = 1;
    for (auto d : kv.second) n *= (size_t)d;
    t.data.assign(n, 0.f);
    for (size_t i = 0; i < n; ++i) t.data[i] = 0.001f * (float)((i * 7 + kv.first.size()) % 1000) - 0.5f;
    P[kv.first] = t;
  }
  // a windowed DFT the FFT frontend accepts: window w[n] = 1, conv_real = cos, conv_imag = sin
  auto& wr = P["spectrogram_extractor.stft.conv_real.weight"].data;
  auto& wi = P["spectrogram_extractor.stft.conv_imag.weight"].data;
  for (int k = 0; k < 257; ++k)
    for (int n = 0; n < 512; ++n) {
      const double ang = -2.0 * M_PI * (double)((int64_t)n * k % 512) / 512;
      wr[(size_t)k * 512 + n] = (float)std::cos(ang), wi[(size_t)k * 512 + n] = (float)std::sin(ang);
    }
  for (auto& v : P["bn0.running_var"].data) v = 2.0f;
  DevWeights W;
  WeightBlob blob;
  GammaGeom gg;
  std::string err;
  Params Q = P;
  Q.erase("vggish.0.11.bias");
  CHECK(prepare_weights(m, Q, &W, &blob, &gg, &err) == SEDX_EKEY && err.find("vggish.0.11.bias") != std::string::npos,
        "a missing key is not named: %s", err.c_str());
  const sedx_status st = prepare_weights(m, P, &W, &blob, &gg, &err);
  CHECK(st == SEDX_OK, "prepare_weights(%d): %s", id, err.c_str());
  if (st != SEDX_OK) return;
  blob.bind(blob.image.data());   // host addresses: read the image as the device would
  const char* lo = blob.image.data();
  const char* hi = lo + blob.image.size();
  auto in_image = [&](const void* p, size_t bytes) { return (const char*)p >= lo && (const char*)p + bytes <= hi; };
  CHECK(in_image(W.c1_w, 576 * 4) && in_image(W.c1_b, 64 * 4) && in_image(W.zero, ZERO_BLOCK_FLOATS * 4), "conv1 slots");
  if (in_image(W.c1_w, 576 * 4))
    CHECK(std::memcmp(W.c1_w, P["vggish.0.0.weight"].data.data(), 576 * 4) == 0 &&
              std::memcmp(W.c1_b, P["vggish.0.0.bias"].data.data(), 64 * 4) == 0,
          "conv1's weights are not the state_dict's");
  for (int l = 1; l < VGG_LAYERS; ++l) {
    const size_t n = (size_t)9 * VGG_CIN[l] * VGG_COUT[l];
    CHECK(in_image(W.wp[l], n * 4) && in_image(W.cb[l], VGG_COUT[l] * 4), "slot %d", l);
    if (!in_image(W.wp[l], n * 4)) continue;
    const auto& w = P["vggish.0." + std::to_string(VGG_SEQ_INDEX[l]) + ".weight"].data;
    const auto& b = P["vggish.0." + std::to_string(VGG_SEQ_INDEX[l]) + ".bias"].data;
    size_t bad = 0;
    for (int o = 0; o < VGG_COUT[l]; o += 7)
      for (int i = 0; i < VGG_CIN[l]; i += 3)
        for (int t = 0; t < 9; ++t)
          if (W.wp[l][exact_pack_index(VGG_COUT[l], o, i, t)] != w[((size_t)o * VGG_CIN[l] + i) * 9 + t]) ++bad;
    CHECK(bad == 0 && std::memcmp(W.cb[l], b.data(), b.size() * 4) == 0, "pack in slot %d: %zu wrong", l, bad);
  }
  CHECK(!W.wp[0] && !W.wp[6] && !W.wp[7] && !W.cb[6] && !W.cb[7] && !W.c1_wt, "a conv slot the trunk does not use is set");
  for (int k = 0; k < 8; ++k) CHECK(!W.wx3[k] && !W.wu[k] && !W.wu43[k], "an x3 / Winograd pack at %d", k);
  for (int i = 0; i < 64; ++i)
    CHECK(W.bn0_scale[i] == 1.0f && W.bn0_mean[i] == 0.0f && W.bn0_bias[i] == 0.0f, "bn0 is not the identity at %d", i);
  CHECK((W.w_ih != nullptr) == (m.seq == SEQ_GRU) && (W.whh != nullptr) == (m.seq == SEQ_GRU) && W.wac && W.bac && W.wac_x3,
        "sequence / head packs of %d", id);
}

int main() {
  check_params();
  check_geometry();
  const int precisions[3] = {SEDX_PRECISION_WINOGRAD, SEDX_PRECISION_EXACT, SEDX_PRECISION_X3};
  const int64_t shapes[8][2] = {{1, 16}, {3, 17}, {2, 31}, {5, 66}, {33, 161}, {32, 1001}, {1, 1001}, {3, 1343}};
  for (int id : IDS)
    for (int pr : precisions)
      for (const auto& s : shapes) check_plan(id, pr, s[0], s[1]);
  check_plan(SEDX_MODEL_VGGISH_FRAMEAVG, SEDX_PRECISION_WINOGRAD, 2, 16015);
  for (int l = 1; l < VGG_LAYERS; ++l) check_pack(l);
  for (int id : IDS) check_prepare(id);
  return host_check::finish("vggish_driver");
}
