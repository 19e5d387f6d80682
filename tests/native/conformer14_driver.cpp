// Host side of Cnn_14layers_Conformer_FrameAtt under AddressSanitizer + UBSan (make asan-conformer14): the
// geometry table and its refusals (T = 31, 32, T5 = 1000, 1001), the forward plan's regions, the key table with
// both input-layer shapes and the ignored keys' shapes, and prepare_weights with the 2048-wide input layer read
// back from the image.  No GPU, no preload.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_check.h"

using namespace sedx;

// the reference's frame counts ("14-layer trunk"): sequence frames -> (ratio, framewise frames)
static void check_geometry() {
  const Model m = model_of(SEDX_MODEL_CONFORMER14_FRAMEATT);
  CHECK(m.depth == 14 && m.seq == SEQ_CONFORMER && m.head == HEAD_ATT && m.sw == 2048 && m.hw == CF_D && m.nac == 64,
        "the model's parts");
  static const int64_t rows[10][3] = {{1, 1000, 1000}, {2, 500, 1000},  {3, 333, 1000}, {15, 66, 1000}, {31, 32, 1000},
                                      {128, 7, 900},   {129, 7, 1000}, {334, 2, 700},  {501, 1, 600},  {1000, 1, 1000}};
  for (const auto& r : rows)
    for (int64_t T : {32 * r[0], 32 * r[0] + 31}) {
      const Geometry g = geometry_from_T(m, T);
      CHECK(g.Ts == r[0] && g.rep == r[1] && g.fw_len == r[0] * r[1] && g.out_frames == r[2],
            "T %lld: Ts %lld rep %d out_frames %lld", (long long)T, (long long)g.Ts, g.rep, (long long)g.out_frames);
    }
  for (int64_t ts = 1; ts <= 1000; ++ts) {
    const Geometry g = geometry_from_T(m, 32 * ts);
    const int64_t n = (1000 / ts) * ts, want = n == 1000 ? 1000 : (n + 99) / 100 * 100;
    CHECK(g.Ts == ts && g.rep == 1000 / ts && g.out_frames == want && g.fw_len <= g.out_frames && g.out_frames <= 1000,
          "Ts %lld", (long long)ts);
  }
  // the other models' geometry does not move
  const Geometry g9 = geometry_from_T(model_of(SEDX_MODEL_CONFORMER_FRAMEATT), 1001);
  const Geometry g14 = geometry_from_T(model_of(SEDX_MODEL_GRU14_FRAMEATT), 1001);
  CHECK(g9.Ts == 125 && g9.rep == 8 && g9.out_frames == 1000 && g14.Ts == 31 && g14.rep == 32 && g14.out_frames == 1000,
        "geometry of ids 7 and 10");
}

static void check_plan(int precision, int64_t B, int64_t T) {
  const Model m = model_of(SEDX_MODEL_CONFORMER14_FRAMEATT);
  Tuning t;
  t.precision = precision;
  ForwardPlan p;
  const char* why = plan_forward(m, t, B, T, &p);
  const int64_t T5 = T / 32;
  CHECK((why != nullptr) == (T5 < 1 || T5 > 1000), "plan_forward(B %lld, T %lld): %s", (long long)B, (long long)T,
        why ? why : "accepted");
  if (why) {
    CHECK(std::strlen(why) > 0 && std::strlen(why) < sizeof(p.reject), "the reason");
    return;
  }
  // the encoder's scratch and the logits: inside A (free once block 6 wrote the sequence input into P), pairwise
  // disjoint, at least their sizes
  const size_t M = (size_t)p.M;
  const Region* enc[7] = {&p.X, &p.Xn, &p.Hb, &p.AV, &p.Rr, &p.RK, &p.LG};
  const size_t need[7] = {M * CF_D, M * CF_D, M * CF_FF, M * CF_D, (size_t)CF_BLOCKS * T5 * CF_D,
                          (size_t)CF_BLOCKS * T5 * CF_D, M * 64};
  for (int i = 0; i < 7; ++i) {
    CHECK(inside(*enc[i], p.A) && enc[i]->floats >= need[i] && (enc[i]->off * 4) % 256 == 0, "encoder region %d", i);
    for (int j = i + 1; j < 7; ++j) CHECK(disjoint(*enc[i], *enc[j]), "encoder regions %d and %d overlap", i, j);
  }
  CHECK(p.G.floats == 0 && p.Hs.floats == 0 && p.O.floats == 0 && p.gru.floats == 0, "a GRU / MHA region");
  // the GEMM rows: the input layer's K is the trunk's width
  const auto rows = plan_gemm_launches(p, 256);
  CHECK(rows.size() == size_t(CF_BLOCKS + 1 + 8 * CF_BLOCKS + 1), "%zu GEMM rows", rows.size());
  if (rows.size() > CF_BLOCKS)
    CHECK(rows[CF_BLOCKS].K == 2048 && rows[CF_BLOCKS].N == CF_D && rows[CF_BLOCKS].M == p.M &&
              rows[0].M == T5 && rows.back().stage == 10 && rows.back().K == CF_D && rows.back().N == 64,
          "the input layer's row");
}

static void check_keys() {
  const Model m19 = model_of(SEDX_MODEL_CONFORMER14_FRAMEATT), m7 = model_of(SEDX_MODEL_CONFORMER_FRAMEATT);
  const auto e19 = expected_params(m19), e7 = expected_params(m7);
  const std::string in = "encoder.input_layer.0.weight";
  CHECK(e19.at(in) == (std::vector<int64_t>{144, 2048}) && e7.at(in) == (std::vector<int64_t>{144, 512}),
        "the input layer's shape");
  CHECK(e19.at("conv_block6.conv2.weight") == (std::vector<int64_t>{2048, 2048, 3, 3}) && !e7.count("conv_block5.conv1.weight"),
        "the trunk's keys");
  CHECK(e19.at("att_block.att.weight") == (std::vector<int64_t>{25, 144, 1}) && e19.at("att_block.bn_att.running_var") ==
            (std::vector<int64_t>{25}) && e19.at("encoder.input_layer.4.pe") == (std::vector<int64_t>{1, CF_MAX_T, 144}),
        "the head's keys");
  // every encoder key but the input weight has the 9-layer model's shape
  size_t enc = 0;
  for (const auto& kv : e7)
    if (kv.first.compare(0, 8, "encoder.") == 0 && kv.first != in) {
      ++enc;
      CHECK(e19.count(kv.first) && e19.at(kv.first) == kv.second, "%s", kv.first.c_str());
    }
  CHECK(enc == 4 + 3 * 34, "%zu encoder keys", enc);
  // 3 frontend + 4 bn0 + 6 x (2 conv + 8 bn) + 8 att_block + the encoder's 5 + 3 x 34
  CHECK(e19.size() == size_t(3 + 4 + 60 + 8 + 5 + 3 * 34), "%zu keys", e19.size());
  // the ignored keys: at their reference shapes only on id 19; whatever the shape on id 7
  struct Case { const char* key; std::vector<int64_t> shape; bool ok; };
  const Case cases[] = {{"classifier.weight", {25, 144}, true},  {"classifier.weight", {10, 144}, true},
                        {"classifier.weight", {25, 512}, false}, {"classifier.weight", {144}, false},
                        {"classifier.bias", {10}, true},         {"classifier.bias", {10, 1}, false},
                        {"linear_emb.weight", {2048, 1}, true},  {"linear_emb.weight", {512, 1}, false},
                        {"linear_emb.bias", {2048}, true},       {"linear_emb.bias", {512}, false}};
  for (const Case& c : cases) {
    CHECK(ignored_key(m19, c.key) && ignored_key(m7, c.key), "%s is not ignored", c.key);
    CHECK(ignored_key_shape_ok(m19, c.key, c.shape) == c.ok, "%s at a %zu-d shape", c.key, c.shape.size());
    CHECK(ignored_key_shape_ok(m7, c.key, c.shape), "id 7 checks the shape of %s", c.key);
  }
  CHECK(!ignored_key(m19, "gru.weight_ih_l0") && !ignored_key(m19, "fc.weight"), "a key of another model is ignored");
}

// prepare_weights: a missing key is named; with every key the 2048-wide input layer sits in the image as it
// stands in the state_dict, next to the encoder's other tensors, and the head projection is 144 wide
static void check_prepare() {
  const Model m = model_of(SEDX_MODEL_CONFORMER14_FRAMEATT);
  Params P;
  for (const auto& kv : expected_params(m)) {
    Tensor t;
    t.shape = kv.second;
    size_t n = 1;
    for (auto d : kv.second) n *= (size_t)d;
    t.data.resize(n);
    for (size_t i = 0; i < n; ++i) t.data[i] = 0.001f * (float)((i * 7 + kv.first.size()) % 1000) - 0.5f;
    P[kv.first] = std::move(t);
  }
  auto& wr = P["spectrogram_extractor.stft.conv_real.weight"].data;
  auto& wi = P["spectrogram_extractor.stft.conv_imag.weight"].data;
  for (int k = 0; k < 257; ++k)
    for (int n = 0; n < 512; ++n) {
      const double ang = -2.0 * M_PI * (double)((int64_t)n * k % 512) / 512;
      wr[(size_t)k * 512 + n] = (float)std::cos(ang), wi[(size_t)k * 512 + n] = (float)std::sin(ang);
    }
  for (auto& kv : P)
    if (kv.first.size() > 12 && kv.first.compare(kv.first.size() - 12, 12, ".running_var") == 0)
      for (auto& v : kv.second.data) v = 2.0f;
  DevWeights W;
  WeightBlob blob;
  GammaGeom gg;
  std::string err;
  {
    Tensor kept = std::move(P["encoder.input_layer.0.weight"]);
    P.erase("encoder.input_layer.0.weight");
    CHECK(prepare_weights(m, P, &W, &blob, &gg, &err) == SEDX_EKEY && err.find("encoder.input_layer.0.weight") != std::string::npos,
          "a missing key is not named: %s", err.c_str());
    P["encoder.input_layer.0.weight"] = std::move(kept);
  }
  const sedx_status st = prepare_weights(m, P, &W, &blob, &gg, &err);
  CHECK(st == SEDX_OK, "prepare_weights: %s", err.c_str());
  if (st != SEDX_OK) return;
  blob.bind(blob.image.data());   // host addresses: read the image as the device would
  const char* lo = blob.image.data();
  const char* hi = lo + blob.image.size();
  auto in_image = [&](const void* p, size_t bytes) { return p && (const char*)p >= lo && (const char*)p + bytes <= hi; };
  const auto& w = P["encoder.input_layer.0.weight"].data;
  CHECK(w.size() == (size_t)144 * 2048 && in_image(W.cf_in_w, w.size() * 4), "the input layer's slot");
  if (in_image(W.cf_in_w, w.size() * 4))
    CHECK(std::memcmp(W.cf_in_w, w.data(), w.size() * 4) == 0, "the input layer's weights are not the state_dict's");
  // the region that holds it is exactly its size (the next region starts at the next 256-byte boundary)
  for (const auto& r : blob.regions)
    if (*r.dst == (void*)W.cf_in_w) CHECK(r.bytes == w.size() * 4 && r.off % 256 == 0, "the input layer's region");
  CHECK(in_image(W.cf_in_b, 144 * 4) && in_image(W.cf_pe, (size_t)CF_MAX_T * 144 * 4) && in_image(W.cf_inv_freq, 3 * 72 * 4) &&
            in_image(W.cf[2].norm_be, 144 * 4) && in_image(W.cf[0].dw_wt, 7 * 144 * 4),
        "the encoder's slots");
  // the head projection [64][144]: att rows, cla rows, zero rows
  CHECK(in_image(W.wac, (size_t)64 * 144 * 4) && in_image(W.bac, 64 * 4) && !W.wac_x3, "the head's slots");
  if (in_image(W.wac, (size_t)64 * 144 * 4)) {
    const auto& wa = P["att_block.att.weight"].data;
    const auto& wc = P["att_block.cla.weight"].data;
    bool zero = true;
    for (size_t i = (size_t)50 * 144; i < (size_t)64 * 144; ++i) zero = zero && W.wac[i] == 0.0f;
    CHECK(std::memcmp(W.wac, wa.data(), wa.size() * 4) == 0 && std::memcmp(W.wac + 25 * 144, wc.data(), wc.size() * 4) == 0 && zero,
          "the head projection's rows");
  }
  // the deep pack behind wp[7] / cb[7], no GRU / MultiHead tensors
  CHECK(in_image(W.wp[7], deep_w_off(DEEP_LAYERS) * 4) && in_image(W.cb[7], deep_b_off(DEEP_LAYERS) * 4) && !W.w_ih && !W.whh &&
            !W.wqkv && !W.wfc && !W.w_ih_x3 && !W.wqkv_x3,
        "the trunk's deep pack / a sequence layer of another model");
}

int main() {
  check_geometry();
  const int precisions[3] = {SEDX_PRECISION_WINOGRAD, SEDX_PRECISION_EXACT, SEDX_PRECISION_X3};
  // T = 31 and 32, T5 = 1000 and 1001, the table's rows between them
  const int64_t shapes[10][2] = {{2, 31},   {1, 32},    {3, 112},    {33, 64},    {32, 1001},
                                 {1, 4127}, {2, 16032}, {1, 32000}, {1, 32031}, {1, 32032}};
  for (int pr : precisions)
    for (const auto& s : shapes) check_plan(pr, s[0], s[1]);
  check_keys();
  check_prepare();
  return host_check::finish("conformer14_driver");
}
