// Host side of Cnn_9layers_Conformer (id 21) and Cnn_9layers_Gru_Reg (id 22) under AddressSanitizer + UBSan
// (make asan-token): make_model's rows, the token geometry and its refusals (T = 7, 8; 5001 tokens), the forward
// plan's workspace carving for id 21 (the token buffer and the encoder's regions at M = B (8 T3 + 1) rows, block
// 4's conv2 planned with the store epilogue), the key table, and the tag-row fold and the classifier rows in the
// weight pack, read back from the image.  No GPU, no preload.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_check.h"

using namespace sedx;

static void check_models() {
  const Model t = model_of(SEDX_MODEL_CONFORMER_TOKEN), r = model_of(SEDX_MODEL_GRU_REG);
  const Model g = model_of(SEDX_MODEL_GRU_FRAMEATT), c7 = model_of(SEDX_MODEL_CONFORMER_FRAMEATT);
  CHECK(t.depth == 9 && t.seq == SEQ_CONFORMER && t.head == HEAD_TOKEN && t.token && t.sw == 512 && t.hw == CF_D &&
            t.nac == 64 && t.emb == EMB_NONE && t.head_launch == HEAD_LAUNCH_TOKEN && t.frames.tokens == 8,
        "id 21's parts");
  CHECK(model_of(SEDX_MODEL_CONFORMER_TOKEN, 65).nac == 128 && model_of(SEDX_MODEL_CONFORMER_TOKEN, 256).nac == 256,
        "the classifier's padded width");
  CHECK(r.depth == g.depth && r.seq == g.seq && r.head == g.head && r.hw == g.hw && r.nac == g.nac && r.emb == g.emb &&
            r.head_launch == g.head_launch && !r.token && r.frames.pad == PAD_NONE && g.frames.pad == PAD_TO_100,
        "id 22 is id 0 without the pad");
  CHECK(!c7.token && c7.frames.tokens == 0 && c7.head == HEAD_ATT, "id 7 moved");
  sedx_config cfg{};
  cfg.sample_rate = 16000, cfg.window_size = 512, cfg.hop_size = 160, cfg.mel_bins = 64, cfg.classes_num = 25;
  Model m;
  for (int id : {20, 23, 9, 12, 14, 18}) {
    cfg.model_type = id;
    CHECK(!make_model(cfg, &m), "model type %d is known", id);
  }
}

static void check_geometry() {
  const Model t = model_of(SEDX_MODEL_CONFORMER_TOKEN), r = model_of(SEDX_MODEL_GRU_REG);
  char buf[96];
  for (int64_t T = 1; T <= 5100 * 8; T += (T < 1100 ? 1 : 97)) {
    const Geometry g = geometry_from_T(t, T);
    const int64_t T3 = T / 8;
    CHECK(g.T3 == T3 && g.Ts == (T3 ? 8 * T3 + 1 : 0) && g.out_frames == 8 * T3 && g.fw_len == 8 * T3 && g.rep == 1,
          "T %lld: Ts %lld out_frames %lld", (long long)T, (long long)g.Ts, (long long)g.out_frames);
    const bool refused = shape_refusal(t, T, buf, sizeof(buf)) != nullptr;
    CHECK(refused == (T < 8 || 8 * T3 + 1 > CF_MAX_T), "T %lld refusal", (long long)T);
    const Geometry gr = geometry_from_T(r, T);
    CHECK(gr.Ts == T3 && gr.out_frames == 8 * T3 && gr.rep == 8, "id 22 at T %lld", (long long)T);
  }
  // 10400, 7777, 81760 and 160000 samples at hop 160
  CHECK(geometry_from_T(t, 66).out_frames == 64 && geometry_from_T(t, 49).out_frames == 48 &&
            geometry_from_T(t, 512).out_frames == 512 && geometry_from_T(t, 1001).Ts == 1001,
        "the reference's frame counts");
  CHECK(!shape_refusal(t, 8 * 624 + 7, buf, sizeof(buf)) && shape_refusal(t, 8 * 625, buf, sizeof(buf)) &&
            std::strstr(buf, "5000"), "4993 tokens run, 5001 do not: %s", buf);
  CHECK(shape_refusal(t, 7, buf, sizeof(buf)) && std::strstr(buf, "3 pooling"), "7 frames: %s", buf);
  CHECK(geometry_from_T(model_of(SEDX_MODEL_GRU_FRAMEATT), 49).out_frames == 100, "id 0 pads 48 to 100");
}

static void check_plan(int precision, int f43, int block1, int64_t B, int64_t T) {
  const Model m = model_of(SEDX_MODEL_CONFORMER_TOKEN);
  Tuning t;
  t.precision = precision, t.wino_f43 = f43, t.wino_block1 = block1;
  ForwardPlan p;
  const char* why = plan_forward(m, t, B, T, &p);
  const int64_t T3 = T / 8, Ts = 8 * T3 + 1;
  CHECK((why != nullptr) == (T3 < 1 || Ts > CF_MAX_T), "plan_forward(B %lld, T %lld): %s", (long long)B, (long long)T,
        why ? why : "accepted");
  if (why) return;
  const size_t M = (size_t)p.M;
  CHECK(p.M == B * Ts && p.g.Ts == Ts, "M %d", p.M);
  // block 4's conv2 stores all 8 bins into P; tokens.hip reads them from there
  const ConvLayer& c = p.layers[6];
  CHECK(c.epi == EPI_STORE && c.F == 8 && c.Fo == 8 && c.To == T3 && c.cin == 512 && c.cout == 512 && c.out == p.P.off &&
            p.P.floats >= (size_t)B * T3 * 8 * 512 && p.layers[5].epi == EPI_STORE,
        "block 4's conv2");
  const Region* enc[8] = {&p.Tok, &p.X, &p.Xn, &p.Hb, &p.AV, &p.Rr, &p.RK, &p.LG};
  const size_t need[8] = {M * 512, M * CF_D, M * CF_D, M * CF_FF, M * CF_D, (size_t)CF_BLOCKS * Ts * CF_D,
                          (size_t)CF_BLOCKS * Ts * CF_D, M * 64};
  std::vector<Span> spans;
  const char* names[8] = {"Tok", "X", "Xn", "Hb", "AV", "Rr", "RK", "LG"};
  for (int i = 0; i < 8; ++i) {
    CHECK(inside(*enc[i], p.A) && enc[i]->floats >= need[i], "encoder region %s", names[i]);
    CHECK(disjoint(*enc[i], p.P), "%s overlaps P", names[i]);
    spans.push_back(span(names[i], *enc[i]));
  }
  check_spans(spans, p.A.off, p.A.off + p.A.floats, "id 21's encoder");
  CHECK(p.G.floats == 0 && p.Hs.floats == 0 && p.O.floats == 0, "a GRU / MHA region");
  CHECK((p.P.off + p.P.floats) * 4 <= p.total_bytes && (p.A.off + p.A.floats) * 4 <= p.total_bytes, "the total");
  const auto rows = plan_gemm_launches(p, 256);
  CHECK(rows.size() == size_t(CF_BLOCKS + 1 + 8 * CF_BLOCKS + 1), "%zu GEMM rows", rows.size());
  if (rows.size() > CF_BLOCKS)
    CHECK(rows[CF_BLOCKS].K == 512 && rows[CF_BLOCKS].M == p.M && rows[0].M == Ts && rows.back().stage == 10 &&
              rows.back().M == p.M && rows.back().K == CF_D && rows.back().N == 64,
          "the GEMM rows");
  // the Winograd launch plan takes the store epilogue at F = 8
  WinoFamily wf;
  if (conv_launch_family(p, 6, &wf)) {
    const ConvLaunch l = plan_conv_launch(wf, 256, B, c.T, c.F, c.cin, c.cout, c.epi, c.order, p.c4 && wf != WINO_F23, 0,
                                          p.claims && wf == WINO_F43);
    CHECK(!l.reject, "block 4's conv2: %s", l.reject ? l.reject : "");
  }
  // SEDX_TUNE_CF_ATTN: 0 the four-lane kernel, 1 the matrix-pipe one, on every Conformer model; 2 (the default):
  // the matrix-pipe kernel on id 21 alone
  ForwardPlan p7;
  CHECK(p.attn_mx, "id 21's default attention kernel");
  plan_forward(model_of(SEDX_MODEL_CONFORMER_FRAMEATT), t, B, T, &p7);
  CHECK(!p7.attn_mx, "id 7's default attention kernel");
  t.cf_attn = 0;
  plan_forward(m, t, B, T, &p);
  CHECK(!p.attn_mx, "SEDX_TUNE_CF_ATTN 0");
  t.cf_attn = 1;
  plan_forward(m, t, B, T, &p);
  CHECK(p.attn_mx, "SEDX_TUNE_CF_ATTN 1");
  plan_forward(model_of(SEDX_MODEL_CONFORMER_FRAMEATT), t, B, T, &p7);
  CHECK(p7.attn_mx && p7.Tok.floats == 0 && p7.layers[6].epi == EPI_FMEAN, "id 7's plan");
  plan_forward(model_of(SEDX_MODEL_GRU_REG), t, B, T, &p7);
  CHECK(!p7.attn_mx && p7.M == B * T3 && p7.layers[6].epi == EPI_FMEAN, "id 22's plan");
}

static void check_keys_and_pack() {
  const Model m = model_of(SEDX_MODEL_CONFORMER_TOKEN, 10), m7 = model_of(SEDX_MODEL_CONFORMER_FRAMEAVG, 10);
  const auto e = expected_params(m), e7 = expected_params(m7);
  CHECK(e.at("classifier.weight") == (std::vector<int64_t>{10, 144}) && e.at("classifier.bias") == (std::vector<int64_t>{10}) &&
            e.at("linear_emb.weight") == (std::vector<int64_t>{512, 1}) && e.at("linear_emb.bias") == (std::vector<int64_t>{512}) &&
            !e.count("fc.weight") && !e.count("att_block.att.weight") && e.size() == e7.size() + 2,
        "id 21's keys (%zu against %zu)", e.size(), e7.size());
  for (const char* k : {"classifier.weight", "classifier.bias", "linear_emb.weight", "linear_emb.bias"})
    CHECK(!ignored_key(m, k) && ignored_key(m7, k), "%s", k);
  CHECK(expected_params(model_of(SEDX_MODEL_GRU_REG)) == expected_params(model_of(SEDX_MODEL_GRU_FRAMEATT)), "id 22's keys");
  Params P;
  for (const auto& kv : e) {
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
  // values whose fp32 sum rounds: 1 + 2^-24 is a tie (to even: 1), 1 + 3 * 2^-25 rounds up to 1 + 2^-23
  auto& lw = P["linear_emb.weight"].data;
  auto& lb = P["linear_emb.bias"].data;
  lw[0] = 1.0f, lb[0] = 5.9604644775390625e-8f;
  lw[1] = 1.0f, lb[1] = 8.94069671630859375e-8f;
  DevWeights W;
  WeightBlob blob;
  GammaGeom gg;
  std::string err;
  for (const char* k : {"classifier.bias", "linear_emb.weight"}) {
    Tensor kept = std::move(P[k]);
    P.erase(k);
    CHECK(prepare_weights(m, P, &W, &blob, &gg, &err) == SEDX_EKEY && err.find(k) != std::string::npos,
          "a missing %s is not named: %s", k, err.c_str());
    P[k] = std::move(kept);
  }
  const sedx_status st = prepare_weights(m, P, &W, &blob, &gg, &err);
  CHECK(st == SEDX_OK, "prepare_weights: %s", err.c_str());
  if (st != SEDX_OK) return;
  blob.bind(blob.image.data());
  const char* lo = blob.image.data();
  const char* hi = lo + blob.image.size();
  auto in_image = [&](const void* p, size_t bytes) { return p && (const char*)p >= lo && (const char*)p + bytes <= hi; };
  CHECK(in_image(W.bfc, 512 * 4) && ((const char*)W.bfc - lo) % 256 == 0, "the tag token's slot (DevWeights::bfc)");
  if (in_image(W.bfc, 512 * 4)) {
    const std::vector<float> tag = pack_tag_token(P);
    CHECK(tag.size() == 512 && std::memcmp(W.bfc, tag.data(), 512 * 4) == 0, "the tag token in the image");
    CHECK(W.bfc[0] == 1.0f && W.bfc[1] == 1.0f + 1.1920928955078125e-7f, "the fold rounds once");
    bool same = true;
    const auto& w2 = P.at("linear_emb.weight").data;   // (the node was erased and put back above)
    const auto& b2 = P.at("linear_emb.bias").data;
    for (int c = 2; c < 512; ++c) same = same && W.bfc[c] == (float)((double)w2[c] + (double)b2[c]);
    CHECK(same, "the tag token is not fl(w + b)");
  }
  // the classifier [64][144]: 10 rows as they stand, zero rows beyond; no x3 pack of a 144-wide projection
  CHECK(in_image(W.wac, (size_t)64 * 144 * 4) && in_image(W.bac, 64 * 4) && !W.wac_x3, "the classifier's slots");
  if (in_image(W.wac, (size_t)64 * 144 * 4) && in_image(W.bac, 64 * 4)) {
    const auto& cw = P["classifier.weight"].data;
    const auto& cb = P["classifier.bias"].data;
    bool zero = true;
    for (size_t i = (size_t)10 * 144; i < (size_t)64 * 144; ++i) zero = zero && W.wac[i] == 0.0f;
    for (int i = 10; i < 64; ++i) zero = zero && W.bac[i] == 0.0f;
    CHECK(std::memcmp(W.wac, cw.data(), cw.size() * 4) == 0 && std::memcmp(W.bac, cb.data(), cb.size() * 4) == 0 && zero,
          "the classifier's rows");
  }
  CHECK(in_image(W.cf_in_w, (size_t)144 * 512 * 4) && in_image(W.cf_pe, (size_t)CF_MAX_T * 144 * 4) && in_image(W.wu43[7], 4) &&
            in_image(W.wp[7], 4) && in_image(W.wx3[7], 4) && !W.w_ih && !W.wqkv && !W.wfc,
        "the encoder's slots and block 4 conv2's packs");
  // a model without the tag token has no such slot
  DevWeights W7;
  Params P7 = P;
  P7["fc.weight"] = P["classifier.weight"], P7["fc.bias"] = P["classifier.bias"];
  CHECK(prepare_weights(m7, P7, &W7, &blob, &gg, &err) == SEDX_OK && !W7.bfc, "id 8's pack: %s", err.c_str());
}

int main() {
  check_models();
  check_geometry();
  const int64_t shapes[9][2] = {{2, 7}, {1, 8}, {3, 16}, {5, 66}, {32, 1001}, {1, 1031}, {2, 39999}, {1, 40000}, {1, 40008}};
  for (const auto& s : shapes) {
    check_plan(SEDX_PRECISION_WINOGRAD, 2, 2, s[0], s[1]);
    check_plan(SEDX_PRECISION_WINOGRAD, 1, 1, s[0], s[1]);
    check_plan(SEDX_PRECISION_WINOGRAD, 0, 2, s[0], s[1]);
    check_plan(SEDX_PRECISION_EXACT, 2, 2, s[0], s[1]);
    check_plan(SEDX_PRECISION_X3, 2, 2, s[0], s[1]);
  }
  check_keys_and_pack();
  return host_check::finish("token_driver");
}
