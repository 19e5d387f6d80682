// state_dict -> packed device weights, host arithmetic only (weights.h).
// Every layout a kernel reads is built here, beside the comment that states
// it; tests/native/asan_driver.cpp reads each pack back the way its kernel
// addresses it.
#include "weights.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace sedx {

// ---- the model --------------------------------------------------------------
// One row per model: everything the host code knows about a sedx_model follows from its row (make_model).
// Frame rules (FrameRule, weights.h): the 9-layer trunk's three pools and x8 (interpolate_ratio, models.py:741),
// the 14-layer trunk's five and x32 (:1133), the VGGish trunk's four and x12 (:2342, :2444) or x(1000 // seq_len)
// (:2578; Cnn_14layers_Conformer_FrameAtt too, :1791).  max_seq: the Conformer encoder's positional table
// (embedding.py:30 fails past it), the 1000 output frames that x12 / x(1000 // seq_len) must not pass.
namespace {
enum Stage { STAGE_NONE, STAGE_DECISION };   // between the trunk and the head
struct ModelSpec {
  int model_type, trunk, seq, head, stage;
  FrameRule frames;
};
constexpr ModelSpec MODELS[] = {
    {SEDX_MODEL_GRU_FRAMEATT, TRUNK_9, SEQ_GRU, HEAD_ATT, STAGE_NONE, {3, 8, PAD_TO_100, SEQ_ANY}},
    {SEDX_MODEL_TRANSFORMER_FRAMEATT, TRUNK_9, SEQ_MHA, HEAD_ATT, STAGE_NONE, {3, 8, PAD_NONE, SEQ_ANY}},
    {SEDX_MODEL_CNN_FRAMEMAX, TRUNK_9, SEQ_NONE, HEAD_FC_MAX, STAGE_NONE, {3, 8, PAD_NONE, SEQ_ANY}},
    {SEDX_MODEL_CNN_FRAMEAVG, TRUNK_9, SEQ_NONE, HEAD_FC_AVG, STAGE_NONE, {3, 8, PAD_NONE, SEQ_ANY}},
    {SEDX_MODEL_CNN_FRAMEATT, TRUNK_9, SEQ_NONE, HEAD_ATT, STAGE_NONE, {3, 8, PAD_NONE, SEQ_ANY}},
    {SEDX_MODEL_GRU_FRAMEAVG, TRUNK_9, SEQ_GRU, HEAD_FC_AVG, STAGE_NONE, {3, 8, PAD_NONE, SEQ_ANY}},   // the 8 T3 frames (:551)
    {SEDX_MODEL_TRANSFORMER_FRAMEAVG, TRUNK_9, SEQ_MHA, HEAD_FC_AVG, STAGE_NONE, {3, 8, PAD_NONE, SEQ_ANY}},
    {SEDX_MODEL_CONFORMER_FRAMEATT, TRUNK_9, SEQ_CONFORMER, HEAD_ATT, STAGE_NONE, {3, 8, PAD_TO_100, CF_MAX_T}},
    {SEDX_MODEL_CONFORMER_FRAMEAVG, TRUNK_9, SEQ_CONFORMER, HEAD_FC_AVG, STAGE_NONE, {3, 8, PAD_TO_100, CF_MAX_T}},
    {SEDX_MODEL_GRU14_FRAMEATT, TRUNK_14, SEQ_GRU, HEAD_ATT, STAGE_NONE, {5, 32, PAD_TO_100, SEQ_ANY}},
    {SEDX_MODEL_TRANSFORMER14_FRAMEATT, TRUNK_14, SEQ_MHA, HEAD_ATT, STAGE_NONE, {5, 32, PAD_TO_100, SEQ_ANY}},
    {SEDX_MODEL_CNN14_DECISIONLEVELATT, TRUNK_14, SEQ_NONE, HEAD_ATT, STAGE_DECISION, {5, 32, PAD_TO_T_LESS_1, SEQ_ANY}},
    {SEDX_MODEL_VGGISH_FRAMEATT, TRUNK_VGG, SEQ_NONE, HEAD_ATT, STAGE_NONE, {4, 12, PAD_TO_1000, 1000 / 12}},
    {SEDX_MODEL_VGGISH_GRU_FRAMEATT, TRUNK_VGG, SEQ_GRU, HEAD_ATT, STAGE_NONE, {4, 12, PAD_TO_1000, 1000 / 12}},
    {SEDX_MODEL_VGGISH_FRAMEAVG, TRUNK_VGG, SEQ_NONE, HEAD_FC_AVG, STAGE_NONE, {4, -1, PAD_TO_1000, 1000}},
    {SEDX_MODEL_CONFORMER14_FRAMEATT, TRUNK_14, SEQ_CONFORMER, HEAD_ATT, STAGE_NONE, {5, -32, PAD_TO_100, 1000}},
    // a tag token + 8 T3 pixel tokens, one output frame per pixel token (:2159-2189); pe holds CF_MAX_T tokens
    {SEDX_MODEL_CONFORMER_TOKEN, TRUNK_9, SEQ_CONFORMER, HEAD_TOKEN, STAGE_NONE, {3, 1, PAD_NONE, CF_MAX_T, 8}},
    {SEDX_MODEL_GRU_REG, TRUNK_9, SEQ_GRU, HEAD_ATT, STAGE_NONE, {3, 8, PAD_NONE, SEQ_ANY}},   // id 0 without the pad (:2880-2882)
};
static_assert(TRUNK_VGG == VGG_LAYERS, "Model::depth of the VGGish trunk");
}  // namespace

bool make_model(const sedx_config& cfg, Model* m) {
  const ModelSpec* row = nullptr;
  for (const ModelSpec& r : MODELS)
    if (r.model_type == cfg.model_type) row = &r;   // the table's lookup
  if (!row) return false;
  m->cfg = cfg;
  m->seq = row->seq, m->head = row->head, m->frames = row->frames;
  m->depth = row->trunk;
  m->vgg = row->trunk == TRUNK_VGG;
  m->decision = row->stage == STAGE_DECISION;
  m->token = row->head == HEAD_TOKEN;
  // the trunk's output feeds the sequence layer; the Conformer encoder narrows it to 144 for the head
  m->sw = row->trunk == TRUNK_14 ? 2048 : 512;
  m->hw = m->seq == SEQ_CONFORMER ? CF_D : m->sw;
  m->nac = (((m->head == HEAD_ATT ? 2 : 1) * cfg.classes_num + 63) / 64) * 64;
  // the heads that repeat by the frame rule have launchers of their own; the others repeat `rep` and pad
  const bool att = m->head == HEAD_ATT;
  m->head_launch = m->vgg ? (att ? HEAD_LAUNCH_VGG_ATT : HEAD_LAUNCH_VGG_FC)
                   : m->token ? HEAD_LAUNCH_TOKEN
                   : row->frames.rep < 0 ? HEAD_LAUNCH_ATT_REP : att ? HEAD_LAUNCH_ATT : HEAD_LAUNCH_FC;
  m->emb = m->decision || m->token ? EMB_NONE : att && m->seq != SEQ_MHA && m->seq != SEQ_CONFORMER ? EMB_CLA : EMB_HEAD_INPUT;
  m->max_classes = m->decision ? DECISION_MAX_CLASSES : MAX_CLASSES;   // AudioSet's 527 for Cnn14_DecisionLevelAtt alone
  return true;
}

bool ignored_key(const Model& m, const std::string& k) {
  // every VGGish class builds nn.GRU(512, 256) (models.py:2318, :2521); only VGGish_Gru_FrameAtt calls it
  if (m.vgg && m.seq != SEQ_GRU) return k.compare(0, 4, "gru.") == 0;
  if (m.seq != SEQ_CONFORMER || m.token) return false;   // Cnn_9layers_Conformer reads all four
  return k == "classifier.weight" || k == "classifier.bias" || k == "linear_emb.weight" || k == "linear_emb.bias";
}

bool ignored_key_shape_ok(const Model& m, const std::string& k, const std::vector<int64_t>& shape) {
  if (m.depth != 14 || m.seq != SEQ_CONFORMER) return true;
  // classifier = Linear(144, classes_num) at the constructor's classes_num, which the handle does not know (its
  // classes_num is the head's 25): any row count; linear_emb = Linear(1, 2048) (models.py:1727, :1735)
  if (k == "classifier.weight") return shape.size() == 2 && shape[0] >= 1 && shape[1] == CF_D;
  if (k == "classifier.bias") return shape.size() == 1 && shape[0] >= 1;
  return shape == (k == "linear_emb.weight" ? std::vector<int64_t>{m.sw, 1} : std::vector<int64_t>{m.sw});
}

namespace {

// The Conformer encoder's tensors, once: key suffix, shape, and the member
// that receives the tensor as it stands in the state_dict (nullptr: read by
// prepare_weights itself — the depthwise conv and its BatchNorm1d are folded,
// inv_freq of the three blocks is joined).  expected_params and
// prepare_weights both walk these tables; the upload order is the tables'.
template <typename Dst>
struct CfTensor {
  const char* key;
  std::vector<int64_t> shape;
  Dst dst;
};
const CfTensor<float* DevWeights::*> CF_TOP[] = {
    {"encoder.input_layer.0.weight", {CF_D, 512}, &DevWeights::cf_in_w},
    {"encoder.input_layer.0.bias", {CF_D}, &DevWeights::cf_in_b},
    {"encoder.input_layer.1.weight", {CF_D}, &DevWeights::cf_in_g},
    {"encoder.input_layer.1.bias", {CF_D}, &DevWeights::cf_in_be},
    {"encoder.input_layer.4.pe", {1, CF_MAX_T, CF_D}, &DevWeights::cf_pe},
};
// under <block>ffn1.feed_forward_module. and <block>ffn2.feed_forward_module.
const CfTensor<float* (CfBlockWeights::*)[2]> CF_FFN[] = {
    {"0.weight", {CF_D}, &CfBlockWeights::ffn_g},        {"0.bias", {CF_D}, &CfBlockWeights::ffn_be},
    {"1.weight", {CF_FF, CF_D}, &CfBlockWeights::ffn_w1}, {"1.bias", {CF_FF}, &CfBlockWeights::ffn_b1},
    {"4.weight", {CF_D, CF_FF}, &CfBlockWeights::ffn_w2}, {"4.bias", {CF_D}, &CfBlockWeights::ffn_b2},
};
// under encoder.conformer_blocks.<b>.
const CfTensor<float* CfBlockWeights::*> CF_BLOCK[] = {
    {"mhsa.layer_norm.weight", {CF_D}, &CfBlockWeights::att_g},
    {"mhsa.layer_norm.bias", {CF_D}, &CfBlockWeights::att_be},
    {"mhsa.qkv_net.weight", {3 * CF_D, CF_D}, &CfBlockWeights::wqkv},
    {"mhsa.o_net.weight", {CF_D, CF_D}, &CfBlockWeights::wo},
    {"mhsa.r_net.weight", {CF_D, CF_D}, &CfBlockWeights::rnet},
    {"mhsa.r_w_bias", {4, CF_D / 4}, &CfBlockWeights::rwb},
    {"mhsa.r_r_bias", {4, CF_D / 4}, &CfBlockWeights::rrb},
    {"conv.conv.0.weight", {CF_D}, &CfBlockWeights::cv_g},
    {"conv.conv.0.bias", {CF_D}, &CfBlockWeights::cv_be},
    {"conv.conv.1.conv.weight", {2 * CF_D, CF_D, 1}, &CfBlockWeights::pw1_w},
    {"conv.conv.1.conv.bias", {2 * CF_D}, &CfBlockWeights::pw1_b},
    {"conv.conv.8.conv.weight", {CF_D, CF_D, 1}, &CfBlockWeights::pw2_w},
    {"conv.conv.8.conv.bias", {CF_D}, &CfBlockWeights::pw2_b},
    {"norm.weight", {CF_D}, &CfBlockWeights::norm_g},
    {"norm.bias", {CF_D}, &CfBlockWeights::norm_be},
    {"mhsa.pos_emb.inv_freq", {CF_D / 2}, nullptr},
    {"conv.conv.3.conv.weight", {CF_D, 1, 7}, nullptr},
    {"conv.conv.3.conv.bias", {CF_D}, nullptr},
    {"conv.conv.5.weight", {CF_D}, nullptr},
    {"conv.conv.5.bias", {CF_D}, nullptr},
    {"conv.conv.5.running_mean", {CF_D}, nullptr},
    {"conv.conv.5.running_var", {CF_D}, nullptr},
};

std::string cf_block_key(int b) { return "encoder.conformer_blocks." + std::to_string(b) + "."; }
std::string cf_ffn_key(int b, int f) { return cf_block_key(b) + (f ? "ffn2" : "ffn1") + ".feed_forward_module."; }

void add_bn(std::map<std::string, std::vector<int64_t>>& e, const std::string& p, int64_t n) {
  for (const char* s : {".weight", ".bias", ".running_mean", ".running_var"}) e[p + s] = {n};
}

const int CONV_CH[7] = {1, 64, 128, 256, 512, 1024, 2048};   // blocks 5-6: the 14-layer trunk

}  // namespace

std::map<std::string, std::vector<int64_t>> expected_params(const Model& m) {
  std::map<std::string, std::vector<int64_t>> e;
  const int64_t K = m.cfg.window_size / 2 + 1;
  e["spectrogram_extractor.stft.conv_real.weight"] = {K, 1, m.cfg.window_size};
  e["spectrogram_extractor.stft.conv_imag.weight"] = {K, 1, m.cfg.window_size};
  e["logmel_extractor.melW"] = {K, m.cfg.mel_bins};
  add_bn(e, "bn0", 64);   // the VGGish models: in the state_dict, never applied (models.py:2347-2349)
  const bool deep = m.depth == 14;
  for (int l = 0; m.vgg && l < VGG_LAYERS; ++l) {
    const std::string p = "vggish.0." + std::to_string(VGG_SEQ_INDEX[l]);
    e[p + ".weight"] = {VGG_COUT[l], VGG_CIN[l], 3, 3};
    e[p + ".bias"] = {VGG_COUT[l]};
  }
  for (int k = 1; !m.vgg && k <= (deep ? 6 : 4); ++k) {
    const std::string p = "conv_block" + std::to_string(k);
    e[p + ".conv1.weight"] = {CONV_CH[k], CONV_CH[k - 1], 3, 3};
    e[p + ".conv2.weight"] = {CONV_CH[k], CONV_CH[k], 3, 3};
    add_bn(e, p + ".bn1", CONV_CH[k]);
    add_bn(e, p + ".bn2", CONV_CH[k]);
  }
  const int64_t C = m.cfg.classes_num;
  if (m.head == HEAD_ATT) {
    e["att_block.att.weight"] = {C, m.hw, 1};
    e["att_block.att.bias"] = {C};
    e["att_block.cla.weight"] = {C, m.hw, 1};
    e["att_block.cla.bias"] = {C};
    add_bn(e, "att_block.bn_att", C);   // unused in forward (models.py:161-169)
  } else if (m.head == HEAD_TOKEN) {
    e["classifier.weight"] = {C, m.hw};    // nn.Linear(144, classes_num) (models.py:2115)
    e["classifier.bias"] = {C};
    e["linear_emb.weight"] = {m.sw, 1};    // nn.Linear(1, 512) (:2123)
    e["linear_emb.bias"] = {m.sw};
  } else {
    e["fc.weight"] = {C, m.hw};         // nn.Linear(512, classes_num) (models.py:247, :332, :503, :921; 144: :1500)
    e["fc.bias"] = {C};
  }
  if (m.decision) {
    e["fc1.weight"] = {m.hw, m.hw};   // nn.Linear(2048, 2048) (models.py:2722)
    e["fc1.bias"] = {m.hw};
  }
  if (m.seq == SEQ_GRU) {
    // nn.GRU(512, 256), or nn.GRU(2048, 1024) on the 14-layer trunk (models.py:727)
    const int64_t hid = deep ? 1024 : 256;
    for (const char* s : {"", "_reverse"}) {
      e[std::string("gru.weight_ih_l0") + s] = {3 * hid, m.hw};
      e[std::string("gru.weight_hh_l0") + s] = {3 * hid, hid};
      e[std::string("gru.bias_ih_l0") + s] = {3 * hid};
      e[std::string("gru.bias_hh_l0") + s] = {3 * hid};
    }
  } else if (m.seq == SEQ_MHA) {
    // MultiHead(8, 512, 64, 64), or MultiHead(8, 2048, 64, 64) (models.py:1116-1121)
    for (const char* n : {"w_qs", "w_ks", "w_vs"}) {
      e[std::string("multihead.") + n + ".weight"] = {512, m.hw};
      e[std::string("multihead.") + n + ".bias"] = {512};
    }
    e["multihead.fc.weight"] = {m.hw, 512};
    e["multihead.fc.bias"] = {m.hw};
    e["multihead.layer_norm.weight"] = {m.hw};   // unused in forward (models.py:853-877)
    e["multihead.layer_norm.bias"] = {m.hw};
  } else if (m.seq == SEQ_CONFORMER) {
    for (const auto& t : CF_TOP) e[t.key] = t.shape;
    e[CF_TOP[0].key] = {CF_D, m.sw};   // the input Linear reads the trunk's output: (144, 2048) on the 14-layer trunk
    for (int b = 0; b < CF_BLOCKS; ++b) {
      for (int f = 0; f < 2; ++f)
        for (const auto& t : CF_FFN) e[cf_ffn_key(b, f) + t.key] = t.shape;
      for (const auto& t : CF_BLOCK) e[cf_block_key(b) + t.key] = t.shape;
    }
  }
  return e;
}

// ---- the blob -----------------------------------------------------------------
namespace {
size_t append256(std::vector<char>& image, const void* src, size_t bytes) {
  const size_t off = image.size();
  image.resize(off + ((bytes + 255) & ~size_t(255)), 0);
  if (bytes) std::memcpy(image.data() + off, src, bytes);
  return off;
}
}  // namespace

void WeightBlob::add_bytes(void** dst, const void* src, size_t bytes) {
  regions.push_back({dst, append256(image, src, bytes), bytes});
}

void WeightBlob::add_aux(void** dst, const void* src, size_t bytes) {
  aux.push_back({dst, append256(image, src, bytes), bytes});
}

void WeightBlob::bind(void* device_base) const {
  for (const Region& r : regions) *r.dst = static_cast<char*>(device_base) + r.off;
  for (const Region& r : aux) *r.dst = static_cast<char*>(device_base) + r.off;
}

// ---- frontend tables ----------------------------------------------------------
namespace {
// the FFT frontend requires conv_real/imag = Re/Im(DFT) * window (stft.py:209-217);
// row k = 0 of conv_real is the window since DFT[n, 0] = 1
double check_windowed_dft(const std::vector<float>& wr, const std::vector<float>& wi, int nfft) {
  const int K = nfft / 2 + 1;
  double maxerr = 0;
  const int rows[6] = {1, 2, K / 3, K / 2, K - 2, K - 1};
  for (int r : rows)
    for (int n = 0; n < nfft; ++n) {
      const double ang = -2.0 * M_PI * (double)((int64_t)n * r % nfft) / nfft;
      maxerr = std::max(maxerr, std::fabs(wr[(size_t)r * nfft + n] - std::cos(ang) * wr[n]));
      maxerr = std::max(maxerr, std::fabs(wi[(size_t)r * nfft + n] - std::sin(ang) * wr[n]));
    }
  return maxerr;
}

struct MelTables {
  std::vector<float> mel_w;               // the nonzero run of every band, packed
  std::vector<int32_t> mel_off, mel_lo;   // [65] offsets into mel_w, [64] first fft bin
  std::vector<float> mel_tab;             // [4][16][FE16_MEL_MW]
  int32_t mel_wmax = 0;                   // widest band rounded up to 4
  std::vector<float> mel_mt;              // n_fft 512 only
  int32_t mt_klo[4] = {}, mt_ns[4] = {}, mt_off[4] = {};
};
MelTables mel_tables(const std::vector<float>& melW, int nfft) {   // melW [nfft/2 + 1][64]
  const int K = nfft / 2 + 1;
  MelTables t;
  t.mel_off.resize(65);
  t.mel_lo.resize(64);
  for (int m = 0; m < 64; ++m) {
    int lo = -1, hi = -1;
    for (int k = 0; k < K; ++k)
      if (melW[(size_t)k * 64 + m] != 0.0f) {
        if (lo < 0) lo = k;
        hi = k;
      }
    t.mel_off[m] = (int32_t)t.mel_w.size();
    t.mel_lo[m] = lo < 0 ? 0 : lo;
    if (lo >= 0)
      for (int k = lo; k <= hi; ++k) t.mel_w.push_back(melW[(size_t)k * 64 + m]);
  }
  t.mel_off[64] = (int32_t)t.mel_w.size();
  // the n_fft 512 kernel's band table: slot q of lane b is band
  // fe16_band_host(b, q), zero-padded to FE16_MEL_MW bins
  t.mel_tab.assign((size_t)4 * 16 * FE16_MEL_MW, 0.f);
  for (int m = 0; m < 64; ++m) t.mel_wmax = std::max(t.mel_wmax, t.mel_off[m + 1] - t.mel_off[m]);
  t.mel_wmax = (t.mel_wmax + 3) & ~3;
  for (int q = 0; q < 4; ++q)
    for (int b = 0; b < 16; ++b) {
      const int m = fe16_band_host(b, q), wd = t.mel_off[m + 1] - t.mel_off[m];
      for (int e = 0; e < std::min(wd, FE16_MEL_MW); ++e)
        t.mel_tab[((size_t)q * 16 + b) * FE16_MEL_MW + e] = t.mel_w[t.mel_off[m] + e];
    }
  if (t.mel_w.empty()) t.mel_w.push_back(0.f);
  // the MFMA mel path's table (n_fft 512): per 16-band tile j the bin range
  // its bands cover, in 4-bin steps: [step][4 bins][16 bands] of melW (zero
  // outside a band, and past the last bin)
  if (nfft == 512) {
    for (int j = 0; j < 4; ++j) {
      int klo = K, khi = -1;
      for (int m = 16 * j; m < 16 * j + 16; ++m) {
        const int wd = t.mel_off[m + 1] - t.mel_off[m];
        if (wd <= 0) continue;
        klo = std::min(klo, t.mel_lo[m]);
        khi = std::max(khi, t.mel_lo[m] + wd - 1);
      }
      const int ns = khi < klo ? 0 : (khi - klo + 1 + 3) / 4;
      t.mt_klo[j] = ns ? klo : 0;
      t.mt_ns[j] = ns;
      t.mt_off[j] = (int32_t)t.mel_mt.size();
      for (int st = 0; st < ns; ++st)
        for (int kk = 0; kk < 4; ++kk)
          for (int n = 0; n < 16; ++n) {
            const int k = klo + 4 * st + kk, m = 16 * j + n;
            t.mel_mt.push_back(k < K ? melW[(size_t)k * 64 + m] : 0.f);
          }
    }
  }
  return t;
}

// eval-mode BatchNorm of prefix p: scale = weight / sqrt(var + 1e-5) in float64, mean, bias
void bn_fold(const Params& P, const std::string& p, int n, std::vector<double>& sc, std::vector<float>& mu,
             std::vector<float>& bi) {
  const auto& g = P.at(p + ".weight").data;
  const auto& b = P.at(p + ".bias").data;
  const auto& m = P.at(p + ".running_mean").data;
  const auto& v = P.at(p + ".running_var").data;
  sc.resize(n);
  mu.resize(n);
  bi.resize(n);
  for (int i = 0; i < n; ++i) {
    sc[i] = (double)g[i] / std::sqrt((double)v[i] + 1e-5);
    mu[i] = m[i];
    bi[i] = b[i];
  }
}

}  // namespace

// ---- conv / linear layouts ----------------------------------------------------
// exact direct conv (conv.hip): [Cin/4][9][khalf 2][Cout][ks 2] with channel
// 2 ks + khalf of a 4-channel chunk (the MFMA B fragments of both k-steps are
// one 8-byte LDS read)
void pack_conv_exact(const double* wf, int Cin, int Cout, float* out) {
  for (int o = 0; o < Cout; ++o)
    for (int i = 0; i < Cin; ++i)
      for (int t = 0; t < 9; ++t) {
        const int chunk = i / 4, kc = i % 4, ks = kc >> 1, kh = kc & 1;
        out[((((size_t)chunk * 9 + t) * 2 + kh) * Cout + o) * 2 + ks] = (float)wf[((size_t)o * Cin + i) * 9 + t];
      }
}

// a VGGish conv's weight [Cout][Cin][3][3] as it stands -> pack_conv_exact's layout (fp32 values unchanged)
std::vector<float> pack_vgg_conv(const float* w, int Cin, int Cout) {
  const std::vector<double> wf(w, w + (size_t)Cout * Cin * 9);
  std::vector<float> pk((size_t)Cin * 9 * Cout);
  pack_conv_exact(wf.data(), Cin, Cout, pk.data());
  return pk;
}

static void split_bf16(float x, uint16_t* hi, uint16_t* lo) {
  auto rne = [](float v) -> uint32_t {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
  };
  const uint32_t hb = rne(x), hbits = hb << 16;
  float hf;
  std::memcpy(&hf, &hbits, 4);
  *hi = (uint16_t)hb;
  *lo = (uint16_t)rne(x - hf);
}

// 3xbf16 split pack (conv_x3.hip, linear_x3.hip): w [N][K][taps] ->
// [N/BN][K/16][taps][BN][4 slots x 8 bf16]: a record holds 16 input channels
// of one output channel n, hi halves in slots 0-1 and lo halves in slots 2-3,
// slot c stored at c ^ ((n >> 2) & 3).  The linear layers are the layout with
// a single tap.
std::vector<uint16_t> pack_x3(const float* w, int N, int K, int taps, int BN) {
  std::vector<uint16_t> px((size_t)N * K * taps * 2, 0);
  for (int o = 0; o < N; ++o)
    for (int i = 0; i < K; ++i)
      for (int t = 0; t < taps; ++t) {
        const int nt = o / BN, n = o % BN, chunk = i / 16, k = i % 16, sw = (n >> 2) & 3;
        const size_t rec = ((((size_t)nt * (K / 16) + chunk) * taps + t) * BN + n) * 32;
        split_bf16(w[((size_t)o * K + i) * taps + t], &px[rec + 8 * ((k / 8) ^ sw) + (k % 8)],
                   &px[rec + 8 * ((2 + k / 8) ^ sw) + (k % 8)]);
      }
  return px;
}

// fp16 pack (conv_f16.hip): w [N][K][taps] -> q(w) as fp16 bits in the kernel's
// LDS image [N/BN][K/16][taps][BN][2 slots x 8] (f16_geom.h: f16_pack_index)
std::vector<uint16_t> pack_f16(const float* w, int N, int K, int taps, int BN) {
  std::vector<uint16_t> px((size_t)N * K * taps, 0);
  for (int o = 0; o < N; ++o)
    for (int i = 0; i < K; ++i)
      for (int t = 0; t < taps; ++t)
        px[f16_pack_index(K, taps, BN, o, i, t)] = f16_q_bits(w[((size_t)o * K + i) * taps + t]);
  return px;
}

// Winograd F(2x2,3x3) (conv_wino.hip): U = G g G^T per (input channel, output
// channel) in float64 from the BN-folded weights, rounded once to fp32, packed
// [Cin/4][16 p][2 h][Cout][2 ks] with channel 4 chunk + 2 h + ks (one 8-byte
// LDS read gives a lane both k-steps of a position).
void pack_conv_wino(const double* wf, int Cin, int Cout, float* Up) {
  static const double Gm[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  for (int o = 0; o < Cout; ++o)
    for (int i = 0; i < Cin; ++i) {
      const double* g = wf + ((size_t)o * Cin + i) * 9;
      double tmp[4][3];
      for (int a = 0; a < 4; ++a)
        for (int y = 0; y < 3; ++y) tmp[a][y] = Gm[a][0] * g[0 * 3 + y] + Gm[a][1] * g[1 * 3 + y] + Gm[a][2] * g[2 * 3 + y];
      const int chunk = i / 4, h = (i % 4) >> 1, ks = i & 1;
      for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 4; ++c) {
          const double u = tmp[a][0] * Gm[c][0] + tmp[a][1] * Gm[c][1] + tmp[a][2] * Gm[c][2];
          const int p = 4 * a + c;
          Up[((((size_t)chunk * 16 + p) * 2 + h) * Cout + o) * 2 + ks] = (float)u;
        }
    }
}

// Winograd F(4x4,3x3) (conv_wino43.hip): U = G g G^T as above, packed twice:
// [Cout/64][Cin/4][36 p][4 k][16 m][4 nt] with output channel 64 group +
// 16 nt + m and input channel 4 chunk + k (a chunk's slab is the LDS image;
// lane l = 16 k + m reads its 4 channel tiles as one 16-byte word), then the
// same values as [Cout/16][Cin/4][36 p][4 k][16 m] (16-channel items: a
// chunk's 9 KiB slab of one channel tile).  Up: 2 Cin Cout 36 floats.
void pack_conv_wino43(const double* wf, int Cin, int Cout, float* Up) {
  static const double Gm[6][3] = {{1.0 / 4, 0, 0},
                                  {-1.0 / 6, -1.0 / 6, -1.0 / 6},
                                  {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                  {1.0 / 24, 1.0 / 12, 1.0 / 6},
                                  {1.0 / 24, -1.0 / 12, 1.0 / 6},
                                  {0, 0, 1}};
  const int nch = Cin / 4;
  for (int o = 0; o < Cout; ++o)
    for (int i = 0; i < Cin; ++i) {
      const double* g = wf + ((size_t)o * Cin + i) * 9;
      double tmp[6][3];
      for (int a = 0; a < 6; ++a)
        for (int y = 0; y < 3; ++y) tmp[a][y] = Gm[a][0] * g[0 * 3 + y] + Gm[a][1] * g[1 * 3 + y] + Gm[a][2] * g[2 * 3 + y];
      const int grp = o / 64, nt = (o % 64) / 16, m = o % 16, chunk = i / 4, k = i % 4;
      for (int a = 0; a < 6; ++a)
        for (int c = 0; c < 6; ++c) {
          const double u = tmp[a][0] * Gm[c][0] + tmp[a][1] * Gm[c][1] + tmp[a][2] * Gm[c][2];
          const int p = 6 * a + c;
          Up[(((((size_t)grp * nch + chunk) * 36 + p) * 4 + k) * 16 + m) * 4 + nt] = (float)u;
          Up[(size_t)Cin * Cout * 36 + ((((size_t)(o / 16) * nch + chunk) * 36 + p) * 4 + k) * 16 + m] = (float)u;
        }
    }
}

// 14-layer trunk's direct conv (conv_deep.hip): [Cout/32][Cin/16][9][4 q][32 n][4 c]
// with output channel 32 g + n and input channel 16 chunk + 4 q + c: a wave's
// 32 output channels read one (chunk, tap, q) as 512 contiguous bytes, lane n
// its four channels as one 16-byte word (deep_pack_index, weights.h)
void pack_conv_deep(const double* wf, int Cin, int Cout, float* out) {
  for (int o = 0; o < Cout; ++o)
    for (int i = 0; i < Cin; ++i)
      for (int t = 0; t < 9; ++t) out[deep_pack_index(Cin, o, i, t)] = (float)wf[((size_t)o * Cin + i) * 9 + t];
}

// head projection [nac][hw] and its bias [nac], rows zero-padded to nac:
// att | cla (row c, row C + c), or fc, or (HEAD_TOKEN) classifier
void pack_head(const Model& m, const Params& P, std::vector<float>* wac, std::vector<float>* bac) {
  const size_t C = m.cfg.classes_num, hw = m.hw;
  wac->assign((size_t)m.nac * hw, 0.f);
  bac->assign(m.nac, 0.f);
  if (m.head != HEAD_ATT) {
    const auto& wf = P.at(m.head == HEAD_TOKEN ? "classifier.weight" : "fc.weight").data;
    const auto& bf = P.at(m.head == HEAD_TOKEN ? "classifier.bias" : "fc.bias").data;
    std::copy(wf.begin(), wf.end(), wac->begin());
    std::copy(bf.begin(), bf.end(), bac->begin());
  } else {
    const auto& wa = P.at("att_block.att.weight").data;
    const auto& ba = P.at("att_block.att.bias").data;
    const auto& wc = P.at("att_block.cla.weight").data;
    const auto& bc = P.at("att_block.cla.bias").data;
    std::copy(wa.begin(), wa.end(), wac->begin());
    std::copy(wc.begin(), wc.end(), wac->begin() + C * hw);
    std::copy(ba.begin(), ba.end(), bac->begin());
    std::copy(bc.begin(), bc.end(), bac->begin() + C);
  }
}

std::vector<float> pack_tag_token(const Params& P) {
  const auto& w = P.at("linear_emb.weight").data;   // [512][1]
  const auto& b = P.at("linear_emb.bias").data;
  std::vector<float> tag(b.size());
  for (size_t c = 0; c < tag.size(); ++c) tag[c] = w[c] + b[c];
  return tag;
}

// ---- everything ---------------------------------------------------------------
namespace {
sedx_status fail(std::string* err, sedx_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (err) *err = buf;
  return st;
}
}  // namespace

sedx_status prepare_weights(const Model& m, const Params& P, DevWeights* Wp, WeightBlob* blob, GammaGeom* gamma,
                            std::string* err, F16Weights* f16) {
  for (const auto& kv : expected_params(m))
    if (!P.count(kv.first)) return fail(err, SEDX_EKEY, "missing key in state_dict: %s", kv.first.c_str());
  auto get = [&](const std::string& k) -> const std::vector<float>& { return P.at(k).data; };
  const int nfft = m.cfg.window_size;
  const int hw = m.hw, nac = m.nac;
  DevWeights& W = *Wp;
  W = DevWeights();
  *blob = WeightBlob();
  *gamma = GammaGeom();
  {
    // the seven packed conv layers (exact, x3, F(2x2) and F(4x4) packs: 1 + 1 +
    // 16/9 + 8 times the weights) are nearly all of the image
    size_t conv = 0;
    for (int k = 1; k <= 4; ++k) conv += (size_t)CONV_CH[k] * ((k > 1 ? CONV_CH[k - 1] : 0) + CONV_CH[k]) * 9;
    blob->image.reserve(conv * 4 * 12 + (size_t(16) << 20));
  }

  // ---- frontend: twiddles, the window, mel tables, bn0 ----
  const auto& wr = get("spectrogram_extractor.stft.conv_real.weight");
  const double dft_err = check_windowed_dft(wr, get("spectrogram_extractor.stft.conv_imag.weight"), nfft);
  if (dft_err > 1e-5)
    return fail(err, SEDX_EINVAL, "STFT conv weights are not a windowed DFT (max err %.3g); "
                                  "the FFT frontend cannot reproduce them", dft_err);
  {
    std::vector<float> tw(2 * nfft);
    for (int k = 0; k < nfft; ++k) {
      tw[2 * k] = (float)std::cos(-2.0 * M_PI * k / nfft);
      tw[2 * k + 1] = (float)std::sin(-2.0 * M_PI * k / nfft);
    }
    blob->add(&W.twiddle, tw.data(), tw.size());
    blob->add(&W.window, wr.data(), (size_t)nfft);
    const MelTables mt = mel_tables(get("logmel_extractor.melW"), nfft);
    blob->add(&W.mel_w, mt.mel_w.data(), mt.mel_w.size());
    blob->add(&W.mel_tab, mt.mel_tab.data(), mt.mel_tab.size());
    if (!mt.mel_mt.empty() && mt.mel_mt.size() <= (size_t)FE_MT_MAX_FLOATS) {
      blob->add(&W.mel_mt, mt.mel_mt.data(), mt.mel_mt.size());
      std::copy(mt.mt_klo, mt.mt_klo + 4, W.mt_klo);
      std::copy(mt.mt_ns, mt.mt_ns + 4, W.mt_ns);
      std::copy(mt.mt_off, mt.mt_off + 4, W.mt_off);
      W.mt_floats = (int32_t)mt.mel_mt.size();
    }
    W.mel_wmax = mt.mel_wmax;
    blob->add(&W.mel_off, mt.mel_off.data(), mt.mel_off.size());
    blob->add(&W.mel_lo, mt.mel_lo.data(), mt.mel_lo.size());
    std::vector<double> s0;
    std::vector<float> mu0, bi0, sc0f(64);
    bn_fold(P, "bn0", 64, s0, mu0, bi0);
    for (int i = 0; i < 64; ++i) sc0f[i] = (float)s0[i];
    // the VGGish models feed the raw log-mel to the trunk: the frontend's fused multiply-add gets the identity
    if (m.vgg) sc0f.assign(64, 1.0f), mu0.assign(64, 0.0f), bi0.assign(64, 0.0f);
    blob->add(&W.bn0_scale, sc0f.data(), 64);
    blob->add(&W.bn0_mean, mu0.data(), 64);
    blob->add(&W.bn0_bias, bi0.data(), 64);
  }

  // ---- conv stack: BN folded into the weights in float64, then each layout ----
  const bool deep = m.depth == 14;
  std::vector<float> deep_w, deep_b;
  // the VGGish trunk: no BatchNorm, the convs' own biases; fp32 in every precision mode, so the exact pack
  // only.  conv1 in block 1 conv1's slots, convs 2-6 in wp[1..5] / cb[1..5]
  for (int l = 0; m.vgg && l < VGG_LAYERS; ++l) {
    const std::string p = "vggish.0." + std::to_string(VGG_SEQ_INDEX[l]);
    const auto& wt = get(p + ".weight");
    const auto& bias = get(p + ".bias");
    if (l == 0) {
      blob->add(&W.c1_w, wt.data(), wt.size());   // [64][9]
      blob->add(&W.c1_b, bias.data(), bias.size());
      const std::vector<float> zeros(std::max(ZERO_BLOCK_FLOATS, 64 * 128), 0.f);
      blob->add(&W.zero, zeros.data(), (size_t)ZERO_BLOCK_FLOATS);
      blob->add(&W.trash, zeros.data(), (size_t)64 * 128);
      continue;
    }
    const std::vector<float> pk = pack_vgg_conv(wt.data(), VGG_CIN[l], VGG_COUT[l]);
    blob->add(&W.wp[l], pk.data(), pk.size());
    blob->add(&W.cb[l], bias.data(), bias.size());
  }
  for (int k = 1; !m.vgg && k <= (deep ? 6 : 4); ++k)
    for (int j = 1; j <= 2; ++j) {
      const std::string p = "conv_block" + std::to_string(k);
      const int cin = (j == 1) ? CONV_CH[k - 1] : CONV_CH[k], cout = CONV_CH[k];
      const auto& wt = get(p + ".conv" + std::to_string(j) + ".weight");
      std::vector<double> sc;
      std::vector<float> mu, bi;
      bn_fold(P, p + ".bn" + std::to_string(j), cout, sc, mu, bi);
      std::vector<float> bias(cout);
      for (int o = 0; o < cout; ++o) bias[o] = (float)((double)bi[o] - (double)mu[o] * sc[o]);
      std::vector<double> wf((size_t)cout * cin * 9);
      for (int o = 0; o < cout; ++o)
        for (size_t q = 0; q < (size_t)cin * 9; ++q) wf[(size_t)o * cin * 9 + q] = wt[(size_t)o * cin * 9 + q] * sc[o];
      std::vector<float> wff(wf.begin(), wf.end());   // rounded once: the direct conv1 and the x3 split read it
      if (k == 1 && j == 1) {
        // block 1's conv1 (Cin 1): [64][9], and [tap][64] (channel pairs adjacent)
        std::vector<float> c1wt(9 * 64);
        for (int o = 0; o < 64; ++o)
          for (int t = 0; t < 9; ++t) c1wt[t * 64 + o] = wff[o * 9 + t];
        blob->add(&W.c1_w, wff.data(), wff.size());
        blob->add(&W.c1_wt, c1wt.data(), c1wt.size());
        blob->add(&W.c1_b, bias.data(), bias.size());
        const std::vector<float> zeros(std::max(ZERO_BLOCK_FLOATS, 64 * 128), 0.f);
        blob->add(&W.zero, zeros.data(), (size_t)ZERO_BLOCK_FLOATS);   // >= Cin + 4 floats: the Winograd halo DMA steps through it
        blob->add(&W.trash, zeros.data(), (size_t)64 * 128);
        continue;
      }
      const int idx = 2 * (k - 1) + (j - 1);
      if (deep && idx >= 7) {
        // block 4's conv2 (pooled here) and blocks 5-6: the deep pack only, fp32 in
        // every mode; the five layers back to back behind wp[7] / cb[7] (weights.h)
        const int l = idx - 7;
        if (l == 0) deep_w.assign(deep_w_off(DEEP_LAYERS), 0.f), deep_b.assign(deep_b_off(DEEP_LAYERS), 0.f);
        if (cin != DEEP_CIN[l] || cout != DEEP_COUT[l]) return fail(err, SEDX_EINVAL, "deep layer %d shape", l);
        pack_conv_deep(wf.data(), cin, cout, deep_w.data() + deep_w_off(l));
        std::copy(bias.begin(), bias.end(), deep_b.begin() + deep_b_off(l));
        if (l == DEEP_LAYERS - 1) {
          blob->add(&W.wp[7], deep_w.data(), deep_w.size());
          blob->add(&W.cb[7], deep_b.data(), deep_b.size());
          std::vector<float>().swap(deep_w);
        }
        continue;
      }
      std::vector<float> pk((size_t)cin * 9 * cout);
      pack_conv_exact(wf.data(), cin, cout, pk.data());
      blob->add(&W.wp[idx], pk.data(), pk.size());
      blob->add(&W.cb[idx], bias.data(), bias.size());
      const std::vector<uint16_t> px = pack_x3(wff.data(), cout, cin, 9, cout == 64 ? 64 : 128);
      blob->add(&W.wx3[idx], px.data(), px.size());
      if (f16) {
        const std::vector<uint16_t> ph = pack_f16(wff.data(), cout, cin, 9, cout == 64 ? 64 : 128);
        blob->add_aux(&f16->w[idx], ph.data(), ph.size() * sizeof(uint16_t));
      }
      pk.assign((size_t)cin * cout * 16, 0.f);
      pack_conv_wino(wf.data(), cin, cout, pk.data());
      blob->add(&W.wu[idx], pk.data(), pk.size());
      // block 1's conv2 and blocks 2-4: the F(4x4,3x3) pack as well
      pk.assign((size_t)2 * cin * cout * 36, 0.f);
      pack_conv_wino43(wf.data(), cin, cout, pk.data());
      blob->add(&W.wu43[idx], pk.data(), pk.size());
    }

  // ---- sequence layer ----
  std::vector<float> w_ih, wqkv;   // kept for their x3 packs, which follow the head in the image
  if (m.seq == SEQ_GRU && deep) {
    // nn.GRU(2048, 1024): both directions' W_ih stacked [6144][2048], W_hh as it stands [2][3072][1024]
    std::vector<float> b_ih, whh_nat, bhh;
    const char* sfx[2] = {"", "_reverse"};
    for (int d = 0; d < 2; ++d) {
      const auto& wih = get(std::string("gru.weight_ih_l0") + sfx[d]);
      const auto& whh = get(std::string("gru.weight_hh_l0") + sfx[d]);
      const auto& bi = get(std::string("gru.bias_ih_l0") + sfx[d]);
      const auto& bh = get(std::string("gru.bias_hh_l0") + sfx[d]);
      w_ih.insert(w_ih.end(), wih.begin(), wih.end());
      whh_nat.insert(whh_nat.end(), whh.begin(), whh.end());
      b_ih.insert(b_ih.end(), bi.begin(), bi.end());
      bhh.insert(bhh.end(), bh.begin(), bh.end());
    }
    blob->add(&W.w_ih, w_ih.data(), w_ih.size());
    blob->add(&W.b_ih, b_ih.data(), b_ih.size());
    blob->add(&W.whh, whh_nat.data(), whh_nat.size());
    blob->add(&W.bhh, bhh.data(), bhh.size());
  } else if (m.seq == SEQ_GRU) {
    std::vector<float> b_ih(1536), whhT(2 * 256 * 768), whh_nat, bhh(2 * 768);
    w_ih.resize(1536 * 512);
    const char* sfx[2] = {"", "_reverse"};
    for (int d = 0; d < 2; ++d) {
      const auto& wih = get(std::string("gru.weight_ih_l0") + sfx[d]);
      const auto& whh = get(std::string("gru.weight_hh_l0") + sfx[d]);
      const auto& bi = get(std::string("gru.bias_ih_l0") + sfx[d]);
      const auto& bh = get(std::string("gru.bias_hh_l0") + sfx[d]);
      std::copy(wih.begin(), wih.end(), w_ih.begin() + (size_t)d * 768 * 512);
      std::copy(bi.begin(), bi.end(), b_ih.begin() + d * 768);
      std::copy(bh.begin(), bh.end(), bhh.begin() + d * 768);
      for (int r = 0; r < 768; ++r)
        for (int q = 0; q < 256; ++q) whhT[((size_t)d * 256 + q) * 768 + r] = whh[(size_t)r * 256 + q];
      whh_nat.insert(whh_nat.end(), whh.begin(), whh.end());
    }
    blob->add(&W.w_ih, w_ih.data(), w_ih.size());
    blob->add(&W.b_ih, b_ih.data(), b_ih.size());
    blob->add(&W.whhT, whhT.data(), whhT.size());
    blob->add(&W.whh, whh_nat.data(), whh_nat.size());
    blob->add(&W.bhh, bhh.data(), bhh.size());
  } else if (m.seq == SEQ_MHA) {
    std::vector<float> bqkv(1536);
    wqkv.resize((size_t)1536 * hw);   // q | k | v rows, [1536][hw]
    const char* nm[3] = {"w_qs", "w_ks", "w_vs"};
    for (int i = 0; i < 3; ++i) {
      const auto& ww = get(std::string("multihead.") + nm[i] + ".weight");
      const auto& bb = get(std::string("multihead.") + nm[i] + ".bias");
      std::copy(ww.begin(), ww.end(), wqkv.begin() + (size_t)i * 512 * hw);
      std::copy(bb.begin(), bb.end(), bqkv.begin() + i * 512);
    }
    blob->add(&W.wqkv, wqkv.data(), wqkv.size());
    blob->add(&W.bqkv, bqkv.data(), bqkv.size());
    blob->add(&W.wfc, get("multihead.fc.weight").data(), (size_t)hw * 512);
    blob->add(&W.bfc, get("multihead.fc.bias").data(), (size_t)hw);
  }
  if (m.decision) {
    // fc1 as it stands (decision.hip reads row n of [2048][2048] along k), in the slots of the
    // MultiHead fc this model does not have
    blob->add(&W.wfc, get("fc1.weight").data(), (size_t)hw * hw);
    blob->add(&W.bfc, get("fc1.bias").data(), (size_t)hw);
  }

  std::vector<float> wac, bac;
  pack_head(m, P, &wac, &bac);
  blob->add(&W.wac, wac.data(), wac.size());
  blob->add(&W.bac, bac.data(), bac.size());
  if (m.token) {
    const std::vector<float> tag = pack_tag_token(P);
    blob->add(&W.bfc, tag.data(), tag.size());   // the MultiHead fc bias's slot (weights.h)
  }

  // ---- x3 packs of the linear layers ----
  auto add_x3 = [&](void** dst, const float* w, int N, int BN) {
    const std::vector<uint16_t> px = pack_x3(w, N, 512, 1, BN);
    blob->add(dst, px.data(), px.size());
  };
  if (deep) {
    // the 14-layer models' linear layers run fp32 in every mode: no x3 packs
  } else if (m.seq == SEQ_GRU) {
    add_x3(&W.w_ih_x3, w_ih.data(), 1536, 128);
  } else if (m.seq == SEQ_MHA) {
    add_x3(&W.wqkv_x3, wqkv.data(), 1536, 128);
    add_x3(&W.wfc_x3, get("multihead.fc.weight").data(), 512, 128);
  }
  if (hw == 512) add_x3(&W.wac_x3, wac.data(), nac, 64);   // the 144-wide projection runs fp32 in every mode

  // ---- Conformer encoder: the state_dict's own tensors (the tables above),
  // except the depthwise conv with its BatchNorm1d folded in (eval mode, eps 1e-5) ----
  if (m.seq == SEQ_CONFORMER) {
    auto up = [&](float** dst, const std::string& k) {
      const auto& v = get(k);
      blob->add(dst, v.data(), v.size());
    };
    for (const auto& t : CF_TOP) up(&(W.*t.dst), t.key);
    std::vector<float> inv_freq;
    for (int b = 0; b < CF_BLOCKS; ++b) {
      const std::string p = cf_block_key(b);
      CfBlockWeights& c = W.cf[b];
      for (int f = 0; f < 2; ++f)
        for (const auto& t : CF_FFN) up(&(c.*t.dst)[f], cf_ffn_key(b, f) + t.key);
      for (const auto& t : CF_BLOCK)
        if (t.dst) up(&(c.*t.dst), p + t.key);
      const auto& fr = get(p + "mhsa.pos_emb.inv_freq");
      inv_freq.insert(inv_freq.end(), fr.begin(), fr.end());
      std::vector<double> sc;
      std::vector<float> mu, bi;
      bn_fold(P, p + "conv.conv.5", CF_D, sc, mu, bi);
      const auto& dw = get(p + "conv.conv.3.conv.weight");   // [144][1][7]
      const auto& db = get(p + "conv.conv.3.conv.bias");
      std::vector<float> dw_wt(7 * CF_D), dw_b(CF_D);
      for (int ch = 0; ch < CF_D; ++ch) {
        for (int t = 0; t < 7; ++t) dw_wt[t * CF_D + ch] = (float)((double)dw[ch * 7 + t] * sc[ch]);
        dw_b[ch] = (float)(((double)db[ch] - (double)mu[ch]) * sc[ch] + (double)bi[ch]);
      }
      blob->add(&c.dw_wt, dw_wt.data(), dw_wt.size());
      blob->add(&c.dw_b, dw_b.data(), dw_b.size());
    }
    blob->add(&W.cf_inv_freq, inv_freq.data(), inv_freq.size());
  }

  // ---- gammatone tables (float64, numpy operation order: gamma_weights.cpp) ----
  if (m.cfg.feature_type == SEDX_FEATURE_GAMMA) {
    // fft_gtgram (fftweight.py:151-152) + gtgram_strides (gtgram.py:23-40)
    const double fs = m.cfg.sample_rate;
    if (!gamma_geometry(m.cfg.sample_rate, m.cfg.window_size, m.cfg.hop_size, gamma))
      return fail(err, SEDX_EINVAL, "gammatone nfft %d unsupported", gamma->nfft);
    const int nfft_g = gamma->nfft;
    std::vector<double> g_tw, g_win, g_wT;
    gamma_tables(fs, nfft_g, gamma->nwin, 64, m.cfg.fmin, g_wT, gamma_kp(nfft_g), g_tw, g_win);
    blob->add(&W.g_twiddle, g_tw.data(), g_tw.size());
    blob->add(&W.g_window, g_win.data(), g_win.size());
    blob->add(&W.g_weightsT, g_wT.data(), g_wT.size());
  }
  return SEDX_OK;
}

}  // namespace sedx
