// Host side of the weight contract between the state_dict and the kernels:
// what a model expects, the device weight table and the packed layouts
// (weights.cpp, gamma_weights.cpp).  Plain C++: no HIP header, so the packing
// builds and runs without a GPU (tests/native/asan_driver.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/sedx.h"
#include "f16_geom.h"

namespace sedx {

// ---- constants shared with the kernels ------------------------------------
// logmel512_kernel: lane b of a frame's 16-lane row sums mel bands b, 31 - b,
// 32 + b, 63 - b (slots q = 0..3, balanced widths) from a zero-padded table
constexpr int FE16_MEL_MW = 36;
constexpr int FE_MT_MAX_FLOATS = 8192;    // MFMA mel table limit (32 KB of LDS)
inline int fe16_band_host(int b, int q) { return q == 0 ? b : q == 1 ? 31 - b : q == 2 ? 32 + b : 63 - b; }
// floats in the handle's device zero block (the halo DMA's source for pixels
// outside the clip; the Winograd DMA walks it by up to Cin + 4 floats)
constexpr int ZERO_BLOCK_FLOATS = 1024;
// Conformer encoder (conformer.hip)
constexpr int CF_D = 144;        // adim
constexpr int CF_FF = 576;       // eunits
constexpr int CF_BLOCKS = 3;     // elayers
constexpr int CF_MAX_T = 5000;   // rows of the positional table pe (PositionalEncoding max_len)
constexpr int MAX_CLASSES = 256;            // sedx_create's limit ...
constexpr int DECISION_MAX_CLASSES = 527;   // ... and Cnn14_DecisionLevelAtt's (AudioSet)
// 14-layer trunk: the launches of conv_deep.hip (block 4's conv2, blocks 5-6)
constexpr int DEEP_LAYERS = 5;
constexpr int DEEP_CK = 16;      // input channels per K chunk
constexpr int DEEP_BN = 128;     // output channels per workgroup (4 waves x 32)
constexpr int DEEP_CIN[DEEP_LAYERS] = {512, 512, 1024, 1024, 2048};    // b4c2, b5c1, b5c2, b6c1, b6c2
constexpr int DEEP_COUT[DEEP_LAYERS] = {512, 1024, 1024, 2048, 2048};
// float offsets of deep layer l in the handle's deep weight pack / bias block (DevWeights::wp[7], cb[7])
constexpr size_t deep_w_off(int l) { return l == 0 ? 0 : deep_w_off(l - 1) + (size_t)9 * DEEP_CIN[l - 1] * DEEP_COUT[l - 1]; }
constexpr size_t deep_b_off(int l) { return l == 0 ? 0 : deep_b_off(l - 1) + DEEP_COUT[l - 1]; }

// ---- the model ------------------------------------------------------------
// a model = the CNN trunk, then a sequence layer, then a head
enum SeqKind { SEQ_NONE = 0, SEQ_GRU = 1, SEQ_MHA = 2, SEQ_CONFORMER = 3 };
// HEAD_TOKEN: Cnn_9layers_Conformer's classifier = Linear(144, C) on every token; no sigmoid (models.py:2177-2179)
enum HeadKind { HEAD_ATT = 0, HEAD_FC_AVG = 1, HEAD_FC_MAX = 2, HEAD_TOKEN = 3 };

struct Tensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};
using Params = std::map<std::string, Tensor>;

// How T input frames become output frames (geometry_from_T and shape_refusal, plan.cpp, read nothing else of
// a model): `pools` flooring halvings give the sequence frames Ts; each is repeated `rep` times, or (rep < 0)
// 1000 // Ts times, -rep where no forward runs; `pad` repeats the last frame; no forward runs Ts > max_seq.
// `tokens` > 0 (Cnn_9layers_Conformer, models.py:2159-2164): the sequence is a learned tag token, then every
// (pooled frame, frequency bin) pixel of the trunk's `tokens` bins: Ts = tokens * T3 + 1, and the framewise
// output is one frame per pixel token, tokens * T3 of them, no repeat and no pad.
enum FramePad {
  PAD_NONE,
  PAD_TO_100,      // up to the next multiple of 100, unless the repeats give 1000 (pad_framewise_output, models.py:678-681)
  PAD_TO_T_LESS_1, // to T - 1 frames: (T % 32) - 1 copies, so a multiple of 32 has no output (models.py:2738, :2778)
  PAD_TO_1000      // always 1000 frames (models.py:2376, :2478, :2580-2582)
};
constexpr int SEQ_ANY = INT32_MAX;
struct FrameRule {
  int pools = 3, rep = 8, pad = PAD_NONE, max_seq = SEQ_ANY, tokens = 0;
};
enum Trunk { TRUNK_9 = 9, TRUNK_14 = 14, TRUNK_VGG = 6 };   // the value: Model::depth
// which launcher finishes the head projection's logits, and what d_embedding receives (api.cpp run_body)
enum HeadLaunch { HEAD_LAUNCH_ATT, HEAD_LAUNCH_ATT_REP, HEAD_LAUNCH_FC, HEAD_LAUNCH_VGG_ATT, HEAD_LAUNCH_VGG_FC, HEAD_LAUNCH_TOKEN };
enum EmbKind { EMB_NONE, EMB_CLA, EMB_HEAD_INPUT };   // nothing; cla [B][C][Ts] (models.py:683-686, :459); the head's input transposed

// what sedx_create derives from the config: one row of the model table (weights.cpp), and what follows from it
struct Model {
  sedx_config cfg{};
  int seq = SEQ_GRU;   // what follows the CNN trunk
  int head = HEAD_ATT; // the head that reads its output
  FrameRule frames;
  // ---- derived from the row ----
  int depth = 9;       // conv layers of the trunk: 9, or 14 (blocks 5-6 and five pools: T/32 sequence frames)
  int hw = 512;        // width of the head's input: 512, 144 after the Conformer encoder, 2048 on the 14-layer trunk
  int sw = 512;        // width of the sequence layer's input (the trunk's output): 512, or 2048 on the 14-layer trunk
  int nac = 64;        // rows of the head projection: att|cla (2C) or fc (C), rounded up to 64
  int head_launch = HEAD_LAUNCH_ATT;
  int emb = EMB_CLA;
  int max_classes = 256;   // MAX_CLASSES, or DECISION_MAX_CLASSES
  // Cnn14_DecisionLevelAtt: between the trunk and the head, max + avg pooling over 3 sequence frames and
  // fc1 = Linear(2048, 2048) + ReLU (decision.hip); T - 1 framewise frames, no embedding output
  bool decision = false;
  // VGGish_FrameAtt / VGGish_Gru_FrameAtt / VGGish_FrameAvg (models.py:2284-2592): the trunk is six 3x3 convs
  // with bias and ReLU, no BatchNorm (bn0 is never applied either), max pools after convs 1, 2, 4 and 6
  // (conv_vgg.hip, conv.hip's max-pool epilogues); T / 16 sequence frames, always 1000 output frames
  bool vgg = false;
  // Cnn_9layers_Conformer (models.py:2019-2189): block 4's conv2 keeps its 8 frequency bins, tokens.hip turns
  // them into the encoder's input (frames.tokens), the head is HEAD_TOKEN; no embedding output
  bool token = false;
};
// the VGGish trunk: vggish.0.<VGG_SEQ_INDEX[l]>.{weight, bias} is conv l (nn.Sequential indices of VGGish.features)
constexpr int VGG_LAYERS = 6;
constexpr int VGG_SEQ_INDEX[VGG_LAYERS] = {0, 3, 6, 8, 11, 13};
constexpr int VGG_CIN[VGG_LAYERS] = {1, 64, 128, 256, 256, 512};
constexpr int VGG_COUT[VGG_LAYERS] = {64, 128, 256, 256, 512, 512};
// cfg -> Model: the model table's row and what follows from it; false for an unknown model_type
bool make_model(const sedx_config& cfg, Model* m);
// keys of modules the Conformer models build and never call at inference
// (models.py:1290-1300, :1505-1515): accepted with any shape, not stored.  Cnn_9layers_Conformer calls both
// (classifier, linear_emb): there they are expected_params' keys and none is ignored
bool ignored_key(const Model& m, const std::string& k);
// whether an ignored key may have `shape`: Cnn_14layers_Conformer_FrameAtt takes its ignored keys (models.py:1727,
// :1735) at the reference's shapes only; the 9-layer Conformer and the VGGish models take theirs at any shape
bool ignored_key_shape_ok(const Model& m, const std::string& k, const std::vector<int64_t>& shape);
// every state_dict key the model reads, with its shape
std::map<std::string, std::vector<int64_t>> expected_params(const Model& m);

// ---- the device weight table ----------------------------------------------
// one ConformerBlock (conformer_block.py:8-24); every matrix in its
// state_dict layout [out][in]
struct CfBlockWeights {
  float* ffn_g[2] = {};    // ffn1 / ffn2: LayerNorm weight, bias [144]
  float* ffn_be[2] = {};
  float* ffn_w1[2] = {};   // [576][144]
  float* ffn_b1[2] = {};
  float* ffn_w2[2] = {};   // [144][576]
  float* ffn_b2[2] = {};
  float* att_g = nullptr;  // mhsa.layer_norm
  float* att_be = nullptr;
  float* wqkv = nullptr;   // [432][144]
  float* wo = nullptr;     // [144][144]
  float* rnet = nullptr;   // [144][144]
  float* rwb = nullptr;    // [4][36]
  float* rrb = nullptr;
  float* cv_g = nullptr;   // conv module's LayerNorm
  float* cv_be = nullptr;
  float* pw1_w = nullptr;  // [288][144]
  float* pw1_b = nullptr;
  float* dw_wt = nullptr;  // [7][144]: depthwise taps x BN scale, tap-major
  float* dw_b = nullptr;   // [144]: folded bias
  float* pw2_w = nullptr;  // [144][144]
  float* pw2_b = nullptr;
  float* norm_g = nullptr; // the block's final LayerNorm
  float* norm_be = nullptr;
};

struct DevWeights {
  float* twiddle = nullptr;   // [n_fft][2] exp(-2 pi i m / n_fft)
  float* window = nullptr;
  float* mel_w = nullptr;
  float* mel_tab = nullptr;   // logmel512_kernel's per-(slot, lane) band weights
  float* mel_mt = nullptr;    // logmel512_kernel's MFMA mel table (FrontendParams::mel_mt)
  int32_t mt_klo[4] = {}, mt_ns[4] = {}, mt_off[4] = {}, mt_floats = 0;
  int32_t mel_wmax = 0;
  int32_t* mel_off = nullptr;
  int32_t* mel_lo = nullptr;
  float* bn0_scale = nullptr;
  float* bn0_mean = nullptr;
  float* bn0_bias = nullptr;
  float* c1_w = nullptr;
  float* c1_wt = nullptr;
  float* c1_b = nullptr;
  float* zero = nullptr;   // ZERO_BLOCK_FLOATS zeros (LDS-DMA source of out-of-clip halo pixels)
  float* trash = nullptr;  // 32 KB write-only scratch (the Winograd kernel's dummy / out-of-range stores)
  float* wp[8] = {};    // packed conv weights: block k conv j -> index 2(k-1)+(j-1); [0] unused
  float* cb[8] = {};    // folded biases
  void* wx3[8] = {};    // split bf16 hi/lo packs for conv3x3_x3 (same indices)
  float* wu[8] = {};    // Winograd U = G g G^T packs for conv3x3_wino (same indices)
  float* wu43[8] = {};  // F(4x4,3x3) U packs for conv3x3_wino43 (block 1's conv2: 1, blocks 2-4: 2..7)
  // 14-layer trunk (conv_deep.hip): wp[7] holds pack_conv_deep of b4c2, b5c1, b5c2, b6c1, b6c2 back to
  // back (layer l at deep_w_off(l)) and cb[7] their folded biases (at deep_b_off(l)); block 4's conv2
  // has no other pack on such a handle and blocks 5-6 no other slot
  // VGGish trunk (Model::vgg): c1_w / c1_b hold vggish.0.0's weight [64][9] and bias as they stand, wp[l] /
  // cb[l] (l = 1..5) pack_vgg_conv of conv l and its own bias; bn0_* the identity; no x3 / Winograd packs
  float* w_ih = nullptr;   // [1536][512]; 14-layer: [6144][2048]
  float* b_ih = nullptr;   // [1536]; [6144]
  float* whhT = nullptr;   // [2][256][768] (9-layer only)
  float* whh = nullptr;    // [2][768][256] (cooperative recurrence); 14-layer: [2][3072][1024] (gru1024.hip)
  float* bhh = nullptr;    // [2][768]; [2][3072]
  float* wqkv = nullptr;   // [1536][512]; 14-layer: [1536][2048]
  float* bqkv = nullptr;
  float* wfc = nullptr;    // [512][512]; 14-layer: [2048][512]; Cnn14_DecisionLevelAtt (no MultiHead): fc1.weight
  float* bfc = nullptr;    //   as it stands [2048][2048] and fc1.bias [2048]; Cnn_9layers_Conformer (no MultiHead either):
                           //   bfc = the tag token [512], fl(linear_emb.weight[c][0] + linear_emb.bias[c]) (pack_tag_token)
  float* wac = nullptr;    // [nac][hw]
  float* bac = nullptr;
  // Conformer encoder (fp32 in every mode)
  float* cf_in_w = nullptr;      // [144][512]; on the 14-layer trunk [144][2048]
  float* cf_in_b = nullptr;
  float* cf_in_g = nullptr;      // input layer's LayerNorm
  float* cf_in_be = nullptr;
  float* cf_pe = nullptr;        // [5000][144] (the state_dict's buffer)
  float* cf_inv_freq = nullptr;  // [3][72]
  CfBlockWeights cf[CF_BLOCKS];
  // x3 (split bf16) packs of the linear weights for linear_x3.hip
  void* w_ih_x3 = nullptr;
  void* wqkv_x3 = nullptr;
  void* wfc_x3 = nullptr;
  void* wac_x3 = nullptr;
  // gamma
  double* g_twiddle = nullptr;   // [nfft][2]
  double* g_window = nullptr;
  double* g_weightsT = nullptr;  // [gamma_kp(nfft)][64] ERB weights (fft_weights)
};

// SEDX_PRECISION_F16's conv weights: pack_f16 of block k conv j at index 2(k-1)+(j-1), as DevWeights::wx3 (half
// the exact pack's bytes).  They live in the same device allocation as every other pack; a caller of
// prepare_weights that passes no F16Weights gets an image without them.
struct F16Weights {
  void* w[8] = {};
};

// The host image of the one device allocation that holds every packed weight.
// add() copies its source at once, at the next 256-byte offset, and remembers
// the pointer to set; bind() sets every such pointer once the image's device
// address is known.  No source has to outlive its add().
struct WeightBlob {
  struct Region {
    void** dst;
    size_t off, bytes;
  };
  std::vector<char> image;
  std::vector<Region> regions;
  std::vector<Region> aux;   // regions whose pointers are not DevWeights members (F16Weights); bound with the others
  template <typename D, typename T>
  void add(D** dst, const T* src, size_t n) {
    add_bytes(reinterpret_cast<void**>(dst), src, n * sizeof(T));
  }
  void add_bytes(void** dst, const void* src, size_t bytes);
  void add_aux(void** dst, const void* src, size_t bytes);
  void bind(void* device_base) const;
};

// ---- packed layouts (weights.cpp) -------------------------------------------
// wf = BN-folded weights [Cout][Cin][9] in float64 for the three conv packers
void pack_conv_exact(const double* wf, int Cin, int Cout, float* out);    // out: Cin * 9 * Cout floats
std::vector<float> pack_vgg_conv(const float* w, int Cin, int Cout);     // a VGGish conv [Cout][Cin][9] -> the exact layout
// where pack_conv_exact puts weight (o, i, tap): [Cin/4][9][khalf 2][Cout][ks 2], channel 2 ks + khalf of a chunk
inline size_t exact_pack_index(int Cout, int o, int i, int tap) {
  return ((((size_t)(i / 4) * 9 + tap) * 2 + (i & 1)) * Cout + o) * 2 + ((i % 4) >> 1);
}
void pack_conv_wino(const double* wf, int Cin, int Cout, float* U);       // U: Cin * Cout * 16 floats
void pack_conv_wino43(const double* wf, int Cin, int Cout, float* U);     // U: 2 * Cin * Cout * 36 floats
void pack_conv_deep(const double* wf, int Cin, int Cout, float* out);     // out: Cin * 9 * Cout floats
// where pack_conv_deep puts weight (o, i, tap): [Cout/32][Cin/16][9][4 q][32 n][4 c], o = 32 g + n, i = 16 chunk + 4 q + c
inline size_t deep_pack_index(int Cin, int o, int i, int tap) {
  return ((((((size_t)(o / 32) * (Cin / DEEP_CK) + i / DEEP_CK) * 9 + tap) * 4 + (i % DEEP_CK) / 4) * 32 + o % 32) * 4) + i % 4;
}
// w [N][K][taps] fp32 -> split-bf16 pack for conv_x3.hip (taps 9) and linear_x3.hip (taps 1):
// x = hi + lo + (dropped), hi = bf16(x), lo = bf16(x - hi), both round-to-nearest-even
std::vector<uint16_t> pack_x3(const float* w, int N, int K, int taps, int BN);
// w [N][K][taps] fp32 (K % 16 == 0, N % BN == 0) -> the fp16 LDS image of conv_f16.hip, N * K * taps fp16 values
// [N/BN][K/16][taps][BN][2 slots][8]: output channel o = BN nt + n, input channel i = 16 chunk + 8 c + j sits in
// record n's slot c ^ ((n >> 3) & 1) at element j (f16_geom.h: f16_pack_index), as q(w): clamped to +-65504,
// rounded to nearest even with gradual underflow, then everything below 2^-14 in magnitude set to +0 (f16_q_bits)
std::vector<uint16_t> pack_f16(const float* w, int N, int K, int taps, int BN);

void pack_head(const Model& m, const Params& P, std::vector<float>* wac, std::vector<float>* bac);   // [nac][hw], [nac]
// Cnn_9layers_Conformer's tag token [512]: linear_emb on a tensor of ones, w[c][0] * 1 + b[c] in fp32 (one rounding)
std::vector<float> pack_tag_token(const Params& P);

// gammatone tables (gamma_weights.cpp); gamma_kp: bins nfft / 2 + 1 padded to a multiple of 32
inline int gamma_kp(int nfft) { return ((nfft / 2 + 1) + 31) / 32 * 32; }
// host: ERB weights [kp][nfilts] (zero rows past nfft/2), twiddles [2 nfft], window [nfft]
// trace (tests/native/gamma_tables_driver.cpp): the intermediates of erb_space, make_erb_filters and
// fft_weights per channel (complex values as re, im pairs), for a step-by-step comparison with numpy
struct GammaTrace {
  std::vector<double> cf, ucirc, erb, B, arg, vec, common, k1, A1, gain_arg, gain, B2, r, theta, pole;
};
void gamma_tables(double fs, int nfft, int nwin, int nfilts, double fmin, std::vector<double>& weightsT,
                  int kp, std::vector<double>& twiddle, std::vector<double>& window, GammaTrace* trace = nullptr);
struct GammaGeom {
  int nfft = 0, nwin = 0, hop = 0;
};
// fft_gtgram's sizes (fftweight.py:151-152, gtgram.py:23-40) from the
// handle's sample_rate / window_size / hop_size; false: nfft not 512 / 1024 / 2048
bool gamma_geometry(int sample_rate, int window_size, int hop_size, GammaGeom* g);
// The gammatone workspace of B clips of L >= nfft samples, byte offsets from
// its base: mag [B][T][kp] f64, db [B][64][T] f64, mm [B][2] u64 (per-clip
// max / min keys).  The forward carves by it and the size query returns
// total_bytes.  T = 1 + (L - nfft) / hop columns, of which specgram's loop
// range(0, L - nfft, hop) fills the first T_fill.
struct GammaLayout {
  int64_t T = 0, T_fill = 0;
  int kp = 0;
  size_t mag_off = 0, db_off = 0, mm_off = 0, total_bytes = 0;
};
GammaLayout gamma_layout(int64_t B, int64_t L, int nfft, int hop);

// Everything sedx_finalize_weights uploads: checks that params holds every key
// of expected_params(m), fills the image, records where every pointer of *W
// goes (WeightBlob::bind sets them) and sets W's scalar fields.
// f16: where the fp16 conv packs' pointers go (blob->aux); nullptr: they are not built.
sedx_status prepare_weights(const Model& m, const Params& params, DevWeights* W, WeightBlob* blob,
                            GammaGeom* gamma, std::string* err, F16Weights* f16 = nullptr);

}  // namespace sedx
