// The host's plan of one forward: its geometry, which kernel runs each conv
// layer and the recurrence, and where everything lives in the workspace.
// api.cpp launches from it and sizes the workspace by it, so what a forward
// writes and what sedx_workspace_size asks for cannot drift apart.  Also what
// a Winograd conv launch looks like (plan_conv_launch: the launchers ask it), which
// kernel an fp32 GEMM launch runs (plan_linear_launch), the windowed drivers' loop, merge plan (windows.cpp) and device-area layout.
// Plain C++: no HIP header, so the plans build and run without a GPU
// (tests/native/asan_driver.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/sedx.h"
#include "weights.h"

namespace sedx {

// every workspace region starts on a 256-byte boundary
constexpr size_t align256(size_t bytes) { return (bytes + 255) & ~size_t(255); }
// the one carve: `bytes` at the aligned end of what was carved so far
inline size_t carve(size_t& end, size_t bytes) {
  const size_t at = end;
  end = at + align256(bytes);
  return at;
}

// ---- launch contracts the plan shares with the kernels ----------------------
// EPI_MAXPOOL2 / EPI_MAXPOOL2_FMEAN: the VGGish trunk's max_pool2d(2x2) (floor on an odd T), the second followed by
// the mean of the 4 pooled bins at F = 8 (conv.hip; the exact fp32 kernel only)
enum ConvEpi { EPI_STORE = 0, EPI_POOL2 = 1, EPI_FMEAN = 2, EPI_MAXPOOL2 = 3, EPI_MAXPOOL2_FMEAN = 4 };
constexpr int CONV_SCHED_INTS = 256;   // per conv launch: 8 tile-claim counters, 128 B apart
// the zero-bordered bn0 output [B][T+2][66] (launch_pad_x0)
constexpr size_t block1_pad_floats(int B, int T) { return (size_t)B * (T + 2) * 66; }
// launch_gru_coop's scratch: the 256-byte aligned sync block (gru.hip asserts
// its size), then the exchange space of 8 pairs x 2 parities x 32 x 256 floats
constexpr size_t gru_coop_workspace_bytes(int /*B*/) { return 10240 + (size_t)8 * 2 * 32 * 256 * 4; }

// ---- geometry ---------------------------------------------------------------
// Ts: the sequence's frames (T3 on the 9-layer trunk, T5 on the 14-layer one); rep: frames per sequence frame
struct Geometry {
  int64_t T, T1, T2, T3, fw_len, out_frames;
  int64_t T4 = 0, T5 = 0, Ts = 0;
  int rep = 8;
};
inline int64_t conv_T(const Model& m, int64_t L) { return L / m.cfg.hop_size + 1; }
// the frames the model's own frontend makes of L samples: conv_T (log-mel), or fft_gtgram's un-centred
// 1 + (L - nfft) / hop on a gamma model (<= 0: L is shorter than the gammatone FFT)
int64_t audio_T(const Model& m, int64_t L);
// nullptr, or why no frontend runs L samples ("input of ... samples is too short for ..."; into buf)
const char* audio_refusal(const Model& m, int64_t L, char* buf, size_t n);
// the model's frame rule (Model::frames, weights.h) applied to T frames; it answers for shapes no forward runs too
Geometry geometry_from_T(const Model& m, int64_t T);
// The one rule of which shapes a model refuses, by its frame rule: nullptr, or why no forward runs T frames
// (written into buf; fits ForwardPlan::reject).  Too few frames for the trunk's pools (the reference's pool
// raises); T - 1 frames at a multiple of 32 (the reference pads by -1 frames and raises); more sequence frames
// than max_seq (the Conformer encoder's positional add does not broadcast, embedding.py:30; x12 passes the
// 1000 output frames and the pad count is negative; 1000 // seq_len is 0 and the reference returns an empty
// framewise tensor).  plan_forward, the size queries (api.cpp query_geometry) and window_geometry all ask it.
const char* shape_refusal(const Model& m, int64_t T, char* buf, size_t n);

// ---- what the handle's setters store ----------------------------------------
struct Tuning {
  int precision = SEDX_PRECISION_WINOGRAD;   // GEMM arithmetic (sedx_set_precision; the default is fp32 Winograd)
  int gru_kernel = SEDX_GRU_KERNEL_AUTO;     // sedx_set_tuning
  int gru_handoff = SEDX_GRU_HANDOFF_AUTO;
  int wino_block1 = 2;                       // SEDX_TUNE_WINO_BLOCK1 (2: conv1 inside the Winograd launch)
  int wino_f43 = 2;                          // SEDX_TUNE_WINO_F43 (2: blocks 1-4 as F(4x4,3x3), 1: blocks 2-4)
  int wino_order = 1;                        // SEDX_TUNE_WINO_ORDER (4 x 8 rounds on the 512-channel layers;
                                             // 3: as 1 with block 1's chunk-of-4 conv1 + conv2 pair)
  int mel_mfma = 0;                          // SEDX_TUNE_MEL_MFMA (measured slower: opt-in)
  int gamma_spec = 0;                        // SEDX_TUNE_GAMMA_SPEC
  int gru_spin = 1 << 24;                    // SEDX_TUNE_GRU_SPIN: bound of every GRU hand-off spin (polls)
  int cf_attn = 2;                           // SEDX_TUNE_CF_ATTN (2: per model, plan_forward)
  // sedx_set_pipelined: conv stacks of successive forwards run in issue order
  // (each waits for the previous one's conv-done event), whatever streams
  // they are issued on, so the sequence + head of batch i overlap the conv
  // stack of batch i+1 instead of two conv stacks sharing the chip
  bool pipelined = false;
  bool pipe_conv1_first = false;             // sedx_set_pipelined(h, 2): block 1's first launch before the wait
};

// ---- the plan ---------------------------------------------------------------
struct Region {
  size_t off = 0, floats = 0;   // floats from the workspace start
};
// block 1 = a first launch into A (none for F23_FUSED, which reads X0), then the stage-2 launch
enum Block1Form {
  B1_PAD_EXACT,     // launch_pad_x0 + launch_block1_exact (exact; Winograd with SEDX_TUNE_WINO_BLOCK1 0)
  B1_PAD_X3,        // launch_pad_x0 + launch_block1_fused_x3
  B1_PAD_F16,       // launch_pad_x0 + launch_block1_fused_f16 (conv1 in fp32 inside conv2's halo staging)
  B1_F23_FUSED,     // launch_block1_wino: conv1 inside the F(2x2,3x3) launch
  B1_CONV1_F23,     // launch_conv1_nhwc + launch_conv3x3_wino
  B1_CONV1_F43,     // launch_conv1_nhwc + launch_conv3x3_wino43
  // launch_conv1_planar + launch_conv3x3_wino43 with planar_in (ForwardPlan::b1_planar, the default), or
  // launch_conv1_c4 + launch_conv3x3_wino43 in the chunk-of-4 layout (SEDX_TUNE_WINO_ORDER 3)
  B1_CONV1C4_F43,
  B1_VGG,           // launch_vgg_conv1 (conv 1 -> 64 + bias + ReLU + 2x2 max pool), then launch_conv3x3 on conv2
};
enum ConvFamily { CONV_EXACT, CONV_X3, CONV_WINO, CONV_WINO43, CONV_F16 };   // layers 2-7
constexpr int MAX_CONV_LAYERS = 11;   // conv launches after block 1's first: 7, or 11 on the 14-layer trunk
struct ConvLayer {
  int T, F, cin, cout, epi;
  int To, Fo;       // the output's rows and columns ([B][To][Fo][cout]; EPI_FMEAN: Fo = 1)
  size_t in, out;   // float offsets in the workspace
  int order;        // a Winograd launch's round order: SEDX_TUNE_WINO_ORDER (0 for block 1's F(2x2) conv2)
};
// One GEMM launch of the sequence layer (stage 9) or the head projection (stage 10).  plan_forward lists them in
// launch order; run_body (api.cpp) takes M, K, N and act of each launch from the next row and supplies the
// pointers, and sedx_gemm_launch_plan reports the same rows.
enum GemmLauncher { GEMM_BY_LINEAR, GEMM_BY_X3, GEMM_BY_CF };   // launch_linear, launch_linear_x3, launch_cf_gemm
struct GemmLaunch {
  int kernel = 0, grid_x = 0, grid_y = 0, threads = 0;   // kernel: GemmKernel (below)
};
struct GemmRow {
  int stage, M, K, N, act, launcher;
  GemmLaunch l;   // filled by plan_gemm_launches
};
constexpr int MAX_GEMM_ROWS = 32;   // the Conformer models: 3 r_net + input + 3 x 8 + head = 29
struct ForwardPlan {
  Geometry g{};
  int64_t B = 0;
  int M = 0;                       // B * Ts: rows of the sequence / head GEMMs
  // conv launches after block 1's first: 7 (the VGGish trunk's: 5, conv2 .. conv4_2, all launch_conv3x3 in
  // every precision mode, after launch_vgg_conv1); the 14-layer trunk's 11, of which
  // layers[first_deep ..] run launch_conv3x3_deep (fp32 in every mode; block
  // 4's conv2 reads block 4 conv1's layout, then NHWC)
  int nlayers = 7, first_deep = 7;
  Block1Form block1 = B1_PAD_EXACT;
  ConvFamily family = CONV_EXACT;
  // winograd with F(4x4,3x3): block 1 and blocks 2-4 keep their activations
  // in the chunk-of-4 layout [B][C/4][T][F][4] (dense halo DMA)
  bool c4 = false;
  // B1_CONV1C4_F43: conv1's activation channel-planar [B][64][T][64] in A (the same bytes as the
  // chunk-of-4 one), staged by block 1's conv2 with one 16-byte LDS-DMA per wave per step
  bool b1_planar = false;
  // claim counters zeroed once per forward and passed to the conv launches:
  // always in x3; F(4x4,3x3) from 8 clips (below: the static item order, same
  // outputs, and no memset: one fill launch less on the one-clip latency path)
  bool claims = false;
  ConvLayer layers[MAX_CONV_LAYERS] = {};   // stages 2-8 (and the 14-layer trunk's blocks 5-6)
  // launch_gru_coop's variant (-1: launch_gru, SEDX_GRU_KERNEL_SIMPLE), allow_fast, spread
  int gru_variant = 2;
  bool gru_fast = false, gru_spread = false;
  Region x0, A, P, sched;          // bn0 output, the two activation buffers, 7 x CONV_SCHED_INTS counters
  // inside A once the conv stack is done: G/QKV [M][1536], H [M][512], O
  // [M][512], the logits [M][nac] and the cooperative recurrence's scratch
  // (14-layer: G [M][6144] or QKV [M][1536], H [M][2048], O [M][512], no scratch) ...
  Region G, Hs, O, LG, gru;
  // ... or the Conformer encoder's x [M][144], LayerNorm(x), the hidden [M][576],
  // the attention / depthwise output, r and r_k [3][Ts][144] (and LG)
  Region X, Xn, Hb, AV, Rr, RK;
  Region Tok;                      // Cnn_9layers_Conformer: the token buffer [M][512] (capture 8), ahead of X
  bool attn_mx = false;            // the encoder's attention: launch_cf_relattn_mx (SEDX_TUNE_CF_ATTN)
  GemmRow gemms[MAX_GEMM_ROWS] = {};   // the sequence layer's and the head's GEMM launches, in launch order
  int ngemms = 0;
  size_t total_bytes = 0;
  char reject[96] = {};            // plan_forward's reason
};
// The plan of B items of T frames.  Always filled (the size queries answer for
// shapes no forward runs); returns why a forward rejects the shape, else nullptr.
const char* plan_forward(const Model& m, const Tuning& t, int64_t B, int64_t T, ForwardPlan* p);

// a forward from audio (sedx_forward_audio): the model workspace of B items of audio_T(L) frames, then, on a
// gamma model, the frontend's regions (gamma_layout's mag / db / mm for B items of L samples) at fe.  A log-mel
// model has no such regions (fe_bytes 0).  frontend_bytes: those regions' size for `items` items (0: log-mel)
struct AudioLayout {
  size_t model_bytes = 0, fe = 0, fe_bytes = 0, total_bytes = 0;   // fe: bytes from the workspace start
};
size_t frontend_bytes(const Model& m, int64_t items, int64_t L);
AudioLayout audio_layout(const Model& m, const Tuning& t, int64_t B, int64_t L);

// ---- one Winograd conv launch -----------------------------------------------
// What launch_conv3x3_wino, launch_block1_wino and launch_conv3x3_wino43
// launch for a layer: the item shape, the persistent grid, the item order and
// the split of a batch into launches of whole clips.  Every shape performs
// the same operations in the same order per (tile, channel), so none of this
// changes an output.  No device: sedx_conv_launch_plan answers for any CU count.
enum WinoFamily { WINO_F23 = SEDX_CONV_F23, WINO_F23_BLOCK1 = SEDX_CONV_F23_BLOCK1, WINO_F43 = SEDX_CONV_F43 };
struct ConvLaunch {
  const char* reject = nullptr;   // why no launch runs this shape (hipErrorInvalidValue), else nullptr
  // 32-bit offsets in the kernels: a batch runs as launches of at most
  // clips_per_launch whole clips (same per-clip work); this plan is the
  // first one's, of `clips` = min(B, clips_per_launch) clips
  int64_t clips_per_launch = 0, in_clip = 0, out_clip = 0;   // in, out: floats per clip
  int clips = 0, nitems = 0, nwg = 0;   // items (padded to the XCD decode), persistent workgroups
  // the item: TG tile groups x NT channel tiles.  F(2x2): groups of 32 tiles,
  // tiles of 32 channels; F(4x4): groups of 16 tiles, NT 4 (64 channels) or 1 (16)
  int TG = 0, NT = 0;
  int tb_per_clip = 0, ngroups = 0;   // tile blocks of a clip, channel groups
  bool claim = false;                 // F(4x4): workgroups claim items from the counters
  int order2d = 0;                    // channel groups per L2 round (0: tile block major; -1: block 1's contiguous order)
};
// order: SEDX_TUNE_WINO_ORDER; nt_force: launch_conv3x3_wino43's; sched:
// claim counters were passed.  F(2x2) block 1 takes only B, T and c4.
ConvLaunch plan_conv_launch(WinoFamily family, int ncu, int64_t B, int T, int F, int Cin, int Cout, int epi, int order,
                            bool c4, int nt_force, bool sched);
// the Winograd launcher of stage 2 + i of a forward plan; false: the exact or
// x3 launchers run it (they keep their own shape choice)
bool conv_launch_family(const ForwardPlan& p, int i, WinoFamily* family);

// ---- one fp32 GEMM launch (seq.hip launch_linear) ----------------------------
// Which of launch_linear's kernels runs C [M][N] = act(A [M][K] W^T + b) and on
// what grid.  Every kernel chains an output's k in ascending pairs from zero
// (the K-split one per K quarter), so the choice between the tiled and the
// one-wave kernel changes no output bit; the K-split kernel takes the head
// projection at every M.  No device: sedx_gemm_launch_plan answers for any CU count.
enum GemmKernel {
  GEMM_TILED = SEDX_GEMM_TILED,         // linear_kernel: 128 x 64 tiles, 256 threads
  GEMM_ONE_WAVE = SEDX_GEMM_ONE_WAVE,   // linear_small_kernel<act, 1>: 32 x 32 tiles, one wave
  GEMM_KSPLIT = SEDX_GEMM_KSPLIT,       // linear_small_kernel<0, 4>: 32 x 32 tiles, four waves on K quarters
  GEMM_X3 = SEDX_GEMM_X3,               // launch_linear_x3 and launch_cf_gemm keep their own shape choice:
  GEMM_CONFORMER = SEDX_GEMM_CONFORMER  // their rows carry the GEMM only
};
GemmLaunch plan_linear_launch(int M, int K, int N, int act, int ncu);
// sedx_gemm_launch_plan's rows: the plan's GEMM rows (ForwardPlan::gemms) with plan_linear_launch attached to
// launch_linear's
std::vector<GemmRow> plan_gemm_launches(const ForwardPlan& p, int ncu);

// ---- windowed drivers (windows.cpp) ------------------------------------------
// loop control of predict.py:297-338 / main_strong.py:786-832: the sample
// offset of every window and the samples fed to the model for it
struct WindowLoop {
  std::vector<int64_t> start, len;
};
// nullptr on success, else why the reference's loop raises / never ends
const char* window_loop(int sample_rate, int64_t L_clip, const sedx_window_spec& sp, WindowLoop* out);
// utilities.merge replayed window by window on index lists, then avg_merge's
// divisors: merged frame f = left fold, in order, of the values with packed
// ids src[off[f] .. off[f+1]) (window w, frame t -> win_base[w] + t), divided
// by div[f] when div[f] > 1.
struct MergePlan {
  int64_t N = 0;
  std::vector<int32_t> win_base;   // [n_win + 1]
  std::vector<int32_t> off;        // [N + 1]
  std::vector<int32_t> src;
  std::vector<int32_t> div;        // [N]
};
const char* build_merge_plan(const std::vector<int64_t>& frames, int64_t step, int sample_duration, bool avg,
                             MergePlan* plan);

// windows fed to the model as one batch: consecutive windows of one length
// (every predict.py window; main_strong's full windows, then each window
// that runs past the 10 s padded clip on its own)
struct WinGroup {
  int w0 = 0, nw = 0;
  int64_t len = 0;
  Geometry g{};
};
struct WinGeom {
  WindowLoop loop;
  int n_win = 0;
  int64_t full_len = 0;     // samples of a full window (sample_duration * sr)
  int64_t clip_len = 0;     // samples backing each clip (beyond: pad_truncate zeros)
  int64_t step = 0;         // int(100 * overlap_value)
  int sd = 0;
  std::vector<WinGroup> groups;
  MergePlan plan;
  char reject[128] = {};    // window_geometry's reason
};
// nullptr, or why the spec / clip length is refused (SEDX_EINVAL)
const char* window_geometry(const Model& m, int64_t L_clip, const sedx_window_spec* spec, bool avg, WinGeom* wg);

// per-call device area after the model workspace: per-window framewise and
// clipwise outputs, vote thresholds, then the tables (window starts, output
// bases, merge plan), all at 256-B aligned offsets
struct WinLayout {
  size_t model_bytes = 0;                 // max over the groups' plans
  std::vector<size_t> fw_off, clip_off;   // per group, floats from the area start
  size_t vthr = 0, tables = 0, table_bytes = 0, total_bytes = 0;
  // a gamma model's frontend regions (gamma_layout for the largest group's items), bytes from the area start,
  // between the vote thresholds and the tables; a log-mel model has none (fe_bytes 0: the layout as it was)
  size_t fe = 0, fe_bytes = 0;
  size_t t_start = 0, t_wb = 0, t_wcs = 0, t_off = 0, t_src = 0, t_div = 0;   // byte offsets in the tables
};
WinLayout win_layout(const Model& m, const Tuning& t, int64_t n_clips, const WinGeom& wg);

// ---- ragged windowed driver (predict.py's directory loop) ----------------------
// Clips of different lengths in one call.  Every clip follows window_geometry
// for its own length and duration (the predict driver: every window is
// pad_truncate'd to full_len samples, so all items share one Geometry); the
// windows of all clips form one item list, clip by clip in window order, and
// one MergePlan per DISTINCT window count serves every clip with that count.
struct RaggedGeom {
  int64_t full_len = 0;              // samples of a window
  Geometry g{};                      // of every item
  std::vector<int64_t> clip_len;     // [n_clips]
  std::vector<int32_t> n_win;        // [n_clips]
  std::vector<int32_t> plan_of;      // [n_clips] index into plans
  std::vector<int64_t> item_off;     // [n_clips + 1] first item of clip c
  std::vector<int64_t> frame_off;    // [n_clips + 1] first merged frame of clip c
  std::vector<int64_t> win_start;    // [items] sample offset of the item inside its clip
  std::vector<MergePlan> plans;
  char reject[192] = {};
};
// nullptr, or why the call is refused (SEDX_EINVAL; a refused clip is named by index).  dur: nullptr or
// [n_clips] loop bounds in seconds (<= 0: the clip's own length)
const char* ragged_geometry(const Model& m, const int64_t* clip_len, int64_t n_clips, const sedx_window_spec* spec,
                            const double* dur, RaggedGeom* rg);

// the item table row of the log-mel frontend (FrontendParams::item_tab): where the item's samples start in the
// audio buffer and how many of them are backed by audio (beyond: pad_truncate zeros; <= 0: none)
struct ItemRow {
  int64_t src, avail;
};
// a clip's row of the ragged merge: merged frames [frame0, next row's frame0), items from item0, and where its
// plan's tables start in the concatenated off / src tables (div is laid out like off)
struct RaggedClipRow {
  int32_t frame0, item0, off0, src0;
};
// the device area: the model workspace of one forward of `chunk` items, every item's framewise output, the
// chunk's clipwise outputs, then the tables, 256-B aligned, built on the host and uploaded once
struct RaggedLayout {
  int64_t items = 0, chunk = 0;          // items per forward (the last forward runs the rest)
  size_t model_bytes = 0;
  size_t fw = 0, clipwise = 0;           // floats from the area start
  size_t fe = 0, fe_bytes = 0;           // a gamma model's frontend regions for `chunk` items (bytes; WinLayout::fe)
  size_t tables = 0, table_bytes = 0, total_bytes = 0;   // tables: floats from the area start
  size_t t_item = 0, t_clip = 0, t_off = 0, t_src = 0, t_div = 0;   // byte offsets in the tables
  size_t n_off = 0, n_src = 0;           // entries of the concatenated off (= div) and src tables
};
RaggedLayout ragged_layout(const Model& m, const Tuning& t, const RaggedGeom& rg, int64_t items_per_forward);
// the tables' image (table_bytes).  clip_off [n_clips + 1]: the clips' sample offsets in the audio buffer
void ragged_tables(const RaggedGeom& rg, const RaggedLayout& l, const int64_t* clip_off, std::vector<char>* blob);

}  // namespace sedx
