/*
 * sedx.h — C ABI of the MI355X-native sound-event-detection inference path.
 *
 * Drop-in boundary for the reference's hot path (yazdayy/sound-event-detection,
 * read-only at /root/reference).  The reference is pure Python/PyTorch; its
 * "plugin API" for this path is the model classes instantiated by name
 * (`Model = eval(model_type)`, pytorch/predict.py:229, pytorch/main_strong.py:529)
 * with a fixed constructor, `forward()` and state_dict.  Each entry point below
 * names the reference interface it replaces.  The host-side mirror of those
 * classes (sound-event-detection_amd/sedx/models.py) binds these symbols with
 * ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - Plain pointers and sizes; no torch / HIP types.  `stream` is a
 *    hipStream_t passed as void* (NULL = the null stream).
 *  - All `d_*` pointers are device pointers on the handle's device, fp32,
 *    row-major, caller-owned.  `h_*` pointers are host memory.
 *  - Every call returns sedx_status; on failure sedx_last_error(h) holds a
 *    message (the Python shim raises RuntimeError with it), replacing the
 *    reference's Python exceptions (e.g. pytorch/models.py:139).
 *  - A handle is bound to one device and owns packed weights + a cached
 *    workspace.  Host calls on one handle must be serialised by the caller
 *    (the reference's DataParallel uses one replica per device, one thread
 *    each); the device work they issue may run concurrently on different
 *    streams when every such call passes its own d_workspace (the weights
 *    are read-only after sedx_finalize_weights).  Handles share no mutable
 *    state: calls on different handles (e.g. one per device, each from its
 *    own thread) need no coordination.
 */
#ifndef SEDX_H
#define SEDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  SEDX_OK = 0,
  SEDX_EINVAL = 1,    /* bad argument / shape                     */
  SEDX_ENOMEM = 2,    /* device allocation failed                  */
  SEDX_EHIP = 3,      /* HIP runtime error                         */
  SEDX_ESTATE = 4,    /* weights not finalised / wrong call order  */
  SEDX_EKEY = 5       /* unknown or mis-shaped state_dict key      */
} sedx_status;

typedef enum {
  SEDX_MODEL_GRU_FRAMEATT = 0,          /* Cnn_9layers_Gru_FrameAtt   pytorch/models.py:564 */
  SEDX_MODEL_TRANSFORMER_FRAMEATT = 1,  /* Cnn_9layers_Transformer_FrameAtt  :981       */
  /* the other models on the same 9-layer CNN trunk.  "fc" heads: sigmoid(fc(x))
   * per frame, x8 repeat, clipwise = max / mean over the frames */
  SEDX_MODEL_CNN_FRAMEMAX = 2,          /* Cnn_9layers_FrameMax  :213-295: trunk, fc, max      */
  SEDX_MODEL_CNN_FRAMEAVG = 3,          /* Cnn_9layers_FrameAvg  :298-380: trunk, fc, mean     */
  SEDX_MODEL_CNN_FRAMEATT = 4,          /* Cnn_9layers_FrameAtt  :383-461: trunk, AttBlock     */
  SEDX_MODEL_GRU_FRAMEAVG = 5,          /* Cnn_9layers_Gru_FrameAvg  :466-561: bi-GRU, fc, mean
                                           (no padding to a multiple of 100, :551)            */
  SEDX_MODEL_TRANSFORMER_FRAMEAVG = 6,  /* Cnn_9layers_Transformer_FrameAvg  :880-978: MultiHead, fc, mean */
  /* the same trunk, then the 3-block Conformer encoder (models_2020/conformer/:
   * ConformerEncoder(512, adim 144, aheads 4, elayers 3, eunits 576, kernel 7))
   * and a 144-wide head; framewise padded to a multiple of 100 with its last
   * frame (:1359-1360, :1571-1572).  fp32 in every precision mode. */
  SEDX_MODEL_CONFORMER_FRAMEATT = 7,    /* Cnn_9layers_Conformer_FrameAtt  :1189-1410: AttBlock(144, 25) */
  SEDX_MODEL_CONFORMER_FRAMEAVG = 8,    /* Cnn_9layers_Conformer_FrameAvg  :1412-1625: fc(144), mean over
                                           the padded frames (:1575)                                   */
  /* the 14-layer trunk: blocks 1-3 as above, block 4 pooled 2x2, block 5
   * (512 -> 1024, pooled) and block 6 (1024 -> 2048, frequency mean of its 2
   * bins): T/32 sequence frames of 2048 channels, x32 frame repeat, framewise
   * padded to a multiple of 100 with its last frame unless it has 1000 frames.
   * AttBlock(2048, 25).  feature_type must be LOGMEL.  Blocks 5-6, block 4's
   * conv2, the sequence layer and the head are fp32 in every precision mode
   * (sedx_set_precision and the Winograd knobs select the arithmetic of
   * blocks 1-3 and block 4's conv1 only). */
  /* 9 is not assigned: callers written against the nine 9-layer models probe it
   * as the first unknown model_type, and sedx_create keeps answering SEDX_EINVAL */
  SEDX_MODEL_GRU14_FRAMEATT = 10,         /* Cnn_14layers_Gru_FrameAtt  :691-791: nn.GRU(2048, 1024, bidirectional) */
  SEDX_MODEL_TRANSFORMER14_FRAMEATT = 11, /* Cnn_14layers_Transformer_FrameAtt  :1080-1184: MultiHead(8, 2048, 64, 64) */
  /* 12 is not assigned either (probed as the first unknown id after the two models above) */
  /* Cnn14_DecisionLevelAtt  :2685-2783, the PANNs architecture: the 14-layer
   * trunk, then over the T/32 sequence frames max_pool1d(3, 1, 1) +
   * avg_pool1d(3, 1, 1) (zero padding, always / 3), fc1 = Linear(2048, 2048) +
   * ReLU, AttBlock(2048, classes_num) with classes_num up to 527 (every other
   * model: 256).  feature_type must be LOGMEL.
   *   geometry   T = L / hop + 1 frames; seq_len = T / 32; out_frames = T - 1:
   *              every sequence frame x32, then the last frame repeated
   *              (T % 32) - 1 times (10 s at hop 320 / 32 kHz: 992 + 8 = 1000)
   *   refusals   T < 32 (the fifth pool has no output) and every T % 32 == 0
   *              (the reference's padding count is -1 and it raises):
   *              SEDX_EINVAL from the forwards, sedx_output_geometry,
   *              sedx_workspace_size and the windowed drivers alike
   *   keys       the 14-layer trunk's (frontend buffers, bn0, conv_block1-6),
   *              fc1.{weight [2048][2048], bias}, att_block.{att,cla}.{weight
   *              [C][2048][1], bias} and att_block.bn_att.* (accepted, unused)
   *   outputs    framewise and clipwise only: the reference returns no
   *              'embedding', d_embedding is ignored and may be NULL
   * The pooling, fc1 and the head are fp32 in every precision mode; captures:
   * 43 is the pooling's input, 9 is fc1's output [items][T/32][2048], and the
   * timed stage 9 is the one pooling + fc1 launch. */
  SEDX_MODEL_CNN14_DECISIONLEVELATT = 13,
  /* 14 is not assigned (probed as the first unknown id after 13) */
  /* The transfer-learning models on the VGGish trunk, pytorch/models.py:2219-2592.
   * The trunk is six 3x3 convs with bias and ReLU and no BatchNorm (1 -> 64 ->
   * 128 -> 256 -> 256 -> 512 -> 512) with max_pool2d(2x2) after convs 1, 2, 4
   * and 6, on the raw log-mel: bn0 is in the state_dict and never applied.  fp32
   * in every precision mode (sedx_set_precision and the Winograd knobs are
   * accepted and change nothing in it); the GRU and the head projection run as
   * on the 9-layer models.  feature_type must be LOGMEL; classes_num is the
   * head's width (the reference's head has 25 outputs whatever its constructor
   * is given, and sedx.models passes 25).
   *   geometry   T = L / hop + 1 frames; each pool floors: seq_len = T / 16;
   *              out_frames = 1000 always.  The FrameAtt models repeat every
   *              sequence frame x12, VGGish_FrameAvg x(1000 / seq_len), then the
   *              last frame is repeated up to 1000 frames; VGGish_FrameAvg's
   *              clipwise output is the mean over all 1000 padded frames.
   *   refusals   T < 16 (the fourth pool has no output); seq_len > 83 for the
   *              two FrameAtt models (the reference's padding count is negative
   *              and it raises); seq_len > 1000 for VGGish_FrameAvg (a
   *              deviation: the reference returns an empty tensor and NaN):
   *              SEDX_EINVAL from the forwards, sedx_output_geometry,
   *              sedx_workspace_size, the launch plans and the windowed drivers
   *   keys       the frontend buffers, bn0.* (accepted, unused),
   *              vggish.0.{0,3,6,8,11,13}.{weight,bias}, gru.* (read by
   *              VGGISH_GRU_FRAMEATT; accepted and unused by the other two),
   *              att_block.* or fc.{weight [C][512], bias}
   *   outputs    d_embedding: cla [B, C, seq_len] (FrameAtt models), the trunk's
   *              output [B, 512, seq_len] (VGGISH_FRAMEAVG)
   * Captures 0, 50-55, 8, 9 (sedx_set_capture); timed stages: 1 is conv1 with
   * its pool, 2-6 the launches of conv2, conv3_1, conv3_2, conv4_1 and conv4_2
   * (7 and 8 are empty), 9 the GRU, 10 the head. */
  SEDX_MODEL_VGGISH_FRAMEATT = 15,        /* VGGish_FrameAtt  :2284-2383: AttBlock(512, 25) */
  SEDX_MODEL_VGGISH_GRU_FRAMEATT = 16,    /* VGGish_Gru_FrameAtt  :2386-2485: nn.GRU(512, 256, bidirectional), AttBlock(512, 25) */
  SEDX_MODEL_VGGISH_FRAMEAVG = 17,        /* VGGish_FrameAvg  :2487-2592: Linear(512, 25), sigmoid */
  /* 18 is not assigned (probed as the first unknown id after the VGGish models) */
  /* Cnn_14layers_Conformer_FrameAtt  :1627-1801: the 14-layer trunk, then the
   * Conformer encoder of ids 7 and 8 on its T/32 sequence frames of 2048
   * channels -- ConformerEncoder(2048, adim 144, aheads 4, elayers 3, eunits
   * 576, kernel 7): only encoder.input_layer.0.weight differs, (144, 2048) --
   * and AttBlock(144, 25).  feature_type must be LOGMEL; classes_num is the
   * head's width (25 in the reference whatever its constructor is given).
   * The encoder and the head are fp32 in every precision mode.
   *   geometry   T = L / hop + 1 frames; seq_len = T / 32; every sequence
   *              frame is repeated 1000 / seq_len times (:1791-1792); unless
   *              that gives 1000 frames, the last one is repeated up to the
   *              next multiple of 100 (:1793-1794): seq_len 31 -> x32, 992 ->
   *              1000; 15 -> x66, 990 -> 1000; 128 -> x7, 896 -> 900; 129 ->
   *              x7, 903 -> 1000; 501 -> x1, 501 -> 600.  clipwise sums over
   *              the seq_len sequence frames, not the padded ones.
   *   refusals   T < 32 (the fifth pool has no output) and seq_len > 1000 (a
   *              deviation: the ratio is 0 and the reference returns an empty
   *              framewise tensor): SEDX_EINVAL from the forwards,
   *              sedx_output_geometry, sedx_workspace_size, the launch plans
   *              and the windowed drivers, before any launch
   *   keys       the 14-layer trunk's, encoder.* as ids 7 and 8 with the
   *              (144, 2048) input weight, att_block.{att,cla}.{weight
   *              [C][144][1], bias}; att_block.bn_att.*, classifier.{weight
   *              [n][144], bias [n]} and linear_emb.{weight [2048][1], bias
   *              [2048]} are shape-checked and dropped.  n is the reference
   *              constructor's classes_num, which this config does not carry
   *              (classes_num here is the head's 25): any n >= 1 is taken,
   *              and sedx.models checks n in its load_state_dict
   *   outputs    d_embedding: the encoder output [B, 144, seq_len]
   * Captures (sedx_set_capture): 0, 2..8 and 40..43 as the 14-layer models; 43
   * [items][T/32][2048] is the encoder's input; 20 and 21 + 4b + j as ids 7 and
   * 8, here [items][T/32][144]; 9 is the encoder's output [M][144], M = items x
   * T/32 (the same tensor as 32); 44 is the head's logits [M][64]: columns
   * 0..C-1 att, C..2C-1 cla, zeros beyond.  Timed stage 8 as the 14-layer
   * models, 9 the encoder, 10 the head. */
  SEDX_MODEL_CONFORMER14_FRAMEATT = 19,
  /* 20 is not assigned (probed as the first unknown id after 19) */
  /* Cnn_9layers_Conformer  :2019-2214, the DCASE-2020-style token model: the 9-layer
   * trunk with all 8 frequency bins of block 4 kept (conv_block4 is not pooled
   * and there is no frequency mean), every (frame, bin) pixel a 512-wide token
   * in (t, f) order behind one learned tag token linear_emb(ones) (:2159-2164),
   * the Conformer encoder of ids 7 and 8 on those tokens, and classifier =
   * Linear(144, classes_num) on every token: token 0 is the clipwise output, the
   * others the framewise output (:2177-2179).  Both outputs are LOGITS: no
   * sigmoid, no frame repeat, no padding.  feature_type must be LOGMEL;
   * classes_num is the classifier's width, 1..256.  The encoder and the
   * classifier are fp32 in every precision mode.
   *   geometry   T = L / hop + 1 frames; T3 = T / 8; seq_len = 8 T3 + 1 tokens;
   *              out_frames = 8 T3 (10 s at hop 160 / 16 kHz: 1001 tokens, 1000
   *              frames; 10400 samples: 64 frames; 7777: 48; 81760: 512)
   *   refusals   T < 8 (the third pool has no output) and seq_len > 5000 (the
   *              encoder's positional table): SEDX_EINVAL from the forwards,
   *              sedx_output_geometry, sedx_workspace_size, the launch plans and
   *              the windowed drivers, before any launch
   *   keys       the 9-layer trunk's (frontend buffers, bn0, conv_block1-4),
   *              encoder.* as ids 7 and 8, classifier.{weight [C][144], bias [C]}
   *              and linear_emb.{weight [512][1], bias [512]}: all four are read
   *              and a missing one is SEDX_EKEY; no att_block.*, no fc.*
   *   outputs    d_framewise [B][8 T3][C] and d_clipwise [B][C]; the reference
   *              returns no 'embedding': d_embedding is ignored and may be NULL
   * Captures (sedx_set_capture): 0 and 2..7 as the 9-layer models; 8 is the token
   * buffer [items][seq_len][512], tag row included; 20 and 21 + 4b + j as ids 7
   * and 8, here [items][seq_len][144]; 9 is the encoder's output (the same tensor
   * as 32); 44 is the classifier's logits [M][nac], M = items x seq_len, nac =
   * classes_num rounded up to 64 (zeros beyond C): the outputs are its rows, bit
   * for bit.  Timed stage 8 is block 4's conv2 plus the token kernel, 9 the
   * encoder, 10 the classifier and the split. */
  SEDX_MODEL_CONFORMER_TOKEN = 21,
  /* Cnn_9layers_Gru_Reg  :2788-2889: Cnn_9layers_Gru_FrameAtt (id 0) without
   * pad_framewise_output (:2880-2882): the same constructor, state_dict keys,
   * AttBlock(512, 25), LOGMEL or GAMMA features, captures and timed stages;
   * out_frames = 8 (T / 8), never padded to a multiple of 100; d_embedding = cla
   * [B, C, seq_len].  Its framewise output is the first out_frames frames of id
   * 0's, bit for bit, and so are the clipwise output and the embedding. */
  SEDX_MODEL_GRU_REG = 22
} sedx_model;

typedef enum { SEDX_FEATURE_LOGMEL = 0, SEDX_FEATURE_GAMMA = 1 } sedx_feature;

/* Constructor arguments of the reference models (pytorch/models.py:565-566):
 * (sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
 * feature_type).  mel_bins must be 64 (bn0 is BatchNorm2d(64), models.py:607). */
typedef struct {
  int32_t model_type;     /* sedx_model   */
  int32_t feature_type;   /* sedx_feature */
  int32_t sample_rate;
  int32_t window_size;    /* n_fft: 256, 512 or 1024 */
  int32_t hop_size;
  int32_t mel_bins;
  float fmin;
  float fmax;
  int32_t classes_num;
} sedx_config;

typedef struct sedx_handle sedx_handle;

/* Model construction: replaces Model(...) (pytorch/models.py:565-623 / :982-1024
 * and the constructors of the other sedx_model values).  feature_type GAMMA is
 * Cnn_9layers_Gru_FrameAtt's alone (Cnn_9layers_Gru_FrameAvg takes the argument
 * and ignores it, :512-518); any other model_type with it is SEDX_EINVAL
 * (the 14-layer and the VGGish models included, SEDX_MODEL_CONFORMER14_FRAMEATT and SEDX_MODEL_CONFORMER_TOKEN too;
 * SEDX_MODEL_GRU_REG takes it as id 0 does).  classes_num: 1..256, and up to 527 for
 * SEDX_MODEL_CNN14_DECISIONLEVELATT. */
sedx_status sedx_create(const sedx_config* cfg, int device, sedx_handle** out);
void sedx_destroy(sedx_handle* h);
const char* sedx_last_error(const sedx_handle* h);
/* "sedx <major>.<minor> (abi N)".  SEDX_ABI_VERSION changes whenever an
 * entry point's signature or a struct layout changes incompatibly; a caller
 * built against this header checks sedx_abi_version() == SEDX_ABI_VERSION
 * at load time ("ABI history"). */
#define SEDX_ABI_VERSION 6
const char* sedx_version(void);
int32_t sedx_abi_version(void);

/* One state_dict entry (host fp32; int64 scalars such as num_batches_tracked
 * are skipped by the caller).  Keys/shapes exactly as the reference
 * state_dict; unused keys (att_block.bn_att.*,
 * multihead.layer_norm.*) are accepted and ignored.  The key set is the
 * model's own: the fc models take fc.weight [C, 512] / fc.bias [C] and no
 * att_block.*, the CNN-only models no gru.* / multihead.*; a key of another
 * family is SEDX_EKEY.  The Conformer models take encoder.input_layer.{0,1}.*,
 * encoder.input_layer.4.pe [1, 5000, 144] (loaded, not recomputed),
 * encoder.conformer_blocks.{0,1,2}.* (ffn1 / ffn2 feed_forward_module.{0,1,4},
 * mhsa.{r_w_bias, r_r_bias, qkv_net, o_net, layer_norm, pos_emb.inv_freq,
 * r_net}, conv.conv.{0,1.conv,3.conv,5,8.conv}, norm) and a 144-wide head
 * (att_block.{att,cla}.weight [25, 144, 1] or fc.weight [C, 144]);
 * classifier.* and linear_emb.* (unused at inference) are accepted and
 * ignored.  Replaces
 * model.load_state_dict(checkpoint['model']) (pytorch/predict.py:232-233). */
sedx_status sedx_load_param(sedx_handle* h, const char* key, const float* h_data,
                            const int64_t* shape, int32_t ndim);
/* Folds BN into conv weights, pre-packs GEMM layouts, uploads to the device.
 * Must follow the last sedx_load_param and precede any forward. */
sedx_status sedx_finalize_weights(sedx_handle* h);

/* Output geometry for a batch of waveforms of L samples (logmel) or of
 * feature matrices with T frames (gamma): frames of framewise_output
 * (after x8 interpolation and, Cnn_9layers_Gru_FrameAtt and the Conformer
 * models only, padding to a multiple of 100: models.py:62-95, :678-681) and the sequence length after
 * the CNN. */
sedx_status sedx_output_geometry(const sedx_handle* h, int64_t L_or_T, int64_t* out_frames,
                                 int64_t* seq_len);
/* Bytes of device workspace sedx_forward* needs for (B, L). */
sedx_status sedx_workspace_size(const sedx_handle* h, int64_t B, int64_t L_or_T, size_t* bytes);

/* The conv launches of stages 2-8 of a forward of (B, L) at the handle's
 * current precision and tuning, as the launchers decide them (read-only; no
 * launch, no output depends on any of it).  One row per launch: a batch whose
 * input passes the kernels' 32-bit offsets runs a stage as several launches of
 * whole clips.  Rows of the exact, x3 and f16 launchers carry the layer only
 * (the fields from `clips` on are 0). */
typedef enum sedx_conv_family {
  SEDX_CONV_EXACT = 0,
  SEDX_CONV_X3 = 1,
  SEDX_CONV_F23 = 2,         /* Winograd F(2x2,3x3) */
  SEDX_CONV_F23_BLOCK1 = 3,  /* block 1 in one F(2x2,3x3) launch (conv1 inside) */
  SEDX_CONV_F43 = 4,         /* Winograd F(4x4,3x3) */
  SEDX_CONV_F16 = 5          /* the fp16 matrix-pipe launcher (SEDX_PRECISION_F16); rows as the x3 launcher's */
} sedx_conv_family;
typedef struct sedx_conv_launch {
  int32_t stage, family;              /* 2..8 (sedx_stage_times' numbering), sedx_conv_family */
  int32_t T, F, cin, cout, epi;       /* the layer: rows, columns, channels; 0 store, 1 2x2 pool, 2 freq mean;
                                       * the VGGish trunk's rows (stages 2..6, the exact launcher): 3 2x2 max pool,
                                       * 4 2x2 max pool + mean of the 4 pooled bins */
  int32_t clips;                      /* clips of this launch */
  int32_t tg, nt, c4;                 /* item: tile groups, channel tiles; chunk-of-4 layout */
  int32_t tb_per_clip, ngroups;       /* tile blocks per clip, channel groups */
  int32_t nitems, nwg;                /* items, persistent workgroups */
  int32_t claim, order2d;             /* items claimed from counters; channel groups per L2 round (0, -1: see DESIGN.md) */
  int64_t clips_per_launch;           /* most clips one launch takes */
} sedx_conv_launch;
/* ncu > 0: the answer for a device of that many CUs, touching no device;
 * ncu <= 0: the handle's device.  *n_rows = rows of the answer; SEDX_EINVAL
 * if capacity is smaller or the forward refuses the shape. */
sedx_status sedx_conv_launch_plan(const sedx_handle* h, int64_t B, int64_t L_or_T, int32_t ncu,
                                  sedx_conv_launch* rows, int32_t capacity, int32_t* n_rows);

/* The GEMM launches of the sequence layer (stage 9) and the head (stage 10) of
 * a forward of (B, L) at the handle's current precision, in launch order
 * (read-only; no launch, no output depends on any of it).  Rows of the fp32
 * GEMM launcher carry the kernel it picks for M = B * seq_len rows on `ncu`
 * CUs and its grid; rows of the split-bf16 and Conformer GEMM launchers carry
 * the GEMM only (grid 0).  Cnn14_DecisionLevelAtt's fused pooling + fc1 launch
 * is not a GEMM launcher's: its one row is the head projection.  ncu, capacity
 * and *n_rows as for the conv query above, and the same refusals. */
typedef enum sedx_gemm_kernel {
  SEDX_GEMM_TILED = 0,     /* 128 x 64 tiles through LDS, 256 threads */
  SEDX_GEMM_ONE_WAVE = 1,  /* 32 x 32 tiles, one wave each, operands from L2 */
  SEDX_GEMM_KSPLIT = 2,    /* 32 x 32 tiles, four waves on K quarters (N <= 64: the AttBlock / fc projection) */
  SEDX_GEMM_X3 = 3,        /* the split-bf16 launcher (9-layer models, SEDX_PRECISION_X3) */
  SEDX_GEMM_CONFORMER = 4  /* the Conformer encoder's launcher */
} sedx_gemm_kernel;
typedef struct sedx_gemm_launch {
  int32_t stage;             /* 9 sequence layer, 10 head */
  int32_t M, K, N, act;      /* C [M][N] = act(A [M][K] W^T + b); act 1 = ReLU (Conformer rows: 0, its own epilogues) */
  int32_t kernel;            /* sedx_gemm_kernel */
  int32_t grid_x, grid_y;    /* workgroups over rows and columns */
} sedx_gemm_launch;
sedx_status sedx_gemm_launch_plan(const sedx_handle* h, int64_t B, int64_t L_or_T, int32_t ncu,
                                  sedx_gemm_launch* rows, int32_t capacity, int32_t* n_rows);

/* Model forward (eval mode): replaces Cnn_9layers_*_FrameAtt.forward(input)
 * (pytorch/models.py:625-688, :1029-1077).
 *   d_wave       [B, L]                         (logmel models)
 *   d_framewise  [B, out_frames, classes_num]
 *   d_clipwise   [B, classes_num]
 *   d_embedding  GRU_FRAMEATT, CNN_FRAMEATT: [B, classes_num, seq_len] (cla);
 *                every other model: [B, 512, seq_len], the head's input
 *                transposed (the GRU / MHA output; CNN_FRAMEMAX / CNN_FRAMEAVG:
 *                block 4's frequency mean); the Conformer models:
 *                [B, 144, seq_len], the encoder output transposed
 *                (may be NULL); CNN14_DECISIONLEVELATT: ignored, nothing is
 *                written (the reference returns no embedding)
 * The Conformer models hold at most 5000 sequence frames (the positional
 * table): beyond, the forward, geometry and workspace queries are SEDX_EINVAL.
 *   d_workspace  NULL = handle-owned cache, else >= sedx_workspace_size bytes. */
sedx_status sedx_forward(sedx_handle* h, const float* d_wave, int64_t B, int64_t L,
                         float* d_framewise, float* d_clipwise, float* d_embedding,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/* Same forward on int16 waveforms as packed in the reference's HDF5 files
 * (utils/features.py:313-317, :370): the loader's int16_to_float32
 * (utils/data_generator.py:39, utils/utilities.py:78-79: float64 x / 32767
 * rounded to float32) is fused into the frontend's loads, halving the input
 * bytes.  Bit-identical to sedx_forward on the dequantised waveform. */
sedx_status sedx_forward_i16(sedx_handle* h, const int16_t* d_wave, int64_t B, int64_t L,
                             float* d_framewise, float* d_clipwise, float* d_embedding,
                             void* d_workspace, size_t workspace_bytes, void* stream);

/* Gamma branch (models.py:636-640): input is the [B, 64, T] feature matrix
 * that the reference model receives (int16-dequantised gammatone dB). */
sedx_status sedx_forward_features(sedx_handle* h, const float* d_feat, int64_t B, int64_t T,
                                  float* d_framewise, float* d_clipwise, float* d_embedding,
                                  void* d_workspace, size_t workspace_bytes, void* stream);

/* Gammatone frontend (utils/gammatone/fftweight.py:126-168 + power_to_db
 * top_db=80 + float32_to_int16 / int16_to_float32, utils/features.py:361-370,
 * utils/utilities.py:73-79): d_audio [B, L] (already pad_truncated to 10 s)
 * -> d_feat [B, 64, T], T = 1 + floor((L - nfft) / hop).  Computed in float64
 * like the reference's numpy (FFT, |X|, the ERB product, dB, top_db clamp and
 * the int16 quantisation), so the int16 codes equal the reference's.
 * d_feat == NULL: geometry query (T_out only).  Workspace:
 * sedx_gamma_workspace_size (NULL d_workspace = handle-owned cache). */
sedx_status sedx_gamma_features(sedx_handle* h, const float* d_audio, int64_t B, int64_t L,
                                float* d_feat, int64_t* T_out, void* d_workspace,
                                size_t workspace_bytes, void* stream);
sedx_status sedx_gamma_workspace_size(const sedx_handle* h, int64_t B, int64_t L, size_t* bytes);
/* Where sedx_gamma_features keeps its stages in the workspace (byte offsets
 * from its base; a debugging and test aid, the contents are only defined
 * after a call on that workspace has completed):
 *   mag [B][T][kp] float64   |FFT| of the windowed frames; bins nfft/2+1 .. kp-1
 *                            and the rows T_fill .. T-1 of every clip are 0
 *   db  [B][64][T] float64   10 log10(max(1e-10, W . mag / nfft))
 *   mm  [B][2]     uint64    per-clip max / min of db as order-preserving keys
 * T = 1 + floor((L - nfft) / hop) columns, of which the reference's specgram
 * loop range(0, L - nfft, hop) fills the first T_fill (T - 1 when hop divides
 * L - nfft).  total_bytes is what sedx_gamma_workspace_size reports.  The
 * sizes follow from the configuration alone: no weights or device needed. */
typedef struct {
  int64_t T, T_fill;
  int32_t nfft, hop, kp, reserved;
  size_t mag_offset, db_offset, mm_offset, total_bytes;
} sedx_gamma_layout;
sedx_status sedx_gamma_workspace_layout(const sedx_handle* h, int64_t B, int64_t L, sedx_gamma_layout* out);

/* One call from audio, whatever the model's features.  On a log-mel handle
 * this is sedx_forward.  On a gamma handle the gammatone frontend runs inside
 * the forward: d_audio [B, L] (pad_truncate'd clips, L >= nfft) -> float64
 * spectrum, ERB product and dB as in sedx_gamma_features, then a quantiser
 * that writes the conv input directly (the int16 quantisation followed by bn0;
 * no [B, 64, T] feature tensor), then the model.  The three outputs equal
 * sedx_gamma_features + sedx_forward_features on the same clips bit for bit.
 * The frontend is timed stage 0 and runs ahead of sedx_set_pipelined's wait,
 * so on a pipelined handle batch i + 1's features overlap batch i's conv
 * stack.  B <= 65535 on a gamma handle.
 *   sedx_audio_geometry        T frames, out_frames, seq_len of L samples
 *                              (any of the three may be NULL)
 *   sedx_audio_workspace_size  the model workspace plus, on a gamma handle,
 *                              the frontend's mag / db / mm for B items
 * Both queries reject exactly what the forward rejects. */
sedx_status sedx_forward_audio(sedx_handle* h, const float* d_audio, int64_t B, int64_t L,
                               float* d_framewise, float* d_clipwise, float* d_embedding,
                               void* d_workspace, size_t workspace_bytes, void* stream);
sedx_status sedx_audio_geometry(const sedx_handle* h, int64_t L, int64_t* T, int64_t* out_frames,
                                int64_t* seq_len);
sedx_status sedx_audio_workspace_size(const sedx_handle* h, int64_t B, int64_t L, size_t* bytes);

/* Windowed drivers: pytorch/predict.py:297-349 (`predict`) and
 * pytorch/main_strong.py:786-835 (`inference_prob_overlap`) / :1052-1100
 * (`inference_prob_vote`).  The reference's loops take three independent
 * numbers, kept apart here exactly as they are there:
 *   stride      how far `start` advances per window:
 *                 predict.py  `start += 1` with --overlap, else
 *                             `start += sample_duration` (predict.py:334-337);
 *                 main_strong `start += overlap_value` (main_strong.py:829, :1094)
 *               (start is an int in predict.py, a float64 running sum in
 *               main_strong; window w reads samples int(start_w * sr) ...)
 *   merge step  int(100 * overlap_value) frames, computed in float64
 *               (utilities.py:406, :426; vad.py:63): window w lands at frame
 *               w * step of the merged output WHATEVER the stride
 *   loop bound  `while end <= audio_duration`, end = start + sample_duration,
 *               audio_duration = librosa.get_duration of the file (predict.py:277,
 *               main_strong.py:778).
 * predict.py pad_truncate's every window to sample_duration s (:305);
 * main_strong pad_truncate's the whole clip to 10 s (:790) and feeds each
 * window as sliced, so a window that runs past 10 s is SHORTER (its own
 * forward, fewer frames; the merge then follows numpy's slicing and
 * broadcasting exactly, raising SEDX_EINVAL where numpy raises).
 *
 * On a gamma handle (the reference's predict.py raises on one; its features
 * are made per clip when the HDF5 files are packed, utils/features.py:356-370)
 * every driver below treats a window as that packing treats a clip: the
 * window's samples, zero-padded to its length where the clip ends, go through
 * fft_gtgram (T = 1 + (len - nfft) / hop un-centred frames), power_to_db
 * (top_db 80) and the int16 quantisation by the WINDOW's own max |dB|, inside
 * the forward (sedx_forward_audio's frontend, one item per window).  A window
 * shorter than nfft samples is refused. */
typedef enum { SEDX_DRIVER_PREDICT = 0, SEDX_DRIVER_MAIN_STRONG = 1 } sedx_window_driver;
typedef struct {
  int32_t driver;           /* sedx_window_driver */
  int32_t overlap;          /* PREDICT: predict.py --overlap (stride 1 s, else sample_duration s); MAIN_STRONG: ignored */
  int32_t sample_duration;  /* seconds (an int in both drivers: predict.py:701, main_strong.py:746) */
  int32_t vote;             /* 0: the averaged merge (sedx_forward_windows, avg_merge after merge);
                               1: the vote merge (sedx_forward_windows_vote, merge only).  Picks the
                               plan sedx_window_geometry / sedx_window_workspace_size size, so they
                               reject exactly what the matching forward rejects (avg_merge raises on
                               a zero step, the vote merge does not).  Was `reserved` (0) before
                               ABI 5: old callers get the averaged path, as before. */
  double overlap_value;     /* merge step int(100 * overlap_value); MAIN_STRONG: also the stride */
  double audio_duration;    /* the loop bound in seconds; <= 0: L_clip / sample_rate */
} sedx_window_spec;

/* Handle-free loop control: the sample offset of every window and the
 * samples the model receives for it (h_len: sample_duration * sr, except
 * main_strong windows that run past the 10 s padded clip).  Fills at most
 * `capacity` entries (h_start / h_len may be NULL) and sets *n_windows.
 * SEDX_EINVAL for sample_duration <= 0 or a stride <= 0 (the reference's loop
 * never ends).  The model-dependent limits (a window of <= n_fft/2 samples
 * fails the STFT's reflect padding, pytorch/stft.py:237; fewer than 8 frames
 * fail the third 2x2 pooling, models.py:139) are checked by
 * sedx_window_geometry, which needs the handle. */
sedx_status sedx_window_starts(int32_t sample_rate, int64_t L_clip, const sedx_window_spec* spec,
                               int64_t* h_start, int64_t* h_len, int64_t capacity, int64_t* n_windows);
/* Handle-free host merge: utilities.merge applied window by window exactly
 * as the drivers call it (predict.py:323-329), then utilities.avg_merge when
 * `avg` (predict.py:349), on float32 host arrays.  h_win = the windows'
 * framewise outputs [frames[w]][C] concatenated in window order; h_out
 * [merged_frames][C] (NULL: size query).  Slicing with numpy's clamping and
 * broadcasting semantics; SEDX_EINVAL where numpy raises (broadcast of
 * mismatched lengths, avg_merge with a zero step). */
sedx_status sedx_merge_host(const float* h_win, const int64_t* frames, int64_t n_win, int64_t C,
                            int32_t sample_duration, double overlap_value, int32_t avg, float* h_out,
                            int64_t capacity_frames, int64_t* merged_frames);

/* Runs ALL windows of ALL clips as one batch (a main_strong window shorter
 * than sample_duration as its own small batch), overlap-adds on the GPU
 * (utilities.py:405-423) and applies the avg_merge divisor schedule
 * (utilities.py:425-446).
 *   d_audio       [n_clips, L_clip] (every clip the same length)
 *   d_merged      [n_clips, merged_frames, classes_num]
 * sedx_window_geometry returns n_windows per clip, samples per full window
 * and merged_frames. */
sedx_status sedx_window_geometry(const sedx_handle* h, int64_t L_clip, const sedx_window_spec* spec,
                                 int64_t* n_windows, int64_t* window_samples, int64_t* merged_frames);
sedx_status sedx_forward_windows(sedx_handle* h, const float* d_audio, int64_t n_clips, int64_t L_clip,
                                 const sedx_window_spec* spec, float* d_merged, void* d_workspace,
                                 size_t workspace_bytes, void* stream);
sedx_status sedx_window_workspace_size(const sedx_handle* h, int64_t n_clips, int64_t L_clip,
                                       const sedx_window_spec* spec, size_t* bytes);
/* Voting variant (inference_prob_vote, pytorch/main_strong.py:1052-1100):
 * every window's framewise output is binarised, x > bin_thres[k] (host f64
 * [classes_num]; the reference passes sed_low_threshold, main_strong.py:1082,
 * binarize_pred :870-883), and the 0/1 windows are overlap-added with
 * utilities.merge — no avg_merge.  d_votes [n_clips, merged_frames,
 * classes_num] holds the vote counts (exact small integers) for
 * sedx_events_device(mode = 1).  Workspace: sedx_window_workspace_size. */
sedx_status sedx_forward_windows_vote(sedx_handle* h, const float* d_audio, int64_t n_clips, int64_t L_clip,
                                      const sedx_window_spec* spec, const double* bin_thres, float* d_votes,
                                      void* d_workspace, size_t workspace_bytes, void* stream);

/* Ragged form of the `predict` driver: recordings of DIFFERENT lengths in one
 * call (pytorch/predict.py:264-407 walks a directory of them).  Every clip
 * follows exactly the rules of sedx_window_geometry for its own length and
 * duration; the windows of all clips then form one item list that runs
 * through the model in forwards of at most items_per_forward items (<= 0:
 * all at once), and each clip is merged and averaged on its own.  A clip's
 * output does not depend on the batch it runs in, so it is the output of
 * sedx_forward_windows on that clip alone, bit for bit.
 *   spec              driver SEDX_DRIVER_PREDICT and vote 0 only (main_strong
 *                     pads every clip to 10 s: it has no ragged form);
 *                     spec->audio_duration must be <= 0:
 *   h_audio_duration  NULL, or [n_clips] loop bounds in seconds (an entry
 *                     <= 0, like NULL: that clip's length / sample_rate)
 *   h_clip_len        [n_clips] samples per clip
 *   h_n_windows       [n_clips] windows per clip (may be NULL)
 *   h_frame_off       [n_clips + 1] prefix sum of the clips' merged frame
 *                     counts (may be NULL)
 * A clip sedx_window_geometry refuses (an empty clip, a window of <= n_fft/2
 * samples, the model's frame limits, a zero merge step), and, here only, a
 * clip without one complete window (fewer than sample_duration * sample_rate
 * samples; alone it runs as one zero-padded window), makes the whole call
 * SEDX_EINVAL before any launch; sedx_last_error names its index.
 *   d_audio           the clips back to back, fp32; clip c holds samples
 *                     h_clip_off[c] .. h_clip_off[c + 1]) (any offsets, odd
 *                     ones included; non-decreasing).  Samples a window needs
 *                     past its clip's end read as zero (pad_truncate), never
 *                     as the next clip's audio, and nothing past
 *                     h_clip_off[n_clips] is read.
 *   d_merged          [h_frame_off[n_clips]][classes_num]; clip c's rows
 *                     start at h_frame_off[c]
 * The workspace holds the model's for ONE forward of items_per_forward items,
 * plus every window's framewise output (out_frames x classes_num floats) and
 * the tables (one upload).  Asynchronous on `stream` like the other drivers;
 * a GRU hand-off time-out surfaces through sedx_check_error. */
sedx_status sedx_ragged_window_geometry(const sedx_handle* h, const int64_t* h_clip_len, int64_t n_clips,
                                        const sedx_window_spec* spec, const double* h_audio_duration,
                                        int64_t* h_n_windows, int64_t* h_frame_off, int64_t* window_samples,
                                        int64_t* total_windows);
sedx_status sedx_ragged_window_workspace_size(const sedx_handle* h, const int64_t* h_clip_len, int64_t n_clips,
                                              const sedx_window_spec* spec, const double* h_audio_duration,
                                              int64_t items_per_forward, size_t* bytes);
sedx_status sedx_forward_windows_ragged(sedx_handle* h, const float* d_audio, const int64_t* h_clip_off,
                                        int64_t n_clips, const sedx_window_spec* spec,
                                        const double* h_audio_duration, int64_t items_per_forward, float* d_merged,
                                        void* d_workspace, size_t workspace_bytes, void* stream);

/* Arithmetic of the GEMM-shaped work: the 9-layer conv stack (96.8 % of the
 * FLOPs), the GRU input projection and recurrence, the MHA projections and
 * the AttBlock projection.
 *  SEDX_PRECISION_EXACT  fp32 operands, fp32 accumulation
 *                       (v_mfma_f32_32x32x2_f32 / fp32 FMA): the reference's
 *                       arithmetic (pytorch/models.py:614-615, :663-670),
 *                       direct 3x3 convolution.
 *  SEDX_PRECISION_WINOGRAD (default)  fp32 throughout as EXACT, with block 1's conv2
 *                       (SEDX_TUNE_WINO_BLOCK1) and the six conv layers
 *                       of blocks 2-4 computed by Winograd F(4x4,3x3)
 *                       (SEDX_TUNE_WINO_F43; 1: block 1 by F(2x2,3x3), 0:
 *                       every layer by F(2x2,3x3)):
 *                       input / weight / output transforms and the
 *                       element-wise GEMMs all in fp32 (weights transformed
 *                       in float64, rounded once), 2.25x / 4x fewer
 *                       multiplies than the direct conv; F(2x2,3x3)'s error
 *                       vs a float64 conv is at or below the direct conv's,
 *                       F(4x4,3x3)'s ~6x it (tools/wino_bench.cpp,
 *                       tools/wino43_bench.cpp).  Different rounding from
 *                       EXACT, so not bit-identical to it.
 *  SEDX_PRECISION_X3    opt-in: bf16 MFMA with a 3-term hi/lo operand split
 *                       (hi*hi + hi*lo + lo*hi, fp32 accumulate): operands
 *                       carry 16 significant bits, products err ~2^-16 rel.
 *  SEDX_PRECISION_F16   opt-in, reduced precision: the conv layers that X3 runs
 *                       on the bf16 pipe (block 1's conv2 and blocks 2-4 of the
 *                       9-layer trunk; on the 14-layer trunk block 1's conv2
 *                       to block 4's conv1) run on the f16 matrix pipe, one
 *                       v_mfma_f32_32x32x16_f16 per product.  Per layer both
 *                       operands v (the BN-folded weight after its one rounding
 *                       to fp32, and the fp32 input activation) become q(v):
 *                       clamped to +-65504, rounded to the nearest-even fp16
 *                       with gradual underflow in the rounding itself, then
 *                       every result with |q| < 2^-14 set to +0 (so the
 *                       result does not depend on how the matrix pipe treats
 *                       fp16 subnormals).  Products are accumulated in fp32;
 *                       the folded-BN bias (fp32), ReLU, the 2x2 average pool
 *                       and block 4's frequency mean are fp32.  Activations
 *                       stay fp32 in memory, in the exact mode's layout, and
 *                       the workspace is the exact mode's.  Everything else
 *                       runs as in EXACT: block 1's conv1, the 14-layer
 *                       trunk's deep layers, the VGGish trunk, the Conformer
 *                       encoder, every sequence layer and head.  One output's
 *                       summation order depends on neither the batch, the
 *                       tile claim order nor the stream.  Outputs move by
 *                       ~5e-5 against EXACT on synthetic weights (DESIGN.md
 *                       §4, "fp16 conv stack").
 * The frontend (FFT, mel, dB), the gates, softmax and the head's
 * element-wise work are fp32 in every mode; the gammatone frontend float64. */
typedef enum {
  SEDX_PRECISION_EXACT = 0,
  SEDX_PRECISION_X3 = 1,
  SEDX_PRECISION_WINOGRAD = 2,
  SEDX_PRECISION_F16 = 3
} sedx_precision;
sedx_status sedx_set_precision(sedx_handle* h, int32_t mode);

/* Implementation choices that leave the arithmetic's meaning unchanged (A/B
 * measurement and tests; the defaults are the fastest measured):
 *  SEDX_TUNE_GRU_KERNEL   SEDX_GRU_KERNEL_AUTO (default): COOP16 (the shorter
 *                         recurrence), on a pipelined handle with its
 *                         workgroups dealt over every XCD (the recurrence
 *                         runs beside the next batch's conv stack);
 *                         SEDX_GRU_KERNEL_COOP: the cooperative
 *                         recurrence, 8 workgroups per (32-clip group,
 *                         direction) exchanging h slices every step (up to 8
 *                         clips: the small-batch VALU kernel with a data-tagged
 *                         hand-off); SEDX_GRU_KERNEL_TAG16 / _TAG8 (exact,
 *                         more than 8 clips): 16-clip groups on 16 / 8
 *                         workgroups exchanging data-tagged granules straight
 *                         into the MFMA operands (lower product latency, more
 *                         CUs held: slower beside a second batch's conv stack);
 *                         SEDX_GRU_KERNEL_SIMPLE: one workgroup per (clip,
 *                         direction), W_hh streamed from L2 (fp32 FMA);
 *                         SEDX_GRU_KERNEL_COOP16 (exact, more than 8 clips):
 *                         the cooperative kernel on 16 workgroups per
 *                         (32-clip group, direction) — half the serial
 *                         product per step, twice the CUs held;
 *                         bit-identical to COOP.
 *                         SEDX_GRU_KERNEL_KSPLIT (exact, more than 8 clips):
 *                         16 workgroups per (32-clip group, direction), each
 *                         K-eighth wave waiting only for the two slices it
 *                         multiplies and loading their h straight into its
 *                         MFMA operands (no LDS gather); bit-identical.
 *                         SEDX_GRU_KERNEL_PAIR (exact, more than 8 clips):
 *                         the K-split structure with each 32-clip group's
 *                         two 16-clip halves stepped alternately in one
 *                         workgroup (one half's hand-off behind the other's
 *                         product); bit-identical.
 *  SEDX_TUNE_GRU_HANDOFF  (COOP) SEDX_GRU_HANDOFF_AUTO (default): XCD-local hand-off
 *                         when all 8 slices share an XCD, else global; on a
 *                         pipelined handle (sedx_set_pipelined) SPREAD;
 *                         SEDX_GRU_HANDOFF_GLOBAL: always the global protocol
 *                         (same bytes, bit-identical results);
 *                         SEDX_GRU_HANDOFF_SPREAD: the global protocol with a
 *                         (group, direction)'s workgroups dealt over every XCD
 *                         (beside a concurrent conv stack no XCD loses a
 *                         quarter of its CUs; bit-identical).
 *                         SEDX_GRU_HANDOFF_LOCAL: a (group, direction)'s
 *                         workgroups on one XCD with the XCD-local hand-off
 *                         when they all landed there, also on a pipelined
 *                         handle (A/B of the placement; bit-identical).
 *  SEDX_TUNE_MEL_MFMA     (n_fft 512) 0 (default): the log-mel frontend's mel
 *                         projection as VALU band sums; 1: on
 *                         v_mfma_f32_16x16x4_f32, the workgroup's 16 frames x
 *                         one 16-band tile per wave over the tile's bin range
 *                         (the same in-order fma chain per band:
 *                         bit-identical; measured 1.4x slower at B = 32: the
 *                         tile's single MFMA chain and two workgroup barriers
 *                         per 16 frames cost more than the band sums' VALU).
 *  SEDX_TUNE_WINO_BLOCK1  (SEDX_PRECISION_WINOGRAD only) 2 (default): block 1
 *                         as ONE launch — conv1 computed into conv2's halo
 *                         images in LDS (the 64-channel activation never
 *                         exists), conv2 as Winograd F(2x2,3x3), pool;
 *                         1: the same conv2 fed by a separate conv1 launch
 *                         (the activation through HBM; bit-identical to 2);
 *                         0: block 1 as the direct fused fp32 kernel.
 *                         With SEDX_TUNE_WINO_F43 2 (its default) 1 and 2
 *                         both run conv1's own launch + the F(4x4,3x3) conv2
 *                         (2: conv1 channel-planar — or in the chunk-of-4
 *                         layout, SEDX_TUNE_WINO_ORDER 3 — 1: NHWC;
 *                         bit-identical).
 *  SEDX_TUNE_GRU_SPIN     bound of every GRU hand-off spin, in polls (default
 *                         2^24 = 16777216).  A spin that runs out turns that
 *                         forward's outputs into NaN and is reported by
 *                         sedx_check_error (tests force it with 0: every
 *                         step that would wait fails, whether or not its data
 *                         has arrived).  The 14-layer GRU model's recurrence
 *                         (hidden size 1024) is one launch per time step
 *                         with no spins: SEDX_TUNE_GRU_SPIN,
 *                         SEDX_TUNE_GRU_KERNEL and SEDX_TUNE_GRU_HANDOFF are
 *                         accepted and ignored on its handles, and
 *                         sedx_check_error has nothing to report for them.
 *  SEDX_TUNE_GAMMA_SPEC  (gammatone, nfft 2048) 0 (default): the spectrum
 *                         as a 256-thread Stockham FFT per frame; 1: one
 *                         wave per frame (16 x 16 x 4 four-step in registers,
 *                         wave-local transposes).  Same int16 codes in every
 *                         test (f64 sums in another order).
 *  SEDX_TUNE_WINO_ORDER   (winograd) 1 (default): layers whose channel groups'
 *                         weight slabs exceed ~8 MB together (the 512-channel
 *                         layers) run each XCD's rounds of 32 concurrent items
 *                         as 8 tile blocks x 4 channel groups of 64 (4 slabs
 *                         per round through the XCD's L2 instead of 8);
 *                         0: tile block major; 2: as 1, and block 1's F(4x4,3x3)
 *                         conv2 gives each XCD a contiguous range of tile
 *                         blocks (neighbouring items' shared halo rows read
 *                         once into that XCD's L2); 3: as 1, and block 1's
 *                         conv1 writes the chunk-of-4 layout that its
 *                         F(4x4,3x3) conv2 then stages plane by plane (the
 *                         default: channel-planar, staged by 16-byte LDS-DMAs;
 *                         the A/B of the two).  Bit-identical outputs.
 *  SEDX_TUNE_WINO_F43     (winograd) 2 (default): block 1's conv2 and the
 *                         six conv layers of blocks 2-4 as fp32 Winograd
 *                         F(4x4,3x3) (36 multiplies per 4x4 tile,
 *                         v_mfma_f32_16x16x4_f32, csrc/conv_wino43.hip),
 *                         block 1 as a conv1 launch + that conv2 (conv1's
 *                         activation in the workspace); 1: blocks 2-4 only
 *                         (block 1 per SEDX_TUNE_WINO_BLOCK1 on F(2x2,3x3));
 *                         0: every layer F(2x2,3x3).  Different
 *                         rounding (both fp32 throughout; F(4,3)'s error vs a
 *                         float64 conv is ~6x the direct conv's, still ~1e-5
 *                         of the 1e-3 bar), so not bit-identical to each other.
 *  SEDX_TUNE_CF_ATTN      (the four Conformer models) the encoder's relative
 *                         attention core.  0: four lanes per query on the vector
 *                         ALUs, exact two-pass softmax (cf_relattn_kernel,
 *                         csrc/conformer.hip); 1: the fp32 matrix pipe
 *                         (v_mfma_f32_16x16x4_f32), 64 queries x 64 keys per
 *                         step, online softmax with rescaling
 *                         (csrc/conformer_attn.hip); 2 (default): per model --
 *                         ids 7, 8 and 19 run 0, so their output bits are those
 *                         of every earlier release; id 21 runs 1 (7.6-8.0 ms
 *                         against 1.56-1.57 ms for the three launches of a
 *                         forward at 32 x 1001 tokens).  Both are fp32
 *                         throughout and differ in summation order only.
 *
 * Co-residency: the cooperative GRU kernels need all workgroups of a
 * (32-clip group, direction) resident at once — 8 CUs (COOP) or 16 (COOP16)
 * per pair, one workgroup per CU — and spin on each other.  AUTO picks
 * COOP16; forwards running concurrently on other streams leave fewer CUs free
 * for it: the spins are bounded (SEDX_TUNE_GRU_SPIN), so the worst case is a
 * NaN batch reported by sedx_check_error, never a hang. */
typedef enum {
  SEDX_TUNE_GRU_KERNEL = 0,
  SEDX_TUNE_GRU_HANDOFF = 1,
  SEDX_TUNE_WINO_BLOCK1 = 2,
  SEDX_TUNE_MEL_MFMA = 3,
  SEDX_TUNE_GRU_SPIN = 4,
  SEDX_TUNE_WINO_ORDER = 5,
  SEDX_TUNE_GAMMA_SPEC = 6,
  SEDX_TUNE_WINO_F43 = 7,
  SEDX_TUNE_CF_ATTN = 8
} sedx_tuning_knob;
enum {
  SEDX_GRU_KERNEL_COOP = 0,
  SEDX_GRU_KERNEL_SIMPLE = 1,
  SEDX_GRU_KERNEL_TAG16 = 2,
  SEDX_GRU_KERNEL_TAG8 = 3,
  SEDX_GRU_KERNEL_COOP16 = 4,
  SEDX_GRU_KERNEL_AUTO = 5,
  SEDX_GRU_KERNEL_KSPLIT = 6,
  SEDX_GRU_KERNEL_PAIR = 7
};
enum { SEDX_GRU_HANDOFF_AUTO = 0, SEDX_GRU_HANDOFF_GLOBAL = 1, SEDX_GRU_HANDOFF_SPREAD = 2, SEDX_GRU_HANDOFF_LOCAL = 3 };
sedx_status sedx_set_tuning(sedx_handle* h, int32_t knob, int32_t value);

/* Asynchronous failures of forwards already issued: a GRU recurrence whose
 * bounded hand-off spin ran out wrote NaN outputs and set a host-mapped word.
 * Call after the work of the forwards in question has completed (a stream
 * sync, or a device-to-host copy of their outputs): SEDX_EHIP (and
 * sedx_last_error names it) when one of them failed, clearing the word;
 * SEDX_OK otherwise.  Every forward entry point also checks it on entry. */
sedx_status sedx_check_error(sedx_handle* h);

/* Serving with several batches in flight (one stream per request): when on,
 * the conv stack of every forward on this handle starts only after the conv
 * stack of the previously issued forward finished (a device-side event wait,
 * no host sync), so batch i's GRU / MHA + head overlap batch i+1's conv stack
 * instead of two conv stacks splitting the chip.  Results are unchanged;
 * order = host issue order.  Off by default.  on = 2: the same, with block
 * 1's first launch (conv1, HBM-bound) issued before the wait, so it may run
 * beside the previous forward's conv tail (its time then counts in stage 11,
 * pipeline wait). */
sedx_status sedx_set_pipelined(sedx_handle* h, int32_t on);

/* Per-stage device timing (the reference only wall-clocks whole loops,
 * pytorch/main_strong.py:565-574).  When on, every forward records HIP events
 * on its stream at the stage boundaries; sedx_stage_times waits for them and
 * returns milliseconds for: 0 frontend, 1 conv1 of block 1, 2..8 the seven
 * implicit-GEMM convs (b1c2, b2c1, b2c2, b3c1, b3c2, b4c1, b4c2), 9 GRU / MHA
 * incl. projections (~0 for the CNN-only models; the whole Conformer encoder), 10 AttBlock / fc head,
 * 11 pipeline wait: with
 * sedx_set_pipelined on, the stream's wait for the previous forward's conv
 * stack (between the frontend and block 1; ~0 otherwise), so stage 0 times
 * the frontend's own work.  on = 1: the last forward's times;
 * on = 2 (accumulate): every forward records into its own event set (so
 * forwards in flight on several streams time independently) and
 * sedx_stage_times returns per-stage averages over all forwards since the
 * previous call (or since profiling was switched on), then resets them. */
#define SEDX_N_STAGES 12
/* Stage capture (per-stage parity tests): every later forward copies the
 * output of stage `stage` (numbering as above) into d_buf (at most `bytes`),
 * on its stream, in the library's channels-last layout:
 *   0  bn0 output X0                  [items][T][64]
 *   2,4,6  block 1..3 output (pooled) [items][T/2^k][64/2^k][C_k]
 *   3,5,7  conv1 of block 2..4        [items][T'][F'][C]
 *   8  block 4 + freq mean            [items][T/8][512]
 *   9  GRU / MHA output               [items][T/8][512]
 *      (the head's input; CNN-only models: the same contents as stage 8;
 *      Conformer models: the encoder output [items][T/8][144])
 * Conformer models only, capture ids beyond the timing stages (all
 * [items][T/8][144]; SEDX_N_STAGES and the timed stages are unchanged):
 *   20          the encoder's input layer output
 *   21 + 4b + j block b = 0..2: j = 0 after ffn1, 1 after mhsa, 2 after the
 *               conv module, 3 the block's output (after ffn2 and its norm);
 *               32 is the same tensor as 9
 * 14-layer models: 0 and 2..7 as above; 8 is block 4's pooled output
 * [items][T/16][4][512], 9 the GRU / MHA output [items][T/32][2048], and
 *   40  conv1 of block 5              [items][T/16][4][1024]
 *   41  block 5 output (pooled)       [items][T/32][2][1024]
 *   42  conv1 of block 6              [items][T/32][2][2048]
 *   43  block 6 + freq mean           [items][T/32][2048] (the sequence input)
 * Their timed stage 8 spans block 4's conv2 and the four launches of blocks
 * 5-6; stage 9 is the sequence layer alone.  SEDX_MODEL_CNN14_DECISIONLEVELATT
 * has no sequence layer: its 9 is relu(fc1) [items][T/32][2048], computed from
 * 43 by the one pooling + fc1 launch that stage 9 times.
 * The VGGish models (channels-last):
 *    0  log-mel (no bn0)              [items][T][64]
 *   50  conv1 + ReLU + max pool       [items][T/2][32][64]
 *   51  conv2 + ReLU + max pool       [items][T/4][16][128]
 *   52  conv3_1 + ReLU                [items][T/4][16][256]
 *   53  conv3_2 + ReLU + max pool     [items][T/8][8][256]
 *   54  conv4_1 + ReLU                [items][T/8][8][512]
 *   55  conv4_2 + ReLU + max pool, before the mean   [items][T/16][4][512]
 *       (capture-only: one more launch, straight into d_buf, which must hold the whole tensor)
 *    8  the mean of 55's 4 bins       [items][T/16][512] (the sequence input)
 *    9  the GRU output (VGGISH_GRU_FRAMEATT), else the same as 8
 * Their timed stages: 1 conv1, 2..6 the launches 51..54 and 8 in this order, 7
 * and 8 empty, 9 the GRU, 10 the head.
 * stage < 0 or d_buf == NULL switches capture off. */
sedx_status sedx_set_capture(sedx_handle* h, int32_t stage, float* d_buf, size_t bytes);
sedx_status sedx_set_profiling(sedx_handle* h, int32_t on);
sedx_status sedx_stage_times(sedx_handle* h, float* ms, int32_t capacity, int32_t* n_stages);

/* Thresholding into events: activity_detection per (clip, class)
 * (utils/vad.py:11-199) as called by frame_prediction_to_event_prediction_v2
 * (pytorch/predict.py:57-121).  Host-side, quirk-exact.
 *   h_framewise [n_clips, T, C] (host), per-class parameter arrays of length C.
 *   use_low_thres = 0 reproduces activity_detection(low_thres=None).
 * Events are written as int32 quadruples (clip, class, bgn_frame, fin_frame)
 * in (clip, class, time) order; onset = bgn / frames_per_second.  When
 * *n_events > capacity the call returns SEDX_EINVAL with the required count. */
sedx_status sedx_events(const float* h_framewise, int64_t n_clips, int64_t T, int64_t C,
                        const double* high_thres, const double* low_thres,
                        int32_t use_low_thres, const int64_t* n_smooth,
                        const int64_t* n_salt, int32_t* h_events, int64_t capacity,
                        int64_t* n_events);

/* The same thresholding on the GPU, one wavefront per (clip, class) series, no
 * host round trip (asynchronous on `stream`; the device that owns d_x must be
 * current).
 *   mode 0: activity_detection (utils/vad.py:11-45) of framewise
 *           probabilities, exactly as sedx_events;
 *   mode 1: activity_detection_binary (utils/vad.py:47-106) of window vote
 *           counts from sedx_forward_windows_vote, as
 *           frame_binary_prediction_to_event_prediction
 *           (utils/utilities.py:216-276) calls it; high_thres is unused there
 *           (may be NULL), overlap_value (float64, int(100 * overlap_value)
 *           frames per block, vad.py:63) / sample_duration give its blocks.
 *   d_x       [n_clips, T, C] device
 *   d_events  int32 [capacity][4] (clip, class, bgn, fin) in (clip, class,
 *             time) order; events past capacity are dropped
 *   d_info    int64 [2]: total number of events (may exceed capacity), and 1
 *             where the reference raises IndexError (see sedx_events)
 *   d_workspace >= sedx_events_workspace_size(n_clips, T, C) bytes;
 *             T <= 655,360 frames (a series' bitmaps are held in LDS). */
sedx_status sedx_events_workspace_size(int64_t n_clips, int64_t T, int64_t C, size_t* bytes);
sedx_status sedx_events_device(const float* d_x, int64_t n_clips, int64_t T, int64_t C,
                               const double* high_thres, const double* low_thres,
                               int32_t use_low_thres, const int64_t* n_smooth, const int64_t* n_salt,
                               int32_t mode, double overlap_value, int32_t sample_duration,
                               int32_t* d_events, int64_t capacity, int64_t* d_info,
                               void* d_workspace, size_t workspace_bytes, void* stream);

/* Mode 0 of the above over clips of different lengths, as
 * sedx_forward_windows_ragged leaves them: d_x [h_frame_off[n_clips]][C], clip
 * c's rows at h_frame_off[c] (host, [n_clips + 1], non-decreasing).  One
 * wavefront per (clip, class) series; events are (clip, class, bgn, fin) with
 * frames relative to the clip, in (clip, class, time) order; d_info as above.
 * Every clip holds at most 655,360 frames. */
sedx_status sedx_events_ragged_workspace_size(const int64_t* h_frame_off, int64_t n_clips, int64_t C, size_t* bytes);
sedx_status sedx_events_device_ragged(const float* d_x, const int64_t* h_frame_off, int64_t n_clips, int64_t C,
                                      const double* high_thres, const double* low_thres, int32_t use_low_thres,
                                      const int64_t* n_smooth, const int64_t* n_salt, int32_t* d_events,
                                      int64_t capacity, int64_t* d_info, void* d_workspace, size_t workspace_bytes,
                                      void* stream);

/* Threshold calibration (utils/optimize_thresholds.py optimize_sed_thresholds):
 * segment-based true / false positive and false negative counts of
 * activity_detection (mode 0 above, always with the low threshold) for V
 * threshold variants at once, without materialising event lists.  Every event
 * (bgn, fin) of a (clip, class) series sets segments [bgn / segment_frames,
 * ceil(fin / segment_frames)); the set is compared with the series' target
 * mask: tp = |est & ref|, fp = |est & ~ref|, fn = |ref & ~est|, summed over
 * clips.  `bad` counts the series where the reference raises IndexError (see
 * the events entry points); such a series adds nothing to tp / fp / fn.
 *   S = ceil(T / segment_frames) <= 64, segment_frames >= 1, 1 <= V <= 64;
 *   anything else returns SEDX_EINVAL and sedx_last_error(NULL) names the
 *   reason (a per-thread message of these handle-free entry points).
 *   target  uint64 [n_clips][C]: bit s = class active in segment s
 *   high / low  float64 [V][C] (host), rounded to float32 for the compares
 *   counts  int64 [V][C][4] = (tp, fp, fn, bad), overwritten
 * The device version is asynchronous on `stream` (the device that owns d_x
 * must be current), zeroes d_counts itself and needs
 * sedx_segment_counts_workspace_size bytes of workspace. */
sedx_status sedx_segment_counts(const float* h_x, int64_t n_clips, int64_t T, int64_t C,
                                const uint64_t* h_target, int64_t segment_frames, int64_t V,
                                const double* high, const double* low,
                                const int64_t* n_smooth, const int64_t* n_salt, int64_t* h_counts);
sedx_status sedx_segment_counts_workspace_size(int64_t n_clips, int64_t T, int64_t C, int64_t V, size_t* bytes);
sedx_status sedx_segment_counts_device(const float* d_x, int64_t n_clips, int64_t T, int64_t C,
                                       const uint64_t* d_target, int64_t segment_frames, int64_t V,
                                       const double* high, const double* low,
                                       const int64_t* n_smooth, const int64_t* n_salt,
                                       int64_t* d_counts, void* d_workspace, size_t workspace_bytes, void* stream);

/* Average precision (pytorch/evaluate.py:24, :76 call
 * sklearn.metrics.average_precision_score: the non-interpolated AP), per class,
 * as a ranking: a segmented radix sort on the device (csrc/rank.hip), a stable
 * sort on the host (csrc/rank_host.cpp).  For one class with M samples, float32
 * scores s_i and labels y_i (target != 0):
 *   ordering    by float32 VALUE, descending, compared as numbers: -0.0 and
 *               +0.0 are one threshold; distinct denormals are distinct
 *               thresholds (nothing is flushed)
 *   thresholds  t_1 > ... > t_K the distinct values; n_k = #{i : s_i >= t_k},
 *               tp_k = #{i : s_i >= t_k, y_i = 1}, tp_0 = 0, P = tp_K
 *   AP          sum over k = 1..K of
 *                 ((double)(tp_k - tp_{k-1}) / (double)P) * ((double)tp_k / (double)n_k)
 *               in float64, in ONE order, the same on the host and the device
 *               and independent of C, of the class's column and of any launch
 *               geometry: 64 consecutive terms (k = 64 q + 1 .. 64 q + 64,
 *               missing ones +0.0) are added by the tree a[j] += a[j + off],
 *               off = 32, 16, 8, 4, 2, 1; 64 consecutive such sums by the same
 *               tree; the resulting sums (one per 4096 terms) in ascending
 *               order, starting from +0.0.  The order of equal scores among
 *               themselves never matters: the curve is read only at the end
 *               of each run of equal scores.
 *   P = 0       AP = NaN: the reference's environment (Python 3.7) has an
 *               sklearn that divides 0 / 0 there, which is why it takes
 *               np.nanmean (main_strong.py:313-323); recent sklearn returns
 *               0.0 with a warning instead.  info still holds (0, K, 0).
 *   non-finite  sklearn raises ValueError for NaN / +-inf scores.  Here a class
 *               with any has AP = NaN, K = 0, no curve written, and its count
 *               in info; the other classes are unaffected.  The host entry
 *               then returns SEDX_EINVAL (all outputs are filled) and the
 *               message counts them; the device entry is asynchronous and
 *               returns SEDX_OK: its caller reads info.
 *   scores  float32 [M][C], target uint8 [M][C], as they lie, class fastest
 *           (a framewise [N][T][C] tensor is [N T][C])
 *   ap      float64 [C]
 *   info    int64 [C][3] = (P, K, number of non-finite scores)
 *   thr / tp / n   optional curve, all three or none (NULL): float32 / int32 /
 *           int32 [C][M], the first K of each row valid: t_k descending (a
 *           zero threshold as +0.0), tp_k, n_k
 * 1 <= M < 2^31 and 1 <= C <= 65535; anything else, a null pointer or a
 * workspace smaller than the size query's answer returns SEDX_EINVAL with a
 * per-thread message (the handle-free message of sedx_last_error).  The device
 * entry is asynchronous on `stream` (the device that owns the pointers must be
 * current), never synchronises and zeroes what it accumulates.  Classes are
 * ranked in groups of max(1, min(C, 2^22 / M)) so the workspace stays bounded:
 * about 14 bytes per (sample, class of a group) plus 1 KiB per (tile, class of
 * a group).  The tile is the number of keys one workgroup takes per radix pass
 * (tests aim at its boundaries). */
sedx_status sedx_average_precision(const float* h_scores, const uint8_t* h_target, int64_t M, int64_t C,
                                   double* h_ap, int64_t* h_info,
                                   float* h_thr, int32_t* h_tp, int32_t* h_n);
sedx_status sedx_average_precision_workspace_size(int64_t M, int64_t C, size_t* bytes);
sedx_status sedx_average_precision_device(const float* d_scores, const uint8_t* d_target, int64_t M, int64_t C,
                                          double* d_ap, int64_t* d_info,
                                          float* d_thr, int32_t* d_tp, int32_t* d_n,
                                          void* d_workspace, size_t workspace_bytes, void* stream);
int64_t sedx_rank_tile(void);

/* ------------------------------------------------------------------------
 * Input side: librosa.core.load(path, sr, mono=True) as
 * pytorch/predict.py:295 and pytorch/main_strong.py:787 call it
 * (librosa 0.8: soundfile read -> to_mono -> resample(res_type='kaiser_best')
 * -> fix_length).  Handle-free; asynchronous on `stream`.
 * ------------------------------------------------------------------------ */
typedef enum { SEDX_WAV_PCM = 1, SEDX_WAV_FLOAT = 3 } sedx_wav_format;
typedef struct {
  int32_t format;           /* sedx_wav_format */
  int32_t channels;
  int32_t sample_rate;
  int32_t bits_per_sample;  /* PCM 8/16/24/32, float 32/64 */
  int64_t frames;
  int64_t data_offset;      /* byte offset of the interleaved samples in the file */
  int64_t data_bytes;
} sedx_wav_info;
/* Parse a RIFF/WAVE file image in host memory (PCM or IEEE float, including
 * WAVE_FORMAT_EXTENSIBLE).  SEDX_EINVAL for anything else. */
sedx_status sedx_wav_parse(const void* h_bytes, size_t n_bytes, sedx_wav_info* info);
/* Interleaved samples (a device copy of the data chunk) -> mono float32
 * d_out [frames]: libsndfile's float scaling, then the mean over channels
 * (librosa.to_mono on the float32 array). */
sedx_status sedx_wav_decode_mono(const void* d_data, const sedx_wav_info* info, float* d_out, void* stream);
typedef enum { SEDX_RESAMPLE_KAISER_BEST = 0, SEDX_RESAMPLE_KAISER_FAST = 1 } sedx_resample_quality;
/* librosa.resample(y, sr_in, sr_out, res_type) length: ceil(n_in * sr_out / sr_in). */
sedx_status sedx_resample_size(int64_t n_in, int32_t sr_in, int32_t sr_out, int64_t* n_out);
sedx_status sedx_resample_workspace_size(int64_t n_in, int32_t sr_in, int32_t sr_out, int32_t quality,
                                         size_t* bytes);
/* resampy band-limited interpolation (restated; resampy is not in the
 * reference) + librosa fix_length; a device copy when sr_in == sr_out. */
sedx_status sedx_resample(const float* d_in, int64_t n_in, int32_t sr_in, int32_t sr_out, int32_t quality,
                          float* d_out, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEDX_H */
