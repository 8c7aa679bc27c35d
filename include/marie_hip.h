/*
 * marie_hip.h — C ABI of libmarie_hip.so, the MI355X (gfx950) OCR hot path.
 *
 * The reference (gregbugaj/marie-icr) has NO FFI on this path: its boundary is
 * three Python abstract classes.  This header is the C boundary
 * the Python mirrors of those classes (the marie_icr_amd Python package) bind with ctypes; each
 * entry point names the reference code it replaces.
 *
 * Conventions
 *   - every function returns 0 on success or a negative MHIP_E* code; nothing
 *     throws across the ABI; mhip_last_error(ctx) holds the message.
 *   - plain pointers and sizes only.  "_dev" pointers are device (HBM) addresses,
 *     "_host" pointers are host addresses; the caller owns both.
 *   - one ctx per (process, GPU); a ctx and its models are NOT thread-safe.
 *   - device entry points enqueue on the ctx stream (mhip_set_stream) and return
 *     without synchronising; *_host entry points synchronise before returning.
 */
#ifndef MARIE_HIP_H
#define MARIE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHIP_OK 0
#define MHIP_EINVAL (-22)  /* bad argument / shape */
#define MHIP_ENOMEM (-12)  /* device allocation failed */
#define MHIP_EHIP (-5)     /* HIP runtime error (see mhip_last_error) */
#define MHIP_ESTATE (-1)   /* call order violated (e.g. forward before finalize) */

/* arithmetic type of the recognizer's conv/GEMM contractions */
#define MHIP_PREC_F16 0 /* f16 operands, fp32 MFMA accumulate (v_mfma_f32_16x16x32_f16)   */
#define MHIP_PREC_F32 1 /* exact fp32 operands and accumulate (v_mfma_f32_16x16x4_f32)    */

typedef struct mhip_ctx mhip_ctx;
typedef struct mhip_crnn mhip_crnn;

/* ---- context ------------------------------------------------------------------------ */
/* replaces: device selection in marie/models/utils.py:initialize_device_settings and the
 * per-processor `.to(device)` calls (marie/document/craft_ocr_processor.py:142-146).     */
int mhip_init(int device_id, mhip_ctx** out);
int mhip_destroy(mhip_ctx* ctx);
const char* mhip_last_error(mhip_ctx* ctx);
/* hipStream_t to enqueue on (NULL = the null stream).  The caller keeps it alive. */
int mhip_set_stream(mhip_ctx* ctx, void* hip_stream);
int mhip_synchronize(mhip_ctx* ctx);
/* "gfx950", CU count and HBM bytes of the bound device */
int mhip_device_info(mhip_ctx* ctx, char* arch, size_t arch_len, int* cu_count, size_t* hbm_bytes);
/* Device-to-device copy on the ctx stream (e.g. weight arena <-> an RCCL broadcast buffer). */
int mhip_memcpy_dev(mhip_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);

/* Phase gate: orders two streams that are fed by two host threads.  replaces: nothing in the reference — its page loop is
 * serial (marie/ocr/ocr_engine.py:172-221: detect, then recognize, page by page); here the detector of page batch k + 1 runs
 * under the HBM-bound decode phase of the recognizer of batch k, and the gate is where that phase starts.
 *   mhip_gate_signal  records an event on ctx's stream and counts it (signal n);
 *   mhip_gate_wait    blocks the calling thread until signal `seq` exists (at most timeout_ms), then makes ctx's stream wait
 *                     for it: returns 1 (stream ordered), 0 (gate open or timed out: the caller proceeds unordered), < 0 error;
 *   mhip_gate_open    1: every present and future wait returns 0 at once (error / shutdown path), 0: closes it again.      */
typedef struct mhip_gate mhip_gate;
int mhip_gate_create(mhip_ctx* ctx, mhip_gate** out);
int mhip_gate_destroy(mhip_gate* g);
int mhip_gate_signal(mhip_gate* g, mhip_ctx* ctx);
long long mhip_gate_count(mhip_gate* g);
int mhip_gate_open(mhip_gate* g, int open);
int mhip_gate_wait(mhip_gate* g, mhip_ctx* ctx, long long seq, int timeout_ms);

/* Per-kernel timing with HIP events on the ctx stream (bench.py's roofline leg).
 * replaces: marie/logging_core/profile.py TimeContextCuda around model calls.
 * While enabled every kernel launch is bracketed by an event pair; mhip_profile_read
 * synchronises and returns the accumulated device time and launch count of one kernel id. */
int mhip_profile_enable(mhip_ctx* ctx, int enable);
int mhip_profile_reset(mhip_ctx* ctx);
int mhip_profile_read(mhip_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);
/* Algorithmic FLOPs (2*MAC) of the launches of an MFMA kernel id timed since the last reset (0 for HBM-bound ids). */
int mhip_profile_flops(mhip_ctx* ctx, int kernel_id, double* flops);
int mhip_kernel_count(void);
const char* mhip_kernel_name(int kernel_id);

/* ---- NHWC convolution / GEMM primitive -------------------------------------------------- */
/* replaces: every nn.Conv2d (+ folded BatchNorm2d + ReLU + MaxPool2d) and nn.Linear on the path,
 * e.g. marie/models/icr/modules/feature_extraction.py:13-25, marie/models/craft/craft.py:14-28,
 * marie/models/craft/basenet/vgg16_bn.py:23-74.
 *   out[b][yp][xp][n] = pool( act( scale[n] * sum_{dy,dx,c} in[b][y+dy-pad][x+dx-pad][c] * w[n][dy][dx][c] + bias[n] ) )
 * in/w/out element type = precision (f16 or f32); out is fp32 when out_f32 != 0.  Stride 1, zero padding.
 * Cin must be a multiple of 64 (f16) / 32 (f32).  pool: 0 none, 1 = 2x2/2 (floor), 2 = (2,1)/(2,1). */
typedef struct mhip_conv_desc {
  int32_t B, H, W, Cin; /* input  [B][H][W][Cin] */
  int32_t KH, KW, pad;  /* filter [N][KH][KW][Cin] */
  int32_t N;            /* output channels */
  int32_t pool, relu, out_f32;
  int32_t dil;          /* filter dilation, 0/1 = dense */
  int32_t Cin1;         /* with in2_dev: channels [0,Cin1) come from in_dev, [Cin1,Cin) from in2_dev */
  int32_t ldc;          /* output row pitch in elements, 0 = N (rows must stay 16-byte aligned; unpooled outputs only)        */
  int32_t pad_cols_writable; /* 1: columns [N, roundup(N, 8)) of a pitched row are the call's own and may be zeroed          */
} mhip_conv_desc;
/* in2_dev (may be NULL) is the second tensor of a channel-concatenated input, torch.cat([a, b], dim=1) followed
 * by a 1x1 conv (marie/models/craft/craft.py:63-64,67-69): the concatenation is never materialised.      */
int mhip_conv2d_nhwc(mhip_ctx* ctx, int precision, const mhip_conv_desc* d, const void* in_dev,
                     const void* in2_dev, const void* w_dev, const float* scale_dev, const float* bias_dev,
                     void* out_dev);
/* The same primitive with every option of the plain epilogue that the model paths use (the ResNet blocks of the attention
 * recognizer, the overlay generator's down-sampling convs, the fp32 patch embeddings), for parity tests of each of them:
 *   out[row(b, yp, xp)][n] = pool( relu( scale[n] * sum_{dy,dx,c} in[b][y*sy + dy*dil - pad][x + dx*dil - pad_x][c] * w[n][dy][dx][c]
 *                                        + bias[n] + res[res_row][n] ) )
 * sy: vertical stride (0 = 1; the horizontal stride is 1).  pad_x: horizontal padding, -1 = pad.  res_dev (may be NULL): a residual of
 * the output's element type and row pitch, added before the ReLU (unpooled outputs; not with GELU).  row_period > 0 (unpooled):
 * output pixel q is written to row (q / row_period) * row_stride + row_offset + q % row_period and takes residual row
 * q % row_period; row_stride >= row_period.  The first fifteen fields are those of mhip_conv_desc, in its order.               */
typedef struct mhip_conv_ex_desc {
  int32_t B, H, W, Cin;
  int32_t KH, KW, pad;
  int32_t N;
  int32_t pool, relu, out_f32;
  int32_t dil;
  int32_t Cin1;
  int32_t ldc;
  int32_t pad_cols_writable;
  int32_t sy;
  int32_t pad_x;
  int32_t row_period, row_stride, row_offset;
  const void* res_dev;
} mhip_conv_ex_desc;
int mhip_conv2d_nhwc_ex(mhip_ctx* ctx, int precision, const mhip_conv_ex_desc* d, const void* in_dev,
                        const void* in2_dev, const void* w_dev, const float* scale_dev, const float* bias_dev,
                        void* out_dev);

/* ---- crop batcher --------------------------------------------------------------------------- */
/* One text fragment inside a device buffer: first pixel at base + src_offset, h rows of w pixels, `channels` = 3
 * (BGR, OpenCV order) or 1 (gray), rows row_stride bytes apart (a fragment may be a window of a whole page). */
typedef struct mhip_crop_desc {
  uint64_t src_offset;
  int32_t h, w, row_stride, channels;
} mhip_crop_desc;
/* replaces: MemoryDataset.__getitem__ (BGR -> RGB -> PIL "L", marie/models/icr/memory_dataset.py:40-55) and
 * AlignCollate/NormalizePAD with keep_ratio_with_pad (marie/models/icr/dataset.py:275-324): every fragment becomes a
 * 32 x img_w uint8 line — Pillow-exact bicubic resize to height 32 keeping the aspect ratio (width capped at img_w),
 * last column replicated.  out_dev: uint8 [n][32][img_w].  Scratch comes from the ctx workspace.              */
int mhip_crop_batch(mhip_ctx* ctx, const uint8_t* base_dev, const mhip_crop_desc* descs_host, int n, int img_w,
                    uint8_t* out_dev);

/* ---- CRNN-family recognizer: None-VGG-BiLSTM-CTC ---------------------------------- */
/* replaces: Model(opt) construction, marie/models/icr/model.py:27-68 (Trans=None, Feat=VGG,
 * Seq=BiLSTM, Pred=CTC; imgH=32, input_channel=1, output_channel=512, hidden_size=256).  */
int mhip_crnn_create(mhip_ctx* ctx, int precision, int num_class, mhip_crnn** out);
int mhip_crnn_destroy(mhip_crnn* m);

/* replaces: model.load_state_dict(torch.load(...)), marie/document/craft_ocr_processor.py:146.
 * `key` is the reference state_dict key ("FeatureExtraction.ConvNet.0.weight", ... an optional
 * "module." prefix is ignored); `data` is host fp32 in the checkpoint's own layout
 * (conv: [Cout][Cin][kh][kw]; LSTM/Linear: [out][in]).  Unknown keys return MHIP_EINVAL,
 * "num_batches_tracked" is accepted and ignored.                                          */
int mhip_crnn_set_tensor(mhip_crnn* m, const char* key, const float* data_host, const int64_t* shape, int ndim);
/* Repack every tensor into the kernels' layouts (NHWC taps, BN folded to scale/shift, LSTM
 * gates in MFMA-fragment order) inside ONE device arena and upload it.  Fails with MHIP_ESTATE
 * if any tensor is missing.                                                                */
int mhip_crnn_finalize(mhip_crnn* m);
/* Allocate the (identically laid out) arena without filling it — for ranks that receive the
 * weights by an RCCL broadcast of the arena instead of reading a checkpoint.              */
int mhip_crnn_alloc_arena(mhip_crnn* m);
int mhip_crnn_arena(mhip_crnn* m, void** arena_dev, size_t* bytes);

/* T (time steps) for a crop of width w: w/4 - 1 (VGG stack, imgH = 32). */
int mhip_crnn_seq_len(int w);

/* Forward + greedy CTC decode of n pre-cropped grayscale lines, all 32 x w (w % 4 == 0, w >= 8).
 * replaces: AlignCollate's ToTensor/normalise for a full-width crop
 * (marie/models/icr/dataset.py:275-283), model(image, text_for_pred)
 * (marie/document/craft_ocr_processor.py:236-237), preds.max(2) (:240),
 * CTCLabelConverter.decode (marie/models/icr/utils.py:41-54) and the confidence
 * softmax/max/cumprod (:255-271).
 *   crops_dev   uint8  [n][32][w]
 *   logits_dev  fp32   [n][T][num_class]          or NULL
 *   argmax_dev  int32  [n][T]      raw per-step argmax (first max on ties)
 *   tokens_dev  int32  [n][T]      collapsed sequence (blank and repeats removed), 0-padded
 *   lengths_dev int32  [n]         number of valid tokens per line
 *   conf_dev    fp32   [n]         product over all T steps of the max softmax probability */
int mhip_crnn_forward(mhip_crnn* m, const uint8_t* crops_dev, int n, int w, float* logits_dev,
                      int32_t* argmax_dev, int32_t* tokens_dev, int32_t* lengths_dev, float* conf_dev);
/* Same with host buffers: H2D of the crops, forward, D2H of the outputs, stream sync. */
int mhip_crnn_forward_host(mhip_crnn* m, const uint8_t* crops_host, int n, int w, float* logits_host,
                           int32_t* argmax_host, int32_t* tokens_host, int32_t* lengths_host,
                           float* conf_host);
/* Crop batcher + forward + decode in one call: fragments described inside base_dev (e.g. word boxes on a page
 * that is already in HBM) -> host outputs.  replaces: CraftOcrProcessor.recognize_from_fragments' DataLoader +
 * model + decode loop (marie/document/craft_ocr_processor.py:184-286).                                        */
int mhip_crnn_forward_crops(mhip_crnn* m, const uint8_t* base_dev, const mhip_crop_desc* descs_host, int n, int img_w,
                            float* logits_host, int32_t* argmax_host, int32_t* tokens_host, int32_t* lengths_host,
                            float* conf_host);
/* Same with the fragments packed back to back in a HOST buffer (src_offset relative to packed_host). */
int mhip_crnn_forward_fragments_host(mhip_crnn* m, const uint8_t* packed_host, size_t packed_bytes,
                                     const mhip_crop_desc* descs_host, int n, int img_w, float* logits_host,
                                     int32_t* argmax_host, int32_t* tokens_host, int32_t* lengths_host,
                                     float* conf_host);
/* Bytes of ctx workspace mhip_crnn_forward of n lines of width w carves: exactly its layout's sizing pass. */
size_t mhip_crnn_workspace_bytes(mhip_crnn* m, int n, int w);
/* Algorithmic FLOPs (2*MAC) of one forward of n lines of width w, per kernel id — what
 * bench.py divides by the measured kernel time for the roofline line.                    */
double mhip_crnn_kernel_flops(mhip_crnn* m, int kernel_id, int n, int w);

/* The BiLSTM recurrence alone (one layer, both directions) on host inputs, through the weight packers and the launcher of the
 * CRNN and ICR recognizers.  replaces: the recurrent part of nn.LSTM(input, 256, bidirectional=True, batch_first=True),
 * marie/models/icr/modules/sequence_modeling.py:8,17 (h0 = c0 = 0), everything in PyTorch's own order:
 *   whh    fp32 [2][1024][256]     weight_hh_l0, weight_hh_l0_reverse (gate rows i, f, g, o)
 *   xproj  fp32 [B][T][2][1024]    x_t W_ih^T + b_ih + b_hh of the forward, then the reverse direction, gate-major
 *   out    fp32 [B + 16][T][512]   h of the forward | reverse direction (f16 widened in the f16 mode).  The device buffer carries
 *                                  16 guard rows (one workgroup tile) behind row B, is filled with 0xff bytes before the launch and
 *                                  comes back whole: a cell never written, or a write past row B, shows (f16 0xffff widens to NaN). */
int mhip_lstm_rec_host(mhip_ctx* ctx, int precision, int B, int T, const float* whh, const float* xproj, float* out);

/* ---- stage entries of the recognizer's non-GEMM kernels (csrc/icr_ops.hip) ------------------------------------------------
 * One kernel each on host buffers, through the launcher the ICR model calls (its argument checks and grid choice included);
 * no model, no weights beyond the arguments.  Conventions of all of them, and of the detector's below:
 *   - activations are fp32 on the host; in the f16 mode they are narrowed to f16 on the way in and widened on the way out
 *     (f16-representable values pass exactly).  Weights, scales, biases, scores and indices stay as they are.
 *   - every output buffer holds MHIP_STAGE_GUARD elements behind the n the launch owns.  The device copy is filled with 0xff
 *     bytes before the launch and comes back whole: a cell never written, or a write past the end, shows (f16 0xffff widens
 *     to the fp32 NaN 0xffffe000).  A refused call writes nothing.                                                        */
#define MHIP_STAGE_GUARD 4096   /* elements: one workgroup's output of the widest kernel (64 pixels x 64 channels) */
/* replaces: nn.Conv2d(1, C, 3, 1, 1, bias=False) + BatchNorm2d (folded: scale, bias) + ReLU, transformation.py:52-53,
 * feature_extraction.py:161-163.  img u8 [B][H][W] (normalised to [-1, 1] on the fly) or fp32 [B][H][W]; w9xC fp32 [9][C]
 * (tap dy*3+dx major); out [B*H*W*64 + guard], NHWC with 64 channels, channels >= C zero. */
int mhip_conv_gray_first_host(mhip_ctx* ctx, int precision, int in_is_u8, const void* img, int B, int H, int W, int C,
                              const float* w9xC, const float* scale, const float* bias, float* out);
/* replaces: nn.MaxPool2d(kernel_size=2, stride=(2, 1), padding=(0, 1)), feature_extraction.py:180.
 * in [B][H][W][C] -> out [B][H/2][W+1][C] + guard */
int mhip_maxpool_s21_p01_host(mhip_ctx* ctx, int precision, const float* in, int B, int H, int W, int C, float* out);
/* replaces: nn.AdaptiveAvgPool2d(1), transformation.py:61.  in [B][HW][C] -> out [B][C] + guard */
int mhip_avgpool_hw_host(mhip_ctx* ctx, int precision, const float* in, int B, int HW, int C, float* out);
/* replaces: GridGenerator.build_P_prime + F.grid_sample(padding_mode="border", align_corners=True), transformation.py:32-42,
 * 158-167.  crops u8 [B][H][W], cprime fp32 [B][F][2], inv_delta_c fp32 [F+3][F+3], p_hat fp32 [H*W][F+3] -> out fp32
 * [B][H][W] + guard (the rectified, normalised crop) */
int mhip_tps_sample_host(mhip_ctx* ctx, const uint8_t* crops, const float* cprime, const float* inv_delta_c,
                         const float* p_hat, int B, int H, int W, int F, float* out);
/* replaces: AttentionCell's e = score(tanh(i2h(H) + h2h(h))), alpha = softmax(e, dim=1), context = alpha^T H, prediction.py:
 * 72-79.  hproj fp32 [B][T][256] = i2h(H); hp fp32 [B][ld_hp], columns 0..255 = h2h(h) + bias (ld_hp >= 256); score_w fp32
 * [256]; H activations [B][T][256] -> ctx_out [B][256] + guard */
int mhip_attn_context_host(mhip_ctx* ctx, int precision, const float* hproj, const float* hp, int ld_hp,
                           const float* score_w, const float* H, int B, int T, float* ctx_out);
/* replaces: nn.LSTMCell(256 + num_class, 256) on [context, one_hot(char)], prediction.py:80-82.  gctx fp32 [B][1024] =
 * W_ih[:, :256] context; ghid fp32 [B][ld_hp], columns 256..1279 = W_hh h + b_ih + b_hh (ld_hp >= 1280); w_onehot fp32
 * [num_class][1024] = W_ih[:, 256:]^T; chars int32 [B] in [0, num_class) (checked here: the kernel does not);
 * c fp32 [B][256] + guard, updated in place; h [B][256] + guard */
int mhip_attn_cell_host(mhip_ctx* ctx, int precision, const float* gctx, const float* ghid, int ld_hp,
                        const float* w_onehot, int num_class, const int32_t* chars, int B, float* c, float* h);
/* replaces: `_, next_input = probs_step.max(1)`, prediction.py:57-59.  logits fp32 [B][ld], the first C columns of a row
 * count -> idx int32 [B] + guard = torch.max(x, 1).indices (first maximum; first NaN if any; 0 for a row of -inf) */
int mhip_argmax_rows_host(mhip_ctx* ctx, const float* logits, int ld, int C, int B, int32_t* idx);
/* replaces: preds_prob = F.softmax(preds, dim=2); preds_prob.max(dim=2), craft_ocr_processor.py:259-262.  logits fp32
 * [rows][C] -> idx int32 [rows] + guard as above, pmax fp32 [rows] + guard = softmax probability at idx */
int mhip_rowmax_softmax_host(mhip_ctx* ctx, const float* logits, int rows, int C, int32_t* idx, float* pmax);

/* ---- production ICR recognizer: TPS-ResNet-BiLSTM-Attn ---------------------------------------- */
typedef struct mhip_icr mhip_icr;
/* replaces: Model(opt) with Transformation="TPS", FeatureExtraction="ResNet", SequenceModeling="BiLSTM",
 * Prediction="Attn" as configured by CraftOcrProcessor (marie/document/craft_ocr_processor.py:49-70,103-146): imgH 32,
 * imgW 100, 20 fiducial points, hidden 256, batch_max_length 48 (49 decode steps), num_class = 94 chars + [GO] + [s].
 * Keys are the reference state_dict names ("Transformation.LocalizationNetwork.conv.0.weight", ...,
 * "Transformation.GridGenerator.P_hat", "FeatureExtraction.ConvNet.layer3.4.bn2.running_var", ...,
 * "Prediction.attention_cell.rnn.weight_ih", "Prediction.generator.bias"; a "module." prefix is ignored).          */
int mhip_icr_create(mhip_ctx* ctx, int precision, int num_class, mhip_icr** out);
int mhip_icr_destroy(mhip_icr* m);
int mhip_icr_set_tensor(mhip_icr* m, const char* key, const float* data_host, const int64_t* shape, int ndim);
int mhip_icr_finalize(mhip_icr* m);
int mhip_icr_alloc_arena(mhip_icr* m);
int mhip_icr_arena(mhip_icr* m, void** arena_dev, size_t* bytes);
int mhip_icr_steps(void); /* 49 */
/* replaces: model(image, text_for_pred, is_train=False) (craft_ocr_processor.py:245): TPS rectification
 * (marie/models/icr/modules/transformation.py:32-42), ResNet-45 (feature_extraction.py:212-246), BiLSTM x2, and the
 * 49-step greedy attention decoder (prediction.py:47-61,72-83).  crops_dev uint8 [n][32][100] (already resized and
 * padded, e.g. by mhip_crop_batch with img_w = 100).  Outputs: logits fp32 [n][49][num_class]; argmax int32 [n][49];
 * pmax fp32 [n][49] = softmax probability of the arg-max (for the confidence product); rectified fp32 [n][32][100] or
 * NULL.  The [s]-cut / confidence rule (craft_ocr_processor.py:259-271) is the caller's, as in the reference.       */
int mhip_icr_forward(mhip_icr* m, const uint8_t* crops_dev, int n, float* logits_dev, int32_t* argmax_dev,
                     float* pmax_dev, float* rectified_dev);
int mhip_icr_forward_host(mhip_icr* m, const uint8_t* crops_host, int n, float* logits_host, int32_t* argmax_host,
                          float* pmax_host, float* rectified_host);

/* ---- CRAFT text detector -------------------------------------------------------------------- */
typedef struct mhip_craft mhip_craft;
/* replaces: CRAFT() + load_state_dict(copyStateDict(torch.load(...))), marie/boxes/craft_box_processor.py:260-285.
 * Keys are CRAFT.state_dict() names ("basenet.slice1.0.weight", "upconv1.conv.0.weight", "conv_cls.8.bias", ...;
 * a "module." prefix is ignored).                                                                           */
int mhip_craft_create(mhip_ctx* ctx, int precision, mhip_craft** out);
int mhip_craft_destroy(mhip_craft* m);
int mhip_craft_set_tensor(mhip_craft* m, const char* key, const float* data_host, const int64_t* shape, int ndim);
int mhip_craft_finalize(mhip_craft* m);
int mhip_craft_alloc_arena(mhip_craft* m);
int mhip_craft_arena(mhip_craft* m, void** arena_dev, size_t* bytes);
/* replaces: resize_aspect_ratio's size arithmetic, marie/models/craft/imgproc.py:45-71.
 * (h, w) page -> ratio, resized (th, tw), /32 canvas (H32, W32); the score maps are H32/2 x W32/2.          */
int mhip_craft_geometry(int h, int w, int canvas_size, double mag_ratio, double* ratio, int* th, int* tw,
                        int* H32, int* W32);
/* Bytes of ctx workspace mhip_craft_forward of an h x w page carves: exactly its layout's sizing pass. */
size_t mhip_craft_workspace_bytes(mhip_craft* m, int h, int w, int canvas_size, double mag_ratio);
/* Algorithmic FLOPs (2*MAC over the checkpoint's real channel counts) of one forward of an h x w page, per kernel id. */
double mhip_craft_kernel_flops(mhip_craft* m, int kernel_id, int h, int w, int canvas_size, double mag_ratio);
/* replaces: get_prediction's resize + normalizeMeanVariance + net(x), craft_box_processor.py:94-110.
 * page_dev uint8 [h][w][3] (channel order as given, the reference feeds BGR) -> scores_dev fp32 [H32/2][W32/2][2]
 * (channel 0 = text/region score, 1 = link/affinity score).                                                  */
int mhip_craft_forward(mhip_craft* m, const uint8_t* page_dev, int h, int w, int canvas_size, double mag_ratio,
                       float* scores_dev);
/* replaces: get_prediction incl. getDetBoxes_core (marie/models/craft/craft_utils.py:25-98): forward, threshold,
 * 4-connected components with statistics (GPU), then per component dilate + minAreaRect + diamond fix + clockwise
 * order.  boxes_host gets n_boxes x 4 corners x (x, y) fp32 in SCORE-MAP coordinates, in OpenCV label order
 * (adjustResultCoordinates is the caller's, as in the reference).  scores_host (may be NULL) receives the maps. */
int mhip_craft_detect(mhip_craft* m, const uint8_t* page_dev, int h, int w, int canvas_size, double mag_ratio,
                      float text_threshold, float link_threshold, float low_text, float* boxes_host,
                      int max_boxes, int* n_boxes, float* scores_host, double* ratio_out);
int mhip_craft_detect_host(mhip_craft* m, const uint8_t* page_host, int h, int w, int canvas_size,
                           double mag_ratio, float text_threshold, float link_threshold, float low_text,
                           float* boxes_host, int max_boxes, int* n_boxes, float* scores_host, double* ratio_out);
/* Stage entry: the post-processing of mhip_craft_detect alone (the same code) on a caller-supplied score map, host fp32
 * [H][W][2] (text, link); needs no model.  boxes as above.  Optional read-backs of the labelling (each may be NULL):
 * labels_host int32 [H*W] (0 = background, components numbered in raster order of their first pixel), flags_host uint8
 * [H*W] (1 = text > low_text, 2 = link > link_threshold), stats_host int32 [stats_cap][6] = left, top, right, bottom,
 * area, max text score as raw float32 bits, rows 1..n_labels-1 (row 0, the background, is zero).  n_labels counts the
 * background; stats_cap < n_labels is MHIP_EINVAL, with n_boxes and n_labels valid and no read-back buffer written. */
int mhip_craft_boxes_host(mhip_ctx* ctx, const float* scores_host, int H, int W, float text_threshold,
                          float link_threshold, float low_text, float* boxes_host, int max_boxes, int* n_boxes,
                          int32_t* labels_host, uint8_t* flags_host, int32_t* stats_host, int stats_cap, int* n_labels);

/* ---- stage entries of the detector's image kernels (csrc/image_ops.hip) -----------------------------------------------------
 * Same conventions as the recognizer's stage entries above (MHIP_STAGE_GUARD elements behind every output). */
/* replaces: cv2.resize(img, (dw, dh), interpolation=cv2.INTER_LINEAR), imgproc.py:58; the coefficient tables are built as
 * mhip_craft_forward builds them.  src u8 [sh][sw][3] -> dst u8 [dh][dw][3] + guard */
int mhip_resize_linear_u8_host(mhip_ctx* ctx, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw);
/* replaces: normalizeMeanVariance + canvas padding + basenet features[0..2] (conv3x3 3 -> 64, folded BatchNorm, ReLU),
 * imgproc.py:26-33,61-66, basenet/vgg16_bn.py:29.  img u8 [th][tw][3] top-left on an [H][W] canvas; w27x64 fp32 [27][64]
 * (k = (dy*3+dx)*3 + c) -> out [H][W][64] + guard.  f16 mode: the MFMA kernel */
int mhip_conv_rgb_first_host(mhip_ctx* ctx, int precision, const uint8_t* img, int th, int tw, int H, int W,
                             const float* w27x64, const float* scale, const float* bias, float* out);
/* replaces: nn.MaxPool2d(2, 2) (k = 2, sizes floor) and nn.MaxPool2d(3, 1, 1) (k = 3), basenet/vgg16_bn.py:27-43.
 * in [B][H][W][C] -> out [B][Ho][Wo][C] + guard */
int mhip_maxpool_host(mhip_ctx* ctx, int precision, int k, const float* in, int B, int H, int W, int C, float* out);
/* replaces: F.interpolate(size=(Ho, Wo), mode='bilinear', align_corners=False), craft.py:67-75.
 * in [B][Hi][Wi][C] -> out [B][Ho][Wo][C] + guard */
int mhip_upsample_bilinear_host(mhip_ctx* ctx, int precision, const float* in, int B, int Hi, int Wi, int C, int Ho, int Wo,
                                float* out);
/* replaces: conv_cls[6..8] = ReLU(conv1x1 16 -> 16), conv1x1 16 -> 2, craft.py:46-49.  in [npix][in_stride] activations, the
 * first 16 channels of a line count (in_stride a multiple of 8); w1 [16][16], b1 [16], w2 [2][16], b2 [2] fp32 -> scores fp32
 * [npix][2] + guard */
int mhip_score_head_host(mhip_ctx* ctx, int precision, const float* in, int in_stride, const float* w1, const float* b1,
                         const float* w2, const float* b2, long long npix, float* scores);

/* ---- stage entry of the row LayerNorm every tower shares (csrc/row_ops.hip) -------------------------------------------------
 * Test surface only, same conventions as the stage entries above.  replaces: nn.LayerNorm(D, eps) over rows.  x fp32 [rows][D];
 * with x_f16 (f16 mode only) it is narrowed to an f16 stream, and x_lo (or NULL) is its low plane, x = hi + lo.  g, b fp32 [D];
 * D a multiple of 64 up to 1024.  h fp32 [rows][D] + guard (NULL: not written); ht [rows][D] + guard in the mode's element type,
 * widened (NULL: not written); one of the two at least.  in_place: h and x are one device buffer (needs h, no x_f16). */
int mhip_row_layernorm_host(mhip_ctx* ctx, int precision, const float* x, int x_f16, const float* x_lo, const float* g,
                            const float* b, int rows, int D, float eps, int in_place, float* h, float* ht);

/* ---- Pillow-exact 8-bit resize (antialiased LANCZOS / BILINEAR / BICUBIC) of RGB images -------------------------------- */
#define MHIP_PIL_LANCZOS 1    /* PIL.Image.LANCZOS  */
#define MHIP_PIL_BILINEAR 2   /* PIL.Image.BILINEAR */
#define MHIP_PIL_BICUBIC 3    /* PIL.Image.BICUBIC  */
/* replaces: ResizeShortestEdge/ResizeTransform's PIL resize (marie/detectron/detector.py:103-105) and TrOCR's
 * im.resize((384, 384), BICUBIC) (marie/document/trocr_ocr_processor.py:116-118); LANCZOS is the document splitter's page
 * resize (marie/components/document_splitter/transformers.py:111-113).  Host u8 [sh][sw][3] -> [dh][dw][3]; a filter other
 * than the three above is MHIP_EINVAL. */
int mhip_pil_resize_rgb_host(mhip_ctx* ctx, const uint8_t* src_host, int sh, int sw, uint8_t* dst_host, int dh, int dw,
                             int filter);
/* The batched form TrOCR and LayoutLMv3 run (n fragments of different sizes -> n images of one size, one launch per pass), on
 * host buffers: fragment i is descs[i] (channels 3) inside base_host [base_bytes] -> dst_host u8 [n][dh][dw][3], each image
 * what Image.fromarray(fragment).resize((dw, dh), filter) gives. */
int mhip_pil_resize_fragments_host(mhip_ctx* ctx, const uint8_t* base_host, size_t base_bytes, const mhip_crop_desc* descs, int n,
                                   int dh, int dw, int filter, uint8_t* dst_host);

/* ---- ViT encoder: the DiT detector backbone (BEiT + fpn1..4) and the TrOCR image encoder ------------------------- */
/* replaces: BEiT.forward_features, marie/boxes/dit/ditod/beit.py:706-748 (dit_base_patch16 :787-800, dit_large_patch16
 * :803-816), and AdaptedVisionTransformer.forward_features, marie/models/unilm/trocr/deit.py:105-146.            */
typedef struct mhip_vit mhip_vit;
typedef struct mhip_vit_config {
  int dim, depth, heads;   /* 768/12/12 base, 1024/24/16 large; head dim must be 64                                     */
  int patch;               /* 16                                                                                    */
  int pos_h, pos_w;        /* pre-training position grid: 14 x 14 (DiT, IMG_SIZE 224), 24 x 24 (TrOCR, 384)          */
  int layer_scale;         /* blocks carry gamma_1 / gamma_2 (DiT: init_values 0.1 / 1e-5)                          */
  int qkv_bias;            /* 0 none (TrOCR DeiT), 1 BEiT q_bias + v_bias, 2 a full qkv.bias                        */
  int final_norm;          /* apply norm.{weight,bias} to the output tokens (TrOCR encoder)                         */
  int fpn;                 /* 1: fpn1..fpn4 on the outputs of blocks taps[0..3] (DiT: 3,5,7,11 / 7,11,15,23)        */
  int taps[4];
  float ln_eps;            /* 1e-6                                                                                  */
} mhip_vit_config;
int mhip_vit_create(mhip_ctx* ctx, int precision, const mhip_vit_config* cfg, mhip_vit** out);
int mhip_vit_destroy(mhip_vit* m);
/* keys relative to the BEiT / VisionTransformer module: cls_token, pos_embed, patch_embed.proj.*, blocks.N.*, norm.*, fpnK.* */
int mhip_vit_set_tensor(mhip_vit* m, const char* key, const float* data, const int64_t* shape, int ndim);
int mhip_vit_finalize(mhip_vit* m);
int mhip_vit_alloc_arena(mhip_vit* m);
int mhip_vit_arena(mhip_vit* m, void** arena_dev, size_t* bytes);
/* B host images u8 [th][tw][3], each placed top-left on a zero (post-normalisation) H32 x W32 canvas; pixel -> (p-127.5)/127.5,
 * swap_rb = 1 reverses the stored channel order.  Any output may be NULL.  tokens_out fp32 [B][1 + np][dim];
 * fpnK fp32 NHWC [B][h_K][w_K][dim] at strides 4, 8, 16, 32.                                                          */
int mhip_vit_forward_host(mhip_vit* m, const uint8_t* imgs_host, int B, int th, int tw, int H32, int W32, int swap_rb,
                          float* tokens_out, float* fpn0, float* fpn1, float* fpn2, float* fpn3);

/* One GEMM of a ViT block in the f16 mode, alone, on device operands: the products vit_encode launches around the split residual
 * stream (x = hi + lo, two f16 planes) with LayerNorm folded into the epilogue, through the same launcher and descriptor.
 * replaces: the norm1 / attn.qkv / attn.proj / norm2 / mlp.fc1 / mlp.fc2 modules of a BEiT / DeiT Block and PatchEmbed.proj
 * (marie/boxes/dit/ditod/beit.py, marie/models/unilm/trocr/deit.py), one product at a time.  For parity tests of each epilogue.
 *   MHIP_EPI_SPLIT    out (hi), out2 (lo) [rows][N] f16 = scale[n] * in[m] . w[n] + bias[n] + res[m][n] + res2[m][n] (res == out and
 *                     res2 == out2 allowed: in place); stats[(c * stats_ld + row) * 2] = (sum, centred sum of squares) of the row
 *                     over columns [64 c, 64 c + 64).  row_period > 0: GEMM row q is written to row
 *                     (q / row_period) * row_stride + row_offset + q % row_period and takes residual row q % row_period
 *   MHIP_EPI_LN_ROWS  out [M][N] f16 = act(ln_a[m] * in[m] . w[n] - ln_b[m] * ln_cs[n] + bias[n]);  ln_a = rstd, ln_b = mean * rstd
 *   MHIP_EPI_LN_COLS  out [M][N] f16 = ln_a[n] * in[m] . w[n] - ln_b[n] * ln_cs[m] + row_bias[m]
 * in [M][K], w [N][K] f16; act: 0 none, 2 erf GELU.  Every pointer is a device address; unused ones are NULL.  Enqueued on the
 * ctx stream.  Shapes and operands the kernel cannot take return MHIP_EINVAL.                                                   */
#define MHIP_EPI_LN_ROWS 1
#define MHIP_EPI_LN_COLS 2
#define MHIP_EPI_SPLIT 3
typedef struct mhip_gemm_fold_desc {
  const void* in_dev;
  const void* w_dev;
  const float* scale_dev;
  const float* bias_dev;
  void* out_dev;
  const float* ln_a_dev;
  const float* ln_b_dev;
  const float* ln_cs_dev;
  const float* row_bias_dev;
  void* out2_dev;
  const void* res_dev;
  const void* res2_dev;
  float* stats_dev;
  int32_t epi, M, N, K, act, stats_ld;
  int32_t row_period, row_stride, row_offset;
} mhip_gemm_fold_desc;
int mhip_gemm_ln_fold(mhip_ctx* ctx, int precision, const mhip_gemm_fold_desc* d);
/* The row statistics of MHIP_EPI_SPLIT (chunks = D / 64 of them per row, ld rows apart) -> rstd [rows] = (var + eps)^-1/2 and
 * mur [rows] = mean * rstd.  replaces: the mean / variance pass of nn.LayerNorm (norm1, norm2 of a Block).                      */
int mhip_ln_finalize(mhip_ctx* ctx, const float* stats_dev, int chunks, int ld, float* rstd_dev, float* mur_dev, int rows, int D,
                     float eps);
/* cls row (row 0) and pad rows (n_tok .. npad - 1) of each of B images of the split stream hi / lo [B * npad][D] f16, and their row
 * statistics (cls_stats fp32 [D / 64][2], zero for the pad rows).  replaces: torch.cat((cls_tokens, x), dim=1) of the forward.    */
int mhip_token_init_split(mhip_ctx* ctx, void* hi_dev, void* lo_dev, const float* cls_row_dev, const float* cls_stats_dev,
                          float* stats_dev, int stats_ld, int B, int npad, int n_tok, int D);

/* ---- DiT Mask R-CNN text detector (BoxProcessorUlimDit's model) ------------------------------------------------------- */
/* replaces: OptimizedDetectronPredictor.invoke_model, marie/detectron/detector.py:83-147 (model built by
 * build_vit_fpn_backbone, marie/boxes/dit/ditod/backbone.py:131-153; config/zoo/unilm/dit/text_detection/ YAMLs).       */
typedef struct mhip_dit mhip_dit;
typedef struct mhip_dit_config {
  int model;                 /* 0 dit_base_patch16 (mask_rcnn_dit_base.yaml), 1 dit_large_patch16 (mask_rcnn_dit_prod.yaml) */
  int min_size_test;         /* INPUT.MIN_SIZE_TEST 800                                                             */
  int max_size_test;         /* INPUT.MAX_SIZE_TEST 1333 (default) / 4000 (prod)                                    */
  int detections_per_image;  /* TEST.DETECTIONS_PER_IMAGE 2000 / 2500                                               */
  float anchor_sizes[5];     /* ANCHOR_GENERATOR.SIZES 4, 8, 16, 32, 64                                             */
  float aspect_ratios[3];    /* ANCHOR_GENERATOR.ASPECT_RATIOS 1.5, 3.5, 6.5                                        */
  float rpn_nms_thresh;      /* RPN.NMS_THRESH 0.7                                                                  */
  float score_thresh;        /* ROI_HEADS.SCORE_THRESH_TEST 0.05                                                    */
  float nms_thresh;          /* ROI_HEADS.NMS_THRESH_TEST 0.5                                                       */
  int num_classes;           /* ROI_HEADS.NUM_CLASSES: 1 (text detector), 5 (document boundary model); 1..16;
                              * more than 1 needs detections_per_image <= 1000                                         */
} mhip_dit_config;
int mhip_dit_default_config(int model, mhip_dit_config* cfg);
/* ResizeShortestEdge output (nh, nw) and the /32 canvas for an h x w page */
int mhip_dit_resized_shape(const mhip_dit_config* cfg, int h, int w, int* nh, int* nw, int* H32, int* W32);
int mhip_dit_create(mhip_ctx* ctx, int precision, const mhip_dit_config* cfg, mhip_dit** out);
int mhip_dit_destroy(mhip_dit* m);
/* detectron2 checkpoint keys ("backbone.bottom_up.backbone.*", "backbone.fpn_*", "proposal_generator.rpn_head.*",
 * "roi_heads.box_head.*", "roi_heads.box_predictor.*"; mask-head keys are accepted and ignored)                          */
int mhip_dit_set_tensor(mhip_dit* m, const char* key, const float* data, const int64_t* shape, int ndim);
int mhip_dit_finalize(mhip_dit* m);
int mhip_dit_alloc_arena(mhip_dit* m);
int mhip_dit_arena(mhip_dit* m, int which /* 0 backbone, 1 heads */, void** arena_dev, size_t* bytes);
/* Bytes of ctx workspace mhip_dit_detect of B h x w pages carves: exactly its layout's sizing pass. */
size_t mhip_dit_workspace_bytes(mhip_dit* m, int B, int h, int w);
/* B device pages u8 BGR [h][w][3] of one size -> per page up to 1000 boxes xyxy fp32 in page coordinates, score-ordered.
 * boxes_host [B][1000][4], scores_host [B][1000] (may be NULL), counts_host [B].                                      */
int mhip_dit_detect(mhip_dit* m, const uint8_t* const* pages_dev, int B, int h, int w, float* boxes_host,
                    float* scores_host, int* counts_host);
int mhip_dit_detect_host(mhip_dit* m, const uint8_t* pages_host, int B, int h, int w, float* boxes_host,
                         float* scores_host, int* counts_host);
/* the same with the predicted class of every box (detectron2 pred_classes, 0-based; all 0 when num_classes is 1):
 * classes_host [B][1000] int32, may be NULL                                                                          */
int mhip_dit_detect_ex(mhip_dit* m, const uint8_t* const* pages_dev, int B, int h, int w, float* boxes_host,
                       float* scores_host, int32_t* classes_host, int* counts_host);
int mhip_dit_detect_ex_host(mhip_dit* m, const uint8_t* pages_host, int B, int h, int w, float* boxes_host,
                            float* scores_host, int32_t* classes_host, int* counts_host);
/* one page plus the intermediates the parity tests compare: FPN maps p2..p6 fp32 NHWC and the RPN proposals (any NULL) */
int mhip_dit_debug_host(mhip_dit* m, const uint8_t* page_host, int h, int w, float* boxes_host, float* scores_host,
                        int* count_host, float* p2, float* p3, float* p4, float* p5, float* p6, float* prop_boxes,
                        float* prop_scores, int* prop_count);
/* same plus the inputs of the two discrete stages as this run computed them: fpn5[l] as above, rpn_head5[l] fp32
 * [H*W][16] for p2..p6, box_head fp32 [1000][8] (rows past *prop_count undefined); any pointer may be NULL             */
int mhip_dit_debug_taps_host(mhip_dit* m, const uint8_t* page_host, int h, int w, float* boxes_host, float* scores_host,
                             int* count_host, float* const* fpn5, float* const* rpn_head5, float* prop_boxes,
                             float* prop_scores, int* prop_count, float* box_head);
/* The detectron2 stages of the detector on caller-supplied host inputs (each also used by the parity tests):
 * RPN.predict_proposals for one image — heads_host[l] fp32 [H[l]*W[l]][16] (3 objectness logits, 3 x 4 deltas, 1 pad) for
 * p2..p6 -> up to 1000 proposals xyxy + logits, score-ordered;                                                          */
int mhip_rpn_proposals_host(mhip_ctx* ctx, const float* const* heads_host, const int* H, const int* W, const int* strides,
                            const float* anchor_sizes, const float* aspect_ratios, int img_h, int img_w, float nms_thresh,
                            float* boxes_out, float* scores_out, int* count_out);
/* ROIPooler (7x7 ROIAlignV2, sampling_ratio 0, levels by box size) — feats_host[l] fp32 NHWC at strides 4..32,
 * rois [n][4] (n <= 1000) -> pooled fp32 [n][49*C] with k = bin*C + c;                                                  */
int mhip_roi_align_host(mhip_ctx* ctx, const float* const* feats_host, const int* H, const int* W, int C,
                        const float* rois_host, int n, float* pooled_out);
/* FastRCNNOutputLayers.inference + detector_postprocess — head_host [n][8] (2 class scores, 4 deltas, 2 pad).           */
int mhip_det_final_host(mhip_ctx* ctx, const float* head_host, const float* rois_host, int n, int img_h, int img_w,
                        int page_h, int page_w, float score_thresh, float nms_thresh, int max_det, float* boxes_out,
                        float* scores_out, int* count_out);
/* The K-class FastRCNNOutputLayers.inference + detector_postprocess (K = num_classes > 1): head_host [n][ld] fp32 with
 * the K + 1 class logits (background last) in columns 0..K and the class-specific deltas [4K] in columns K+1..5K;
 * softmax, decode (10, 10, 5, 5), drop non-finite rows, clip, (row, class) pairs with score > score_thresh, torchvision
 * batched_nms with the class-offset coordinates, top max_det (<= 1000), rescale to the page, clip, drop empty.
 * -> boxes [1000][4], scores [1000], classes [1000] int32, *count.                                                       */
int mhip_det_final_multi_host(mhip_ctx* ctx, const float* head_host, int ld, const float* rois_host, int n, int num_classes,
                              int img_h, int img_w, int page_h, int page_w, float score_thresh, float nms_thresh,
                              int max_det, float* boxes_out, float* scores_out, int32_t* classes_out, int* count_out);
/* ---- document boundary registration (UnilmDocumentBoundaryRegistration.predict_document_image, the warp) ----------------- */
/* replaces: the crop / cv2.resize(INTER_AREA) / cv2.copyMakeBorder / cv2.circle / cv2.resize(INTER_CUBIC) chain of
 * marie/components/document_registration/unilm_dit.py:416-508 on a device page.  The crop window of the page is resized
 * to out_w x out_h (INTER_AREA semantics: area shrink, or OpenCV's linear resampler with area coefficients when either axis
 * enlarges; a plain copy when the sizes agree) and placed at (left, top) of a white canvas_w x canvas_h canvas, every
 * canvas pixel written once; filled Circle()s of marker_radius at the marker centres (clipped to the canvas) in
 * marker_color (array channel order).  When the canvas differs from final_w x final_h it is then resized to it with
 * INTER_CUBIC.                                                                                                              */
typedef struct mhip_register_desc {
  int crop_x, crop_y, crop_w, crop_h;   /* window of the page (inside it); crop_w or crop_h 0: nothing is pasted       */
  int out_w, out_h;                     /* resized window size                                                         */
  int left, top;                        /* where the resized window lands on the canvas                                */
  int canvas_w, canvas_h;               /* the aligned page before the shape restore                                   */
  int n_markers;                        /* 0..4                                                                        */
  int marker_x[4], marker_y[4];
  int marker_radius;                    /* 0..64                                                                       */
  int marker_color[3];
  int final_w, final_h;                 /* the returned page                                                           */
} mhip_register_desc;
/* page_dev u8 [h][w][3] with rows page_pitch bytes apart -> out_dev u8 [final_h][final_w][3] packed.  scratch_dev holds
 * the canvas when a restore is needed (canvas_w * canvas_h * 3 bytes; may be NULL otherwise).  Enqueued on the ctx stream. */
int mhip_register_warp(mhip_ctx* ctx, const uint8_t* page_dev, int h, int w, size_t page_pitch, const mhip_register_desc* d,
                       uint8_t* scratch_dev, uint8_t* out_dev);
int mhip_register_warp_host(mhip_ctx* ctx, const uint8_t* page_host, int h, int w, const mhip_register_desc* d,
                            uint8_t* out_host);
/* ---- overlay cleaner: pix2pixHD LocalEnhancer generator + blend -------------------------------- */
/* replaces: OverlayProcessor.__extract_segmentation_mask / model.test() (marie/overlay/overlay.py:165-189;
 * marie/models/pix2pix/models/networks_hd.py:24-213, netG "local", instance norm, spectral-normed convolutions) — page in HBM
 * -> generator -> image in HBM, no PNG round trip.  ngf: base width (64 in the reference; f16 needs a multiple of 64, f32 32). */
typedef struct mhip_overlay mhip_overlay;
int mhip_overlay_create(mhip_ctx* ctx, int precision, int ngf, mhip_overlay** out);
int mhip_overlay_destroy(mhip_overlay* m);
/* state_dict keys of the reference's netG ("model.1.weight_orig" / ".weight_u" / ".weight_v" / ".bias", "model1_2.3.*",
 * "downsample.weight" ...; an optional "netG." / "module." prefix is ignored); data fp32 in the checkpoint's layout            */
int mhip_overlay_set_tensor(mhip_overlay* m, const char* key, const float* data, const int64_t* shape, int ndim);
int mhip_overlay_finalize(mhip_overlay* m);
/* OverlayProcessor.preprocess (overlay.py:147-163): the white canvas the page is placed on (both sides to the next multiple of
 * 32 when either is ragged)                                                                                                    */
int mhip_overlay_padded_shape(int h, int w, int* H, int* W);
/* page u8 BGR [h][w][3] (device) -> the generator's image u8 RGB [H][W][3] on the padded canvas = tensor2im(fake)             */
int mhip_overlay_forward(mhip_overlay* m, const uint8_t* page_dev, int h, int w, uint8_t* fake_rgb_dev);
int mhip_overlay_forward_host(mhip_overlay* m, const uint8_t* page_host, int h, int w, uint8_t* fake_rgb_host, float* raw_host);
/* replaces: OverlayProcessor.blend_to_text (overlay.py:247-291): real BGR + generator image -> text-only image (BGR)          */
int mhip_overlay_blend(mhip_ctx* ctx, const uint8_t* real_bgr_dev, const uint8_t* mask_dev, uint8_t* out_dev, size_t pixels);
/* replaces: blackout_bboxes, marie/boxes/dit/ulim_dit_box_processor.py:161-198, in place on a device page (BGR).        */
int mhip_blackout_bboxes(mhip_ctx* ctx, uint8_t* page_dev, int h, int w, const int32_t* boxes_xyxy_host, int n,
                         int* changed);
/* replaces: the OpenCV chain of crop_to_content (marie/utils/image_utils.py:190-252, behind OcrEngine.extract(crop_to_content=True),
 * marie/ocr/ocr_engine.py:169-176) and of crop_to_content_box (marie/boxes/dit/ulim_dit_box_processor.py:291-352, behind
 * psm_sparse(bbox_optimization=True), :608-626): BGR2GRAY, then content_aware ? close_2x3(otsu(divide(gray, blur5x5(gray), 255)))
 * : otsu(gray).  For each of n rectangles (x, y, w, h, inside the h x w BGR device page) ext[i] = {xmin, ymin, xmax, ymax, count}
 * of the pixels that come out 0, in rectangle coordinates (count == 0: no such pixel, the rest is 0).  The callers' padding
 * rules stay on the host (marie_icr_amd/content.py).                                                                           */
int mhip_content_extents(mhip_ctx* ctx, const uint8_t* page_dev, int h, int w, const int32_t* rects_xywh_host, int n,
                         int content_aware, int32_t* ext_host);

/* ---- TrOCR recognizer (image encoder + text decoder + beam search) ------------------------------------------------------ */
/* replaces: TrOcrProcessor's model path, marie/document/trocr_ocr_processor.py:116-180 (preprocess_image, get_text), with
 * TrOCREncoder (marie/models/unilm/trocr/trocr_models.py:508-524), fairseq's TransformerDecoder (built :137-147) and
 * TextRecognitionGenerator._generate (marie/models/unilm/trocr/generator.py:11-374).                                      */
typedef struct mhip_trocr mhip_trocr;
typedef struct mhip_trocr_config {
  int enc_dim, enc_depth, enc_heads;            /* trocr_base: beit_base_patch16_384 = 768 / 12 / 12 (trocr_models.py:423-434) */
  int dec_dim, dec_layers, dec_heads, dec_ffn;  /* 1024 / 12 / 16 / 4096                                                      */
  int vocab;                                    /* len(target dictionary)                                                     */
  int max_positions;                            /* decoder max_positions (512): embed_positions has max_positions + pad + 1 rows */
  int beam;                                     /* 3 (trocr_ocr_processor.py:228)                                             */
  int max_len_b;                                /* generation max_len_b (200); max_len = min(max_len_b, max_positions - 1)     */
  int min_len;                                  /* 1                                                                          */
  int pad, eos;                                 /* fairseq dictionary: 1, 2                                                   */
  float embed_scale;                            /* 1.0 with RoBERTa's no_scale_embedding, else sqrt(dec_dim)                  */
  int img_size;                                 /* 384                                                                        */
} mhip_trocr_config;
int mhip_trocr_default_config(int model /* 0 base, 1 large */, mhip_trocr_config* cfg);
int mhip_trocr_max_len(const mhip_trocr_config* cfg);
int mhip_trocr_create(mhip_ctx* ctx, int precision, const mhip_trocr_config* cfg, mhip_trocr** out);
int mhip_trocr_destroy(mhip_trocr* m);
/* fairseq checkpoint keys: "encoder.deit.*" (timm VisionTransformer) and "decoder.*" (TransformerDecoder)                  */
int mhip_trocr_set_tensor(mhip_trocr* m, const char* key, const float* data, const int64_t* shape, int ndim);
int mhip_trocr_finalize(mhip_trocr* m);
int mhip_trocr_alloc_arena(mhip_trocr* m);
int mhip_trocr_arena(mhip_trocr* m, int which /* 0 encoder, 1 decoder */, void** arena_dev, size_t* bytes);
/* Bytes of ctx workspace mhip_trocr_generate of n crops carves (encoder + beam search): exactly its layout's sizing pass. */
size_t mhip_trocr_workspace_bytes(mhip_trocr* m, int n);
/* `gate` (may be NULL) is signalled inside every generate call at the point of the stream where the image encoder ends and
 * the autoregressive decode begins (TextRecognitionGenerator._generate's step loop, generator.py:182-362).  The caller owns it. */
int mhip_trocr_set_decode_gate(mhip_trocr* m, mhip_gate* gate);
/* n device crops u8 [img][img][3] -> best hypothesis per crop: tokens_out [n][max_len + 1] (eos included, pad-filled),
 * lengths_out [n], scores_out [n] = length-normalised log-probability (the reference reports exp(score)).               */
int mhip_trocr_generate(mhip_trocr* m, const uint8_t* crops_dev, int n, int swap_rb, int32_t* tokens_out,
                        int32_t* lengths_out, float* scores_out);
/* host crops; optional parity taps: enc_tokens_out fp32 [n][577][enc_dim], step0_logits_out fp32 [n][vocab]               */
int mhip_trocr_generate_host(mhip_trocr* m, const uint8_t* crops_host, int n, int swap_rb, int32_t* tokens_out,
                             int32_t* lengths_out, float* scores_out, float* enc_tokens_out, float* step0_logits_out);
/* The recognizer in two halves, for callers whose fragments arrive in batches (OcrEngine's batched path: page batches leave the
 * detector one after the other, where the reference's loop calls its recognizer page by page, marie/ocr/ocr_engine.py:172-199):
 * the image encoder (marie/models/unilm/trocr/deit.py:105-146) runs per batch of fragments, the beam search
 * (generator.py:127-362) once over everything encoded since encode_begin — results as mhip_trocr_generate_fragments on the
 * concatenated batches.  encode_begin(max_crops) reserves the token store (grow-only; more than max_crops may follow).       */
int mhip_trocr_encode_begin(mhip_trocr* m, int max_crops);
int mhip_trocr_encode_fragments(mhip_trocr* m, const uint8_t* base_dev, const mhip_crop_desc* descs_host, int n, int swap_rb);
int mhip_trocr_encoded(mhip_trocr* m);      /* crops encoded since encode_begin                                               */
int mhip_trocr_decode(mhip_trocr* m, int32_t* tokens_out, int32_t* lengths_out, float* scores_out);
/* fragments of any size (3 channels) inside one device buffer -> Pillow bicubic to img x img -> generate                    */
int mhip_trocr_generate_fragments(mhip_trocr* m, const uint8_t* base_dev, const mhip_crop_desc* descs_host, int n,
                                  int swap_rb, int32_t* tokens_out, int32_t* lengths_out, float* scores_out);
/* mhip_trocr_generate_host plus the candidate list of every beam-search step as the generator saw it (BeamSearch.step's
 * top 2*beam of cumulative score, generator.py:208-223): trace_* are host arrays [max_len + 1][n][2 * beam] (scores, token ids,
 * source beams), *steps_out the number of steps that ran.  For parity tests: the oracle's search is walked beside it. */
int mhip_trocr_generate_trace_host(mhip_trocr* m, const uint8_t* crops_host, int n, int swap_rb, int32_t* tokens_out,
                                   int32_t* lengths_out, float* scores_out, float* trace_scores, int32_t* trace_tokens,
                                   int32_t* trace_beams, int* steps_out);
/* The decoder's encoder-attention stage alone (one layer, one step) on host inputs, through the f16 kernels that attend over
 * the encoder tokens themselves (key / value projections absorbed: cross_attn.hip).  replaces: fairseq MultiheadAttention
 * (encoder_attn) as TextRecognitionGenerator drives it, marie/models/unilm/trocr/generator.py:127-362.  q [crops*beam][heads*64]
 * (projected, scaled), enc [crops][n_tok][enc_dim], wk / wv [heads*64][enc_dim], bv [heads*64] -> out [crops*beam][heads*64]. */
int mhip_cross_attention_host(mhip_ctx* ctx, const float* q, const float* enc, const float* wk, const float* wv,
                              const float* bv, int crops, int beam, int heads, int n_tok, int enc_dim, float* out);
/* The same call with each of its three kernels (absorb_q, cross_attn, absorb_v) observable, for the kernel-level tests.  enc is
 * [crops][kv_rows][enc_dim] with kv_rows >= n_tok and kv_rows % 8 == 0: rows n_tok .. kv_rows - 1 of a crop are the caller's
 * padding (finite values; the kernel reads them masked), the zero slack rows behind the last crop are appended by the call.
 * The absorbed-query and context scratch and the output are filled with the f16 NaN pattern 0xffff before the launch and
 * copied out as fp32: qt_out / ct_out [crops*beam][16][enc_dim] (either may be NULL), out [crops*beam][heads*64].  Refused
 * without a launch: enc_dim outside {256, 512, 768, 1024}, beam outside 1 .. 4, heads outside 1 .. 16, kv_rows < n_tok,
 * kv_rows % 8, n_tok < 1, crops < 1, a null operand.                                                                       */
int mhip_cross_attention_stages_host(mhip_ctx* ctx, const float* q, const float* enc, const float* wk, const float* wv,
                                     const float* bv, int crops, int beam, int heads, int n_tok, int kv_rows, int enc_dim,
                                     float* qt_out, float* ct_out, float* out);
/* The decoder's decode attention alone (one layer, one step) on host inputs, through the kernels trocr_decode launches: the
 * self-attention over a hypothesis' history and the encoder-attention over projected keys / values (fp32, and f16 without the
 * absorbed path).  replaces: fairseq MultiheadAttention (self_attn with incremental state / encoder_attn) as
 * TextRecognitionGenerator drives it, marie/models/unilm/trocr/generator.py:127-362.  Operands are rounded to the precision's
 * element type and laid out with the production pitches.  q [rows][heads*64] (projected, scaled), rows = groups * nq.
 *   anc != NULL (self-attention, nq = 1): k / v [n_keys][slots][heads*64], key s of row r at step s, slot anc[r*anc_ld + s];
 *   anc == NULL (encoder-attention, nq queries per group): k / v [groups][kv_rows][heads*64], the first n_keys rows attended.
 * force_generic: the generic kernel even where the f16 short-history kernel would run.  -> out [rows][heads*64].          */
int mhip_decode_attention_host(mhip_ctx* ctx, int precision, int heads, int n_keys, int nq, int rows, int slots, int kv_rows,
                               const float* q, const float* k, const float* v, const int32_t* anc, int anc_ld,
                               int force_generic, float* out);
/* The per-step beam search of the decoder alone, on host inputs, through the launchers trocr_decode drives.  replaces:
 * BeamSearch.step, finalize_hypos and the row selection of TextRecognitionGenerator._generate,
 * marie/models/unilm/trocr/generator.py:165-372.
 *
 * mhip_beam_candidates_host: one launch of the candidates kernel.  logits [bsz*beam][ld] in the element type the flag names
 * (fp32, or IEEE half when logits_f16), columns vocab .. ld-1 are row padding and may hold anything; cum [bsz*beam].
 * -> cand_scores / cand_tokens / cand_beams [bsz * 2 * beam + 16]: the device buffers carry 16 guard elements behind the lists,
 * are filled with 0xff bytes before the launch and come back whole.  Refused without writing output: what the launcher refuses
 * (beam outside 1 .. 4, vocab < 2 * beam, a pitch that is no multiple of 8 or shorter than the vocabulary rounded up to 8),
 * min_len > max_len, bsz < 1, a null pointer.                                                                              */
int mhip_beam_candidates_host(mhip_ctx* ctx, int logits_f16, const void* logits, const float* cum, int step, int max_len,
                              int min_len, int pad, int eos, int vocab, int ld, int beam, int bsz, float* cand_scores,
                              int32_t* cand_tokens, int32_t* cand_beams);
/* What mhip_beam_search_host copies out.  S = max_len + 1 rows per step (the steps that ran are filled), M = bsz * beam.    */
typedef struct mhip_beam_trace {
  float* cand_scores;     /* [S][bsz][2*beam] the step's candidate lists as beam_select read them                          */
  int32_t* cand_tokens;
  int32_t* cand_beams;
  int32_t* parent;        /* [S][M] after the step's beam_select                                                            */
  int32_t* last_tok;      /* [S][M]                                                                                         */
  float* cum;             /* [S][M]                                                                                         */
  uint8_t* ignore;        /* [S][M]                                                                                         */
  uint8_t* finished;      /* [S][bsz]                                                                                       */
  int32_t* fin_count;     /* [S][bsz]                                                                                       */
  int32_t* tokens;        /* [S][M][max_len + 2] the token buffer the step wrote                                            */
  int32_t* anc;           /* [S][M][max_len + 2] the ancestry table the step's decoder would read (0xff where never written) */
  int32_t* remaining;     /* [S]                                                                                            */
  int32_t* fin_tokens;    /* [bsz][beam][max_len + 1], at the end; cells never written hold 0xff bytes                      */
  int32_t* fin_len;       /* [M]                                                                                            */
  float* fin_score;       /* [M]                                                                                            */
  int32_t* out_tokens;    /* [bsz][max_len + 1] beam_best                                                                   */
  int32_t* out_len;       /* [bsz]                                                                                          */
  float* out_score;       /* [bsz]                                                                                          */
  int32_t steps;          /* steps that ran, the extra ones included                                                        */
} mhip_beam_trace;
/* mhip_beam_search_host: trocr_decode's launch sequence with the decoder taken out — beam_init; per step ancestry (step > 0),
 * the step's candidates, beam_select; beam_best at the end — on a state carved from the context workspace.  The candidates of
 * step s come from the candidates kernel on logits[s] (logits [max_len + 1][bsz*beam][ld], element type as above), or, with
 * logits == NULL, from the caller's lists in_scores / in_tokens / in_beams [max_len + 1][bsz][2*beam], uploaded in place of that
 * launch.  Steps run until no crop remains or step max_len has run; then `extra_steps` (0 .. 2) more, never past step max_len.
 * trocr_decode, which reads the counter two steps late, enqueues exactly one step past the end; 2 is a margin for a caller that
 * reads it later still.  Refusals as above, checked before anything is written.                                            */
int mhip_beam_search_host(mhip_ctx* ctx, int logits_f16, const void* logits, const float* in_scores, const int32_t* in_tokens,
                          const int32_t* in_beams, int max_len, int min_len, int pad, int eos, int vocab, int ld, int beam,
                          int bsz, int extra_steps, mhip_beam_trace* out);

/* ---- LayoutLMv3 page classifier (OCR words + boxes + page image -> class logits) ------------------------------------------ */
/* replaces: the model path of TransformersDocumentClassifier with task="text-classification-multimodal",
 * marie/components/document_classifier/transformers.py (LayoutLMv3ForSequenceClassification of the transformers library:
 * text + layout embeddings, 16 x 16 patch embeddings of the page resized to input_size, twelve post-LN layers whose attention
 * carries a learned relative-position bias (1-d bucket of the token index, 2-d buckets of x0 and y1) and a padding mask, and
 * the classification head on row 0).                                                                                        */
typedef struct mhip_layoutlmv3 mhip_layoutlmv3;
typedef struct mhip_layoutlmv3_config {
  int hidden, layers, heads, ffn;                 /* 768 / 12 / 12 / 3072                                                    */
  int vocab, type_vocab;                          /* 50265 / 1                                                               */
  int max_position_embeddings;                    /* 514: position ids of max_text unpadded tokens reach pad + max_text      */
  int max_2d_position_embeddings;                 /* 1024                                                                    */
  int coordinate_size, shape_size;                /* 128 / 128: 4 * coordinate_size + 2 * shape_size == hidden               */
  int input_size, patch;                          /* 224 / 16                                                                */
  int rel_pos_bins, max_rel_pos;                  /* 32 / 128                                                                */
  int rel_2d_pos_bins, max_rel_2d_pos;            /* 64 / 256                                                                */
  float layer_norm_eps;                           /* 1e-5 (the visual `norm` keeps the library's fixed 1e-6)                 */
  int pad_id;                                     /* 1                                                                       */
  int num_labels;
  int max_text;                                   /* text rows per page (512)                                                */
} mhip_layoutlmv3_config;
int mhip_layoutlmv3_default_config(mhip_layoutlmv3_config* cfg);
/* MHIP_EINVAL for what the kernels do not cover: hidden != heads * 64, hidden % 256, hidden > 1024, ffn % 64, patch != 16,
 * input_size % 16, 4 * coordinate_size + 2 * shape_size != hidden, max_2d_position_embeddings > 1024, max_text > 1024 or
 * max_text % 8, max_position_embeddings < max_text + pad_id + 1, odd bucket counts.                                        */
int mhip_layoutlmv3_create(mhip_ctx* ctx, int precision, const mhip_layoutlmv3_config* cfg, mhip_layoutlmv3** out);
int mhip_layoutlmv3_destroy(mhip_layoutlmv3* m);
/* Hugging Face state-dict keys: "layoutlmv3.embeddings.word_embeddings.weight" ... "classifier.out_proj.bias"              */
int mhip_layoutlmv3_set_tensor(mhip_layoutlmv3* m, const char* key, const float* data, const int64_t* shape, int ndim);
int mhip_layoutlmv3_finalize(mhip_layoutlmv3* m);
int mhip_layoutlmv3_alloc_arena(mhip_layoutlmv3* m);
int mhip_layoutlmv3_arena(mhip_layoutlmv3* m, void** arena_dev, size_t* bytes);
/* the Pillow filter of the page resize to input_size x input_size: MHIP_PIL_LANCZOS (the document splitter's), _BILINEAR (the
 * default: the classifier's and the indexer's) or _BICUBIC; anything else is MHIP_EINVAL.  Holds for every later call.       */
int mhip_layoutlmv3_set_resample(mhip_layoutlmv3* m, int filter);
/* rows per page of the hidden states: max_text + (input_size / patch)^2 + 1 (709)                                          */
int mhip_layoutlmv3_seq_len(const mhip_layoutlmv3_config* cfg);
/* LayoutLMv3Encoder.relative_position_bucket (bidirectional) of one difference, evaluated in float32 as the library does.
 * Host only, no ctx: the attention tables are folded from it at finalize.                                                  */
int mhip_layoutlmv3_bucket(int relative_position, int num_buckets, int max_distance);
/* n pages (3-channel u8 fragments of any size inside one device buffer, channel order as stored) with their token ids
 * [n][max_text], boxes [n][max_text][4] on the 0..1000 grid and attention mask [n][max_text] (host int32 arrays)
 * -> logits_out fp32 [n][num_labels] (host).  One call runs all n pages through one launch sequence.  A box coordinate
 * outside [0, max_2d_position_embeddings) or an id outside the vocabulary is MHIP_EINVAL.                                  */
int mhip_layoutlmv3_classify(mhip_layoutlmv3* m, const uint8_t* base_dev, const mhip_crop_desc* pages_host, int n,
                             const int32_t* ids, const int32_t* bbox, const int32_t* attention_mask, float* logits_out);
/* the same on one packed host buffer of pages; optional parity taps: hidden_out fp32 [n][seq_len][hidden] (the last hidden
 * states, all rows: padded text rows hold what the library computes for them), resized_out u8 [n][input_size][input_size][3] */
int mhip_layoutlmv3_hidden_host(mhip_layoutlmv3* m, const uint8_t* pages_host, size_t pages_bytes,
                                const mhip_crop_desc* pages_desc, int n, const int32_t* ids, const int32_t* bbox,
                                const int32_t* attention_mask, float* logits_out, float* hidden_out, uint8_t* resized_out);
/* ---- LayoutLMv3 token tagging (the model call of the document indexer) ---------------------------------------------------- */
/* replaces: the model call of TransformersDocumentIndexer.inference, marie/components/document_indexer/transformers.py:519-568
 * (LayoutLMv3ForTokenClassification of the transformers library on the windows of a page, logits.argmax(-1) and
 * logits.softmax(-1) at the arg-max).  The same object serves it: finalize reads the head kind from the state dict,
 *   classifier.weight [num_labels][hidden] + classifier.bias                -> the linear head (the library's for num_labels < 10);
 *   classifier.dense.* + classifier.out_proj.*                              -> dense, tanh, out_proj (num_labels >= 10; the shapes
 *                                                                              of the sequence-classification head).
 * A model with the linear head answers mhip_layoutlmv3_classify / _hidden_host with MHIP_ESTATE; one with the dense head
 * serves both tasks.  The token head covers mhip_layoutlmv3_max_token_labels(hidden) labels (64, or what fits the LDS beside
 * W_o: 48 at hidden 768, 35 at hidden 1024); more are MHIP_EINVAL from tag / tag_host, and from finalize for the linear head,
 * which serves no other task.  The classifier entry points have no such limit.
 * n_win windows of text (ids / bbox / attention_mask [n_win][max_text], as for classify) over n_pages page images: window w
 * belongs to page window_page[w] (0 <= window_page[w] < n_pages <= n_win); resize, patch matrix and patch projection run
 * once per page.  -> label_out int32 [n_win][max_text] (lowest index of the largest logit), score_out fp32 [n_win][max_text]
 * (its soft-max probability, 1 / sum exp(z - z_max)), and, only when logits_out != NULL, the logits fp32
 * [n_win][max_text][num_labels] (host arrays).  Rows of padding carry what the library computes for them.                  */
int mhip_layoutlmv3_tag(mhip_layoutlmv3* m, const uint8_t* base_dev, const mhip_crop_desc* pages_host, int n_pages,
                        const int32_t* window_page, int n_win, const int32_t* ids, const int32_t* bbox,
                        const int32_t* attention_mask, int32_t* label_out, float* score_out, float* logits_out);
/* the same on one packed host buffer of pages                                                                               */
int mhip_layoutlmv3_tag_host(mhip_layoutlmv3* m, const uint8_t* pages_host, size_t pages_bytes, const mhip_crop_desc* pages_desc,
                             int n_pages, const int32_t* window_page, int n_win, const int32_t* ids, const int32_t* bbox,
                             const int32_t* attention_mask, int32_t* label_out, float* score_out, float* logits_out);
/* labels the token head covers at this hidden width (host only, no ctx)                                                      */
int mhip_layoutlmv3_max_token_labels(int hidden);
/* The token head alone on host inputs (parity tests): hidden fp32 [rows][D] (D a multiple of 256 up to 1024).  dense_w [D][D] +
 * dense_b [D] non-NULL: the dense head (hidden and dense_w rounded to the precision's element type, the product through the
 * GEMM the model uses, then tanh); NULL: the linear head.  out_w [L][D], out_b [L] -> label_out int32 [rows], score_out fp32
 * [rows], logits_out fp32 [rows][L] or NULL.  Everything after the dense product is fp32 in both precisions.               */
int mhip_token_head_host(mhip_ctx* ctx, int precision, int rows, int D, int L, const float* hidden, const float* dense_w,
                         const float* dense_b, const float* out_w, const float* out_b, int32_t* label_out, float* score_out,
                         float* logits_out);
/* The biased attention kernel alone on host inputs (parity tests): softmax(q k^T / 8 + (B1[h][b(pj - pi)] + Bx[h][b(xj - xi)]
 * + By[h][b(yj - yi)]) / 8 + mask) v for `heads` heads of 64.  q, k, v fp32 [n_tok][heads*64] (rounded to the precision's
 * element type), pos / x / y int32 [n_tok], valid int32 [n_tok] (0: masked as a key), w1 [heads][bins_1d], wx / wy
 * [heads][bins_2d] -> out fp32 [n_tok][heads*64].                                                                          */
int mhip_attention_bias_host(mhip_ctx* ctx, int precision, int heads, int n_tok, const float* q, const float* k,
                             const float* v, const int32_t* pos, const int32_t* x, const int32_t* y, const int32_t* valid,
                             const float* w1, const float* wx, const float* wy, int bins_1d, int max_1d, int bins_2d,
                             int max_2d, float* out);
/* One launch of the attention kernel (csrc/attn_flash.hip), plain or biased, with the whole descriptor in the caller's hands
 * (kernel-level parity tests).  Rq = images * npad_q + MHIP_ATTN_SLACK_ROWS query rows, Rk = images * npad_k +
 * MHIP_ATTN_SLACK_ROWS key rows, D = heads * 64.  The caller fills EVERY row, the padding rows of each image and the slack
 * behind the last one included; the entry only narrows fp32 to the precision's element type.  q is in the kernel's units
 * (already scaled by head_dim^-0.5 * log2 e).  Nothing is launched, and MHIP_EINVAL returned, for a shape the launcher refuses. */
#define MHIP_ATTN_SLACK_ROWS 128
#define MHIP_ATTN_LAYOUT_FUSED 0 /* q | k rows of pitch 2 D in one buffer, as every model lays them out: npad_q == npad_k   */
#define MHIP_ATTN_LAYOUT_SPLIT 1 /* q and k buffers of pitch D each: npad_q and npad_k are independent                      */
typedef struct mhip_attention_host_desc {
  int32_t precision, layout;
  int32_t images, heads, n_queries, n_keys, npad_q, npad_k;
  const float* q;       /* [Rq][D]                                                                                          */
  const float* k;       /* [Rk][D]                                                                                          */
  const float* vt;      /* [D * images * npad_k + MHIP_ATTN_SLACK_ROWS]: V^T, row pitch images * npad_k, then the slack     */
  /* the biased form (w1 non-NULL): per row pos, x, y (qcode [Rq][3]) and pos, x, y, valid (kcode [Rk][4]), pos in [0, dp],
   * x and y in [0, dx]; the tables are folded from w1 [heads][bins_1d], wx / wy [heads][bins_2d] as the model folds them   */
  const int32_t* qcode;
  const int32_t* kcode;
  const float *w1, *wx, *wy;
  int32_t bins_1d, max_1d, bins_2d, max_2d, dp, dx;
  /* [Rq][D] in the ELEMENT TYPE (f16 or fp32 bits): the device buffer is filled with the byte 0xff (a NaN in both types)
   * before the launch and copied back whole, so that rows nobody wrote and the guard rows behind the last image show       */
  void* out;
} mhip_attention_host_desc;
int mhip_attention_host(mhip_ctx* ctx, const mhip_attention_host_desc* d);

/* ---- VQ-NNF template matching (csrc/vqnnf.hip) -------------------------------------------------------------------------- */
/* replaces: VQNNFMatcher + GaussHaarFilters + KMeans, marie/components/template_matching/vqnnf/matching/, with the colour
 * features of PixelFeatureExtractor (num_features == 27), and the peak loop of vqnnf_template_matching.py:184-202,307.
 * Images are uint8 [H][W][3]; a feature vector is a pixel's RGB and its eight neighbours (wrapping around the edges of its own
 * H x W image, as torch.roll does), / 255.  Equal distances go to the lowest code.  Rectangles are x, y, w, h.              */
#define MHIP_VQ_FEATURES 27
#define MHIP_VQ_MAX_CODES 128
#define MHIP_VQ_MAX_FILTERS 6
typedef struct mhip_vq_filters {
  int32_t n;                                  /* filters, <= MHIP_VQ_MAX_FILTERS                                             */
  float taps[MHIP_VQ_MAX_FILTERS][16];        /* 4 x 4 integral-image taps (rows, cols), already / 16                        */
  int32_t dil[MHIP_VQ_MAX_FILTERS][2];        /* dilation over rows, cols (>= 1): the kernel spans 3 * dil + 1               */
  double weight[MHIP_VQ_MAX_FILTERS];         /* scale weight x filter weight                                                */
} mhip_vq_filters;
typedef struct mhip_vq_template mhip_vq_template;
/* The template-side state of one template: k-means (at most 25 iterations, stop at error <= 1e-4) over the pixels of `box` of
 * `frame` (host memory, or device memory when on_device) from the centroids at rows init_idx[n_init] of those pixels
 * (n_init = min(128, w * h) codes).  The labels kept are those of the last assignment, the codebook the updated one.        */
int mhip_vq_template_create(mhip_ctx* ctx, const uint8_t* frame, int on_device, int H, int W, const int32_t* box,
                            const int32_t* init_idx, int n_init, mhip_vq_template** out);
int mhip_vq_template_destroy(mhip_vq_template* t);
/* codes, iterations run, labels uint8 [h*w] and codebook fp32 [K][27] (any pointer may be NULL)                               */
int mhip_vq_template_state(mhip_vq_template* t, int* n_codes, int* iterations, uint8_t* labels_out, float* codebook_out);
/* the filter bank and the template's responses fp32 [filters][K] (get_template_features); required before a match             */
int mhip_vq_template_set_filters(mhip_vq_template* t, const float* responses, const mhip_vq_filters* filters);
/* Every window (win_h x win_w at win_xy[n_win][2] = x, y of a device page with rows page_pitch bytes apart) against every
 * template: code map, heat map and max_objects rounds of arg-max + suppression, launched over the (window, template) grid.
 * Only the peaks reach the host: peaks_out fp32 [n_win][n_templates][max_objects][3] = row, col, value.                     */
int mhip_vq_match(mhip_ctx* ctx, const uint8_t* page_dev, int page_h, int page_w, size_t page_pitch, const int32_t* win_xy,
                  int n_win, int win_h, int win_w, mhip_vq_template* const* templates, int n_templates, int max_objects,
                  float* peaks_out);
/* The kernels alone on host arrays (parity tests).  vq_assign: codes_out uint8 [h*w] of `rect` of image [H][W][3].           */
int mhip_vq_assign_host(mhip_ctx* ctx, const uint8_t* image, int H, int W, const int32_t* rect, const float* codebook,
                        int n_codes, uint8_t* codes_out);
/* one k-means iteration from centroids_in [K][27]: labels uint8 [h*w], the updated centroids (an empty cluster's is zero),
 * members per cluster int32 [K] and error = sum (new - old)^2                                                               */
int mhip_vq_kmeans_step_host(mhip_ctx* ctx, const uint8_t* image, int H, int W, const int32_t* rect, const float* centroids_in,
                             int n_codes, uint8_t* labels_out, float* centroids_out, int32_t* counts_out, double* error_out);
/* code map uint8 [H][W] -> heat fp32 [H][W] (GaussHaarFilters.get_query_map) and each filter's minimum fp64 [filters] or NULL */
int mhip_vq_heatmap_host(mhip_ctx* ctx, const uint8_t* codes, int H, int W, int n_codes, const float* responses,
                         const mhip_vq_filters* filters, float* heat_out, double* minima_out);
/* n heat maps fp32 [n][H][W], updated in place; box_wh int32 [n][2] = the template box's w, h -> peaks fp32 [n][max_objects][3] */
int mhip_vq_peaks_host(mhip_ctx* ctx, float* heat, int n, int H, int W, const int32_t* box_wh, int max_objects,
                       float* peaks_out);
/* cosine similarity of the colour features of n pairs of clips uint8 [n][h][w][3] -> fp32 [n]                                 */
int mhip_clip_cosine_host(mhip_ctx* ctx, const uint8_t* a, const uint8_t* b, int n, int h, int w, float* out);

/* ---- n-gram text matching (csrc/lev_ngrams.hip) ------------------------------------------------------------------------- */
/* replaces: the Levenshtein.distance of every (template text, page n-gram) pair that MetaTemplateMatcher.predict / score take
 * one at a time, marie/components/template_matching/meta_template_matching.py:152-187,277-281.  Unit-cost edit distance over
 * code points.  The page is one string S of L alphabet ids (1 .. alphabet: the code points of the template texts; 0: any other
 * code point, equal to nothing); word i spans S[ws[i]:we[i]], fs[i] is the first non-blank position >= ws[i] of S and le[i]
 * one past the last non-blank position < we[i], so that candidate (i, n) — words i .. i + n - 1, joined and stripped — is
 * S[a:b], a = min(fs[i], we[i + n - 1]), b = max(le[i + n - 1], a).  line_ids int32 [N] or NULL: with them a candidate whose
 * words do not share one id is none.  Templates: ids concatenated, template t = tmpl_ids[tmpl_off[t]:tmpl_off[t + 1]] (0 ..
 * 1024 ids, each 1 .. alphabet), g[t] >= 1 its word count; the candidate sizes are n = g[t] - 1 + k, k = 0, 1, 2.
 * -> dist, len int32 [T][3][N]: the distance and the candidate's length, or -1 where there is no candidate (n outside 1 .. N,
 * i > N - n, or differing line ids).  MHIP_EINVAL for a pattern over 1024 ids or a bit table ((alphabet + 1) * ceil(m / 64)
 * 64-bit words) over the 64 KiB of LDS budgeted for it.                                                                       */
int mhip_lev_ngrams_host(mhip_ctx* ctx, const uint16_t* page_ids, int L, const int32_t* ws, const int32_t* we, const int32_t* fs,
                         const int32_t* le, const int32_t* line_ids, int N, const uint16_t* tmpl_ids, const int32_t* tmpl_off,
                         const int32_t* g, int T, int alphabet, int32_t* dist_out, int32_t* len_out);

/* ---- CLIP vision tower: image embeddings of the matcher's snippet score (csrc/clip_api.hip, clip_ops.hip) --------------- */
/* replaces: CLIP.encode_image behind OpenAIEmbeddings.get_single_image_embedding, marie/embeddings/openai/
 * openai_embeddings.py:146-157 (clip/model.py VisionTransformer), CLIPModel.get_image_features behind
 * OpenAITransformerEmbeddings (openai_trans_embeddings.py:131-145), and the nn.CosineSimilarity of two embeddings in
 * VQNNFTemplateMatcher.score, marie/components/template_matching/vqnnf_template_matching.py:335-347.
 * "clipvis", not "clip": mhip_clip_cosine_host above is the colour-feature cosine of snippet clips.
 * Clips are uint8 [image_size][image_size][3], already resized and cropped; normalisation (pixel / 255 - mean_c) / std_c with
 * CLIP's constants.  Pre-LN layers with quick-GELU, class row -> post_layernorm -> projection (no bias) -> fp32 [proj_dim].   */
typedef struct mhip_clipvis mhip_clipvis;
typedef struct mhip_clipvis_config {
  int dim, depth, heads;   /* 768/12/12 ViT-B; head dim must be 64, dim <= 1024.  Tokens: 1 + (image_size / patch)^2        */
  int patch;               /* 32 (ViT-B/32), 16 (ViT-B/16): a multiple of 8 that divides image_size                       */
  int image_size;          /* 224                                                                                         */
  int ffn;                 /* 3072; a multiple of 64                                                                      */
  int proj_dim;            /* 512                                                                                         */
  float ln_eps;            /* 1e-5                                                                                        */
} mhip_clipvis_config;
int mhip_clipvis_create(mhip_ctx* ctx, int precision, const mhip_clipvis_config* cfg, mhip_clipvis** out);
int mhip_clipvis_destroy(mhip_clipvis* m);
/* keys of the OpenAI checkpoint's vision tower: visual.conv1.weight, visual.class_embedding, visual.positional_embedding,
 * visual.ln_pre.*, visual.transformer.resblocks.N.{ln_1,attn.in_proj_weight,attn.in_proj_bias,attn.out_proj,ln_2,mlp.c_fc,
 * mlp.c_proj}.*, visual.ln_post.*, visual.proj [dim][proj_dim]; any other key is MHIP_EINVAL                                 */
int mhip_clipvis_set_tensor(mhip_clipvis* m, const char* key, const float* data, const int64_t* shape, int ndim);
int mhip_clipvis_finalize(mhip_clipvis* m);
int mhip_clipvis_alloc_arena(mhip_clipvis* m);
int mhip_clipvis_arena(mhip_clipvis* m, void** arena_dev, size_t* bytes);
/* bytes of context workspace one mhip_clipvis_embed_host call of B clips lays out (0: bad arguments)                         */
size_t mhip_clipvis_workspace_bytes(mhip_clipvis* m, int B);
/* B host clips -> emb_out fp32 [B][proj_dim].  swap_rb: the clips are stored BGR                                            */
int mhip_clipvis_embed_host(mhip_clipvis* m, const uint8_t* clips_host, int B, int swap_rb, float* emb_out);
/* n_clips BGR host clips through the encoder once, then cos_out[p] = x.y / max(|x| |y|, 1e-8) of the embeddings of clips
 * pair_a[p], pair_b[p] (fp32 [n_pairs]); emb_out fp32 [n_clips][proj_dim] or NULL                                           */
int mhip_clipvis_embed_pairs_host(mhip_clipvis* m, const uint8_t* clips_host, int n_clips, const int32_t* pair_a,
                                  const int32_t* pair_b, int n_pairs, float* emb_out, float* cos_out);
/* as embed_host, plus the residual stream after the embedding kernel (pre_layrnorm applied) and after every layer:
 * taps_out fp32 [depth + 1][B][tokens][dim]; emb_out may be NULL                                                             */
int mhip_clipvis_debug_taps_host(mhip_clipvis* m, const uint8_t* clips_host, int B, int swap_rb, float* taps_out, float* emb_out);
/* The kernels alone on host arrays (parity tests).  quick-GELU of x fp32 [n] rounded to the precision's element type, n % 8 == 0 */
int mhip_clipvis_quick_gelu_host(mhip_ctx* ctx, int precision, const float* x, int n, float* out);
/* patches fp32 [B][n_tok - 1][D], cls [D], pos [n_tok][D], LayerNorm g / b [D] -> h_out fp32 [B][roundup(n_tok, 8)][D]
 * (rows past n_tok are zeros)                                                                                               */
int mhip_clipvis_embed_rows_host(mhip_ctx* ctx, const float* patches, const float* cls, const float* pos, const float* g,
                                 const float* b, int B, int n_tok, int D, float eps, float* h_out);
/* h fp32 [B][npad][D] (row 0 of every image is used), LayerNorm g / b [D], proj [D][E] -> emb_out fp32 [B][E]                */
int mhip_clipvis_head_host(mhip_ctx* ctx, const float* h, int B, int npad, int D, const float* g, const float* b, float eps,
                           const float* proj, int E, float* emb_out);
/* emb fp32 [n][E], pairs of row indices -> cos_out fp32 [n_pairs]                                                             */
int mhip_clipvis_pair_cosine_host(mhip_ctx* ctx, const float* emb, int n, int E, const int32_t* pair_a, const int32_t* pair_b,
                                  int n_pairs, float* cos_out);

/* ---- CLIP ModifiedResNet tower: the snippet embeddings of RN50 / RN101 / RN50x4 (csrc/cliprn_api.hip, cliprn_ops.hip) ------ */
/* replaces: CLIP.encode_image behind OpenAIEmbeddings.get_single_image_embedding (marie/embeddings/openai/openai_embeddings.py:
 * 146-157) for the ModifiedResNet checkpoints (clip/model.py: ModifiedResNet, Bottleneck, AttentionPool2d) — the model
 * VQNNFTemplateMatcher and MetaTemplateMatcher build by default, marie/clip-snippet-rn50x4.
 * Clips are uint8 [image_size][image_size][3], already resized and cropped; normalisation with CLIP's constants is part of the
 * stem kernel.  Stem (three 3 x 3 convolutions, the first with stride 2, and a 2 x 2 average pool), four layers of Bottleneck
 * blocks whose strides are average pools, and the attention pool: the mean token as the only query over the mean token and
 * the map's rows, heads of 64, c_proj -> fp32 [proj_dim].  Every BatchNorm (eval mode) is folded into its convolution.
 * Geometry as clip.build_model derives it: embed_dim = 32 width, heads = embed_dim / 64, tokens = (image_size / 32)^2 + 1.     */
typedef struct mhip_cliprn mhip_cliprn;
typedef struct mhip_cliprn_config {
  int width;               /* 80 (RN50x4), 64 (RN50, RN101): even, up to 128                                               */
  int layers[4];           /* 4, 6, 10, 6 (RN50x4); 3, 4, 6, 3 (RN50); 3, 4, 23, 3 (RN101): blocks per layer, 1 .. 64       */
  int image_size;          /* 288 (RN50x4), 224: a multiple of 32 up to 512                                                */
  int proj_dim;            /* 640 (RN50x4), 1024 (RN50), 512 (RN101)                                                      */
  float bn_eps;            /* 1e-5                                                                                        */
} mhip_cliprn_config;
/* MHIP_EINVAL, naming it: an image_size that is no multiple of 32 or above 512, an odd width (heads not 64 wide), a width
 * above 128, a layers entry below 1                                                                                         */
int mhip_cliprn_create(mhip_ctx* ctx, int precision, const mhip_cliprn_config* cfg, mhip_cliprn** out);
int mhip_cliprn_destroy(mhip_cliprn* m);
/* keys of the OpenAI checkpoint's vision tower: visual.conv{1,2,3}.weight, visual.bn{1,2,3}.*, visual.layerL.N.{conv1,bn1,conv2,
 * bn2,conv3,bn3,downsample.0,downsample.1}.*, visual.attnpool.{positional_embedding,q_proj,k_proj,v_proj,c_proj}.*;
 * num_batches_tracked is dropped; a key outside visual. is MHIP_EINVAL.  finalize folds the BatchNorms, pads the channel
 * counts conv2d_nhwc does not take with zeros, and names the first missing or misshapen tensor                                */
int mhip_cliprn_set_tensor(mhip_cliprn* m, const char* key, const float* data, const int64_t* shape, int ndim);
int mhip_cliprn_finalize(mhip_cliprn* m);
int mhip_cliprn_alloc_arena(mhip_cliprn* m);
int mhip_cliprn_arena(mhip_cliprn* m, void** arena_dev, size_t* bytes);
/* bytes of context workspace one mhip_cliprn_embed_host call of B clips lays out (0: bad arguments)                          */
size_t mhip_cliprn_workspace_bytes(mhip_cliprn* m, int B);
/* B (up to 1024) host clips -> emb_out fp32 [B][proj_dim].  swap_rb: the clips are stored BGR                                */
int mhip_cliprn_embed_host(mhip_cliprn* m, const uint8_t* clips_host, int B, int swap_rb, float* emb_out);
/* n_clips BGR host clips through the tower once, then cos_out[p] = x.y / max(|x| |y|, 1e-8) of the embeddings of clips
 * pair_a[p], pair_b[p] (fp32 [n_pairs]); emb_out fp32 [n_clips][proj_dim] or NULL                                           */
int mhip_cliprn_embed_pairs_host(mhip_cliprn* m, const uint8_t* clips_host, int n_clips, const int32_t* pair_a,
                                 const int32_t* pair_b, int n_pairs, float* emb_out, float* cos_out);
/* shape (H, W, C) of tap i: 0 the stem after its pool, 1 .. 4 the layers, 5 the embedding (1, 1, proj_dim)                    */
int mhip_cliprn_tap_shape(mhip_cliprn* m, int i, int32_t shape[3]);
/* as embed_host, plus taps 0 .. 4 one after another in taps_out: fp32 [B][H][W][C] each, the checkpoint's channel counts
 * (no padding channels); emb_out may be NULL                                                                                */
int mhip_cliprn_debug_taps_host(mhip_cliprn* m, const uint8_t* clips_host, int B, int swap_rb, float* taps_out, float* emb_out);
/* The kernels alone on host arrays (parity tests).  The stem's first convolution: clips u8 [B][S][S][3] (S even), w fp32
 * [C0][3][3][3], scale / bias [C0] (the folded BatchNorm) -> out fp32 [B][S/2][S/2][C0] = relu(scale * conv(normalised clip) +
 * bias), rounded to the precision's element type; stride 2, pad 1, zeros around the normalised clip                          */
int mhip_cliprn_stem_host(mhip_ctx* ctx, int precision, const uint8_t* clips, int B, int S, int swap_rb, const float* w,
                          const float* scale, const float* bias, int C0, float* out);
/* x fp32 [B][H][W][C] (rounded to the precision's element type) -> out fp32 [B][H/k][W/k][C]: k x k means, k = 2; H and W
 * multiples of k and C of 8 (f16) / 4 (f32), else MHIP_EINVAL                                                                */
int mhip_avgpool_nhwc_host(mhip_ctx* ctx, int precision, const float* x, int B, int H, int W, int C, int k, float* out);
/* the attention pool: x fp32 [B][HW][E] (the last map), pos [HW + 1][E], q / k / v projections w [E][E] + b [E], c_proj wc
 * [P][E] + bc [P] -> emb_out fp32 [B][P]; HW up to 256, E a multiple of 64 up to 4096                                        */
int mhip_cliprn_attnpool_host(mhip_ctx* ctx, int precision, const float* x, const float* pos, const float* wq, const float* bq,
                              const float* wk, const float* bk, const float* wv, const float* bv, const float* wc,
                              const float* bc, int B, int HW, int E, int P, float* emb_out);

/* ---- CLIP text tower: text embeddings (csrc/cliptext_api.hip, cliptext_ops.hip, attn_seq.hip) ----------------------------- */
/* replaces: CLIP.encode_text behind OpenAIEmbeddings.get_text_embedding, marie/embeddings/openai/openai_embeddings.py:122-129,
 * 159-164 (clip/model.py: token_embedding + positional_embedding, the causal transformer, ln_final, the end-of-text row,
 * text_projection), CLIPModel.get_text_features of transformers.  Token ids come from the caller (marie_icr_amd/
 * clip_tokenizer.py): int32 [B][npad], npad a multiple of 8 up to the context rounded up to 8, the same for every text of a
 * call; eot[b] is the row of text b's end-of-text token, the row that is normalised and projected.  Every row is computed under
 * the causal mask, so what follows a text's end-of-text token (padding ids) cannot reach it, and a text's embedding does not
 * depend on the other texts of the call or on npad, bit for bit.  Pre-LN layers with quick-GELU, fp32 [proj_dim] out.          */
typedef struct mhip_cliptext mhip_cliptext;
typedef struct mhip_cliptext_config {
  int vocab;               /* 49408                                                                                       */
  int context;             /* 77; at most 128                                                                             */
  int dim, heads, depth;   /* 512/8/12 (ViT-B/32's text tower); head dim must be 64, dim <= 1024                           */
  int ffn;                 /* 2048; a multiple of 64                                                                      */
  int proj_dim;            /* 512                                                                                         */
  float ln_eps;            /* 1e-5                                                                                        */
} mhip_cliptext_config;
int mhip_cliptext_create(mhip_ctx* ctx, int precision, const mhip_cliptext_config* cfg, mhip_cliptext** out);
int mhip_cliptext_destroy(mhip_cliptext* m);
/* keys of the OpenAI checkpoint's text tower: token_embedding.weight, positional_embedding, transformer.resblocks.N.{ln_1,
 * attn.in_proj_weight,attn.in_proj_bias,attn.out_proj,ln_2,mlp.c_fc,mlp.c_proj}.*, ln_final.*, text_projection
 * [dim][proj_dim]; any other key is MHIP_EINVAL                                                                              */
int mhip_cliptext_set_tensor(mhip_cliptext* m, const char* key, const float* data, const int64_t* shape, int ndim);
int mhip_cliptext_finalize(mhip_cliptext* m);
int mhip_cliptext_alloc_arena(mhip_cliptext* m);
int mhip_cliptext_arena(mhip_cliptext* m, void** arena_dev, size_t* bytes);
/* bytes of context workspace one mhip_cliptext_embed_host call of B texts of npad rows lays out (0: bad arguments)           */
size_t mhip_cliptext_workspace_bytes(mhip_cliptext* m, int B, int npad);
/* B texts (1 .. 4096) -> emb_out fp32 [B][proj_dim].  MHIP_EINVAL, never a clamp: npad no multiple of 8 or above the context
 * rounded up to 8, an id outside [0, vocab), an eot outside [1, npad)                                                         */
int mhip_cliptext_embed_host(mhip_cliptext* m, const int32_t* ids, const int32_t* eot, int B, int npad, float* emb_out);
/* the texts through the tower once, then cos_out[p] = x.y / max(|x| |y|, 1e-8) of the embeddings of texts pair_a[p], pair_b[p]
 * (fp32 [n_pairs]); emb_out fp32 [B][proj_dim] or NULL                                                                        */
int mhip_cliptext_embed_pairs_host(mhip_cliptext* m, const int32_t* ids, const int32_t* eot, int B, int npad,
                                   const int32_t* pair_a, const int32_t* pair_b, int n_pairs, float* cos_out, float* emb_out);
/* as embed_host, plus the residual stream after the embedding kernel and after every layer: taps_out fp32
 * [depth + 1][B][npad][dim] (rows at positions past the context have a zero position row); emb_out may be NULL                */
int mhip_cliptext_debug_taps_host(mhip_cliptext* m, const int32_t* ids, const int32_t* eot, int B, int npad, float* taps_out,
                                  float* emb_out);
/* The kernels alone on host arrays (parity tests).  table fp32 [vocab][D], pos [npad][D], ids [B][npad] -> h_out [B][npad][D]  */
int mhip_cliptext_embed_rows_host(mhip_ctx* ctx, const float* table, const float* pos, const int32_t* ids, int B, int npad,
                                  int vocab, int D, float* h_out);
/* causal attention of B sequences of npad rows: q, k, v fp32 [B][npad][heads * 64], q already scaled by head_dim^-0.5 * log2(e);
 * rounded to the precision's element type and laid out as the tower lays them out (q | k rows, V^T) -> out fp32, same shape    */
int mhip_cliptext_attention_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v, int B, int heads,
                                 int npad, float* out);
/* h fp32 [B][npad][D], row row_of[i] of block i -> LayerNorm g / b [D] -> proj [D][E] -> emb_out fp32 [B][E]                   */
int mhip_cliptext_head_host(mhip_ctx* ctx, const float* h, int B, int npad, int D, const float* g, const float* b, float eps,
                            const float* proj, int E, const int32_t* row_of, float* emb_out);

/* ---- BERT sentence encoders: text embeddings (csrc/berttext_api.hip, berttext_ops.hip, attn_seq.hip) ---------------------- */
/* replaces: SentenceTransformer.encode behind SentenceTransformerEmbeddings.get_embeddings (marie/embeddings/sentence_transformers/
 * sentence_transformers_embeddings.py, all-MiniLM-L6-v2) and JinaEmbeddings.get_embeddings (marie/embeddings/jina/
 * jina_embeddings.py, jina-embeddings-v2-base-en): BertModel without the pooler — or JinaBERT: no position table, the symmetric
 * ALiBi bias -slope_h |i - j| on the scores, a gated GELU MLP — then masked mean (or [CLS]) pooling and, where asked for, L2
 * normalisation.  Token ids come from the caller (marie_icr_amd/wordpiece_tokenizer.py): int32 [B][npad], npad a multiple of 8 up
 * to 8192 (ALiBi) or to the position table's rows, whichever is less, the same for every text of a call; len[b] in [1, npad] is
 * text b's token count ([CLS] .. [SEP]), the rows after it carry the [PAD] id.  Calls of npad <= 128 hold a text's keys in LDS
 * (attn_short); longer ones stream them in blocks of 128 under an online soft-max (attn_long).  On each side of that boundary a
 * text's embedding does not depend on the other texts of the call or on npad, bit for bit.  A call lays out at most
 * 4096 * 128 = 524288 rows (B * npad).  Post-LN layers, fp32 [dim] out.
 * The same encoder runs three more families once their keys are renamed onto BERT's (marie_icr_amd/embeddings.py:
 * load_sentence_encoder_state): RoBERTa (pos_offset 2, one token type), DistilBERT (no token types) and MPNet (pos_offset 2, no
 * token types, and MPNetEncoder's relative attention bias: one table [rel_buckets][heads] shared by the layers, added to the scores
 * as a function of query - key clamped to +-rel_max_distance).                                                                */
typedef struct mhip_berttext mhip_berttext;
typedef struct mhip_berttext_config {
  int vocab;               /* 30522                                                                                       */
  int max_position;        /* 512: rows of the position table (position 0 only)                                           */
  int type_vocab;          /* 2: row 0 of the token type table is added to every token; 0 (create_ex only): no token type
                              table, no term                                                                              */
  int dim, heads, depth;   /* 384/12/6 (all-MiniLM-L6-v2), 768/12/12 (jina-v2-base); head dim 64 or 32, dim a multiple of
                              64 up to 1024                                                                               */
  int ffn;                 /* 1536 / 3072; a multiple of 64                                                               */
  float ln_eps;            /* 1e-12                                                                                       */
  int position;            /* 0 absolute (a learned table), 1 alibi                                                       */
  int mlp;                 /* 0 gelu (intermediate.dense + erf-GELU), 1 geglu (gated_layers: gelu(x W_a^T) * (x W_b^T))  */
  int pool;                /* 0 mean over the len[b] tokens, 1 cls (row 0)                                               */
  int normalize;           /* 1: divide the pooled row by max(its L2 norm, 1e-12)                                         */
} mhip_berttext_config;
/* the same with the fields of the other families appended; zero in each is the behaviour without it.  (A struct of its own, and
 * mhip_berttext_create_ex below: callers of mhip_berttext_create pass the twelve fields above and nothing behind them.)       */
typedef struct mhip_berttext_config_ex {
  mhip_berttext_config base;
  int pos_offset;          /* the position row of token t is pos_offset + t (RoBERTa, MPNet: pad_id + 1 = 2); a text then
                              has at most max_position - pos_offset tokens                                                */
  int rel_buckets;         /* 0: no relative attention bias; otherwise even and >= 4 (MPNet: 32), and the tensor
                              encoder.relative_attention_bias.weight [rel_buckets][heads] is taken.  Not with alibi       */
  int rel_max_distance;    /* MPNet: 128.  finalize refuses (naming this field) a pair whose bucket still changes past
                              this distance: the table is indexed by the distance clamped to it                           */
} mhip_berttext_config_ex;
/* MHIP_EINVAL with a message that names the field: a head dim other than 64 or 32, dim above 1024, dim or ffn no multiple of 64,
 * an unknown position / mlp / pool / normalize value                                                                          */
int mhip_berttext_create(mhip_ctx* ctx, int precision, const mhip_berttext_config* cfg, mhip_berttext** out);
/* as create, plus: type_vocab 0 is legal; MHIP_EINVAL naming the field for a pos_offset that leaves fewer than 2 position rows (or
 * any with alibi), rel_buckets odd or below 4 (or any with alibi: slopes and a table together), rel_max_distance outside
 * 1 .. 8192 with rel_buckets or non-zero without                                                                              */
int mhip_berttext_create_ex(mhip_ctx* ctx, int precision, const mhip_berttext_config_ex* cfg, mhip_berttext** out);
/* the same with Longformer's windowed attention and a sequence-classification head appended (LongformerForSequenceClassification
 * as pipeline("text-classification") runs it: global attention on <s> alone).  In layer l a token i >= 1 attends to token 0 and to
 * the tokens max(1, i - w_l) .. min(len - 1, i + w_l), w_l = attention_window[l] / 2 (attn_window); token 0 attends to all of them
 * through query_global / key_global / value_global (attn_global_row); logits = out_proj(tanh(dense(row 0))) (cls_head).            */
typedef struct mhip_berttext_config_cls {
  mhip_berttext_config_ex ex;      /* RoBERTa's front: pos_offset 2, type_vocab 1; position absolute, no rel_buckets; heads of 64  */
  const int* attention_window;     /* [depth] the two-sided window of every layer as config.json holds it: even, 2 .. 1024         */
  int num_labels;                  /* 1 .. 1024                                                                                  */
  int head_function;               /* scores of classify_host: 0 the logits, 1 their soft-max, 2 their sigmoid                   */
} mhip_berttext_config_cls;
/* as create_ex, plus MHIP_EINVAL naming the field: attention_window NULL, odd or not positive, a one-sided window above 512;
 * num_labels outside 1 .. 1024; an unknown head_function; a head dimension other than 64; alibi or rel_buckets.  set_tensor then
 * takes, in addition, encoder.layer.N.attention.self.{query,key,value}_global.* and classifier.{dense,out_proj}.* (a "longformer."
 * prefix is stripped as "bert." is), and finalize names the first of them that is missing.  embed_host and debug_taps_host work
 * on such a handle: they pool, and tap, the windowed encoder's rows                                                           */
int mhip_berttext_create_cls(mhip_ctx* ctx, int precision, const mhip_berttext_config_cls* cfg, mhip_berttext** out);
int mhip_berttext_destroy(mhip_berttext* m);
/* keys of Hugging Face BERT (an optional "bert." prefix is stripped): embeddings.{word,position,token_type}_embeddings.weight,
 * embeddings.LayerNorm.*, encoder.layer.N.attention.self.{query,key,value}.*, attention.output.{dense,LayerNorm}.*,
 * intermediate.dense.*, output.{dense,LayerNorm}.*; with mlp = geglu the MLP is JinaBERT's encoder.layer.N.mlp.gated_layers.weight
 * [2 ffn][dim] (no bias; first the GELU half, then the linear half), mlp.wo.*, mlp.layernorm.*, and position = alibi takes no
 * position table; with rel_buckets encoder.relative_attention_bias.weight (finite values).  pooler.* and
 * embeddings.position_ids are ignored; any other key is MHIP_EINVAL.  finalize names the first
 * missing or misshapen tensor                                                                                                 */
int mhip_berttext_set_tensor(mhip_berttext* m, const char* key, const float* data, const int64_t* shape, int ndim);
int mhip_berttext_finalize(mhip_berttext* m);
int mhip_berttext_alloc_arena(mhip_berttext* m);
int mhip_berttext_arena(mhip_berttext* m, void** arena_dev, size_t* bytes);
/* bytes of context workspace one mhip_berttext_embed_host (or debug_taps_host, classify_host) call of B texts of npad rows lays out (0: bad
 * arguments); mhip_berttext_embed_pairs_host lays out three arrays of 4 * n_pairs bytes more, each rounded up to 256            */
size_t mhip_berttext_workspace_bytes(mhip_berttext* m, int B, int npad);
/* the ALiBi slopes of `heads` heads, fp32 [heads]: 2^(-8 (i + 1) / n) for n a power of two; otherwise those of the largest power
 * of two p <= n, then the even-indexed slopes of 2 p, the first n - p of them.  Host only, no ctx                              */
int mhip_berttext_alibi_slopes(int heads, float* slopes_out);
/* MPNet's relative attention bias as the encoder folds it, before the log2(e) factor: table_out fp32 [heads][2 R + 1], R =
 * max_distance, table_out[h][d + R] = weight[bucket(-d)][h] for d = query - key in -R .. R, weight fp32 [buckets][heads], bucket
 * MPNetEncoder.relative_position_bucket(key - query, buckets, max_distance) in float32 as the library computes it.  MHIP_EINVAL
 * where the bucket still changes past +-R (up to 8192): clamping the distance would then differ from the model.  Host only, no ctx */
int mhip_berttext_rel_table(int buckets, int max_distance, const float* weight, int heads, float* table_out);
/* B texts (1 .. 4096) -> emb_out fp32 [B][dim].  MHIP_EINVAL, never a clamp: npad no multiple of 8 or above 8192 (or above the
 * position table rounded up to 8), more than 524288 rows (B * npad), a len outside [1, npad], an id outside [0, vocab)        */
int mhip_berttext_embed_host(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad, float* emb_out);
/* B texts through the encoder and the classification head: logits_out, scores_out fp32 [B][num_labels] (scores: head_function of
 * the logits).  The arguments and refusals of embed_host; MHIP_ESTATE on a handle without a head (not from create_cls).  A text's
 * logits do not depend on the other texts of the call or on npad, bit for bit                                                  */
int mhip_berttext_classify_host(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad, float* logits_out,
                                float* scores_out);
/* the texts through the encoder once, then cos_out[p] = x.y / max(|x| |y|, 1e-8) of the embeddings of texts pair_a[p], pair_b[p]
 * (fp32 [n_pairs]); emb_out fp32 [B][dim] or NULL                                                                             */
int mhip_berttext_embed_pairs_host(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad,
                                   const int32_t* pair_a, const int32_t* pair_b, int n_pairs, float* cos_out, float* emb_out);
/* as embed_host, plus the residual stream after the embedding kernel and after every layer: taps_out fp32
 * [depth + 1][B][npad][dim] (rows >= len[b] hold finite values nobody reads); emb_out may be NULL                             */
int mhip_berttext_debug_taps_host(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad, float* taps_out,
                                  float* emb_out);
/* The kernels alone on host arrays (parity tests).  word fp32 [vocab][D], type0 [D], pos [npad][D] or NULL, LayerNorm g / b [D],
 * ids [B][npad] -> h_out [B][npad][D] = LN(word[id] + type0 (+ pos[t]))                                                       */
int mhip_berttext_embed_rows_host(mhip_ctx* ctx, const float* word, const float* type0, const float* pos, const float* g,
                                  const float* b, float eps, const int32_t* ids, int B, int npad, int vocab, int D, float* h_out);
/* the same with type0 NULL (no token type term) and the position row of token t at pos_offset + t: pos fp32
 * [pos_offset + npad][D] or NULL                                                                                              */
int mhip_berttext_embed_rows_ex_host(mhip_ctx* ctx, const float* word, const float* type0, const float* pos, const float* g,
                                     const float* b, float eps, const int32_t* ids, int B, int npad, int vocab, int D, int pos_offset,
                                     float* h_out);
/* attention of B sequences of npad rows over their first len[b] keys: q, k, v fp32 [B][npad][heads * head_dim], q already scaled
 * by head_dim^-0.5 * log2(e), slopes [heads] in the same log2 units or NULL (no bias term); rounded to the precision's element
 * type and laid out as the encoder lays them out (q | k rows, V^T) -> out fp32, same shape                                    */
int mhip_berttext_attention_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v, const int32_t* len,
                                 const float* slopes, int B, int heads, int head_dim, int npad, float* out);
/* the same through the streamed kernel (attn_long): npad a multiple of 8, 8 .. 8192 (128 and fewer rows too: one key block through
 * the streamed code), at most 524288 rows (B * npad).  mhip_berttext_attention_host keeps its limit of 128 rows                 */
int mhip_berttext_attention_long_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v,
                                      const int32_t* len, const float* slopes, int B, int heads, int head_dim, int npad, float* out);
/* the two attention entries with a relative-distance table in place of the slopes: the score of (query i, key j) gets
 * table[head][clamp(i - j, -radius, radius) + radius]; table fp32 [heads][2 radius + 1] in the log2 units of q, finite (a
 * non-finite value is MHIP_EINVAL), or NULL: then the result is that of the entry above with slopes NULL, bit for bit        */
int mhip_berttext_attention_rel_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v, const int32_t* len,
                                     const float* table, int radius, int B, int heads, int head_dim, int npad, float* out);
int mhip_berttext_attention_rel_long_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v,
                                          const int32_t* len, const float* table, int radius, int B, int heads, int head_dim, int npad,
                                          float* out);
/* attn_window alone, on the layout of the entries above (head_dim 64): query i of sequence b over key 0 and the keys
 * max(1, i - w) .. min(len[b] - 1, i + w), w one-sided in 1 .. 512; npad a multiple of 8 up to 8192.  Row 0 and the rows >= len[b]
 * come back finite and mean nothing                                                                                            */
int mhip_berttext_attention_window_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v,
                                        const int32_t* len, int w, int B, int heads, int head_dim, int npad, float* out);
/* attn_global_row alone: qg fp32 [B][heads * 64] (scaled like q above, kept fp32), kg, vg fp32 [B][npad][heads * 64] rounded to the
 * precision's element type -> out fp32 [B][heads * 64] = softmax(qg . kg[j], j < len[b]) vg per head                            */
int mhip_berttext_attention_global_host(mhip_ctx* ctx, int precision, const float* qg, const float* kg, const float* vg,
                                        const int32_t* len, int B, int heads, int npad, float* out);
/* cls_head alone, fp32: h0 [B][D], dense_w [D][D], dense_b [D], out_w [L][D], out_b [L] -> logits_out, scores_out [B][L];
 * function 0 / 1 / 2 as head_function.  D a multiple of 64 up to 1024, L up to 1024                                             */
int mhip_berttext_cls_head_host(mhip_ctx* ctx, const float* h0, const float* dense_w, const float* dense_b, const float* out_w,
                                const float* out_b, int B, int D, int L, int function, float* logits_out, float* scores_out);
/* x fp32 [R][2 F], rounded to the precision's element type -> out fp32 [R][F] = gelu_erf(x[:, :F]) * x[:, F:]                 */
int mhip_berttext_geglu_host(mhip_ctx* ctx, int precision, const float* x, int R, int F, float* out);
/* h fp32 [B][npad][D], len [B] -> emb_out fp32 [B][D]: mode 0 the mean of rows < len[b], 1 row 0; normalize 0 / 1            */
int mhip_berttext_pool_host(mhip_ctx* ctx, const float* h, const int32_t* len, int B, int npad, int D, int mode, int normalize,
                            float* emb_out);

/* ---- LayoutReader reading order (csrc/layoutreader_api.hip, layoutreader_ops.hip) ---------------------------------------- */
/* replaces: LayoutlmForSeq2SeqDecoder.forward (greedy: search_beam_size 1, pos_shift off) with layoutlm_only_layout_flag behind
 * TextLayout.forward (marie/document/layoutreader/text_layout.py; model in marie/models/unilm/layoutreader/s2s_ft/
 * modeling_decoding.py, rows laid out by Preprocess4Seq2seqDecoder).  S = max_source source rows ([CLS] at box 0, the n <= S - 2
 * words, [SEP] at box 1000, pads), then T = S - 2 greedy pointer steps; always all T.  A page's decisions and scores do not
 * depend on the other pages of the call, bit for bit.                                                                        */
typedef struct mhip_layoutreader mhip_layoutreader;
typedef struct mhip_layoutreader_config {
  int dim;                 /* 768; a multiple of 64 up to 1024                                                            */
  int heads;               /* 12; dim / heads must be 64                                                                  */
  int depth;               /* 12                                                                                          */
  int ffn;                 /* 3072; a multiple of 64                                                                      */
  int max_position;        /* 1024: rows of the position table, >= 2 S - 2                                                */
  int max_2d;              /* 1024: rows of the x / y / h / w tables, > 1000                                              */
  int max_source;          /* S = 513: source rows, and entries of cls.predictions.bias; 2 S - 1 <= 1032                  */
  int type_vocab;          /* 2                                                                                           */
  int source_type;         /* 0                                                                                           */
  int target_type;         /* 1                                                                                           */
  float ln_eps;            /* 1e-5, TF style (inside the root)                                                            */
} mhip_layoutreader_config;
/* MHIP_EINVAL with a message that names the field (a head dim other than 64 among them)                                     */
int mhip_layoutreader_create(mhip_ctx* ctx, int precision, const mhip_layoutreader_config* cfg, mhip_layoutreader** out);
int mhip_layoutreader_destroy(mhip_layoutreader* m);
/* keys of the checkpoint (an optional "bert." prefix is stripped), LayerNorms as weight / bias: embeddings.{position,x_position,
 * y_position,h_position,w_position,token_type}_embeddings.weight, embeddings.LayerNorm.*, encoder.layer.N.* as BERT's,
 * cls.predictions.bias [S], cls.predictions.transform.{dense,LayerNorm}.*.  pooler.*, cls.seq_relationship.*,
 * embeddings.word_embeddings.weight and every attention.self.key.bias are ignored (the model never reads them); any other key is
 * MHIP_EINVAL.  finalize names the first missing or misshapen tensor                                                         */
int mhip_layoutreader_set_tensor(mhip_layoutreader* m, const char* key, const float* data, const int64_t* shape, int ndim);
int mhip_layoutreader_finalize(mhip_layoutreader* m);
int mhip_layoutreader_alloc_arena(mhip_layoutreader* m);
int mhip_layoutreader_arena(mhip_layoutreader* m, void** arena_dev, size_t* bytes);
/* bytes of context workspace one mhip_layoutreader_order_host call of `pages` pages (1 .. 64) lays out, the key / value caches
 * [depth][pages][S + T][dim] among them (0: bad arguments); debug_host lays out the score rows and the forced indices on top */
size_t mhip_layoutreader_workspace_bytes(mhip_layoutreader* m, int pages);
/* boxes int32 [pages][S - 2][4] (x0, y0, x1, y1 in 0 .. 1000; rows >= counts[page] are not read), counts int32 [pages] ->
 * decisions int32 [pages][T]: the arg-max of every step (lowest index on ties), an index into the S source rows (the caller
 * subtracts 1 for word indices).  MHIP_EINVAL, never a clamp: a count outside 0 .. S - 2, a coordinate outside 0 .. 1000,
 * x1 < x0 or y1 < y0                                                                                                         */
int mhip_layoutreader_order_host(mhip_layoutreader* m, const int32_t* boxes, const int32_t* counts, int pages, int32_t* decisions);
/* as order_host, plus (each may be NULL) scores_out fp32 [pages][T][S]: every step's score row; emb_out fp32 [pages][S][dim]: the
 * embedded source rows the pointer head scores against; last_out fp32 [pages][S][dim]: the last layer's output of the source pass
 * (rows past a page's [SEP] are zeros: they are not computed).  forced int32 [pages][T] (0 .. S - 1) or NULL: step t + 1 is fed
 * source row forced[page][t] instead of decision t; decisions and scores still report the kernel's own arg-max                */
int mhip_layoutreader_debug_host(mhip_layoutreader* m, const int32_t* boxes, const int32_t* counts, int pages, const int32_t* forced,
                                 int32_t* decisions, float* scores_out, float* emb_out, float* last_out);
/* The decode attention alone on host arrays (parity tests), heads of 64: q, k, v fp32 [pages][nq][heads * 64] the nq (1 or 2)
 * rows a step feeds per page, q already scaled by 1/8 * log2(e); kc, vc fp32 [pages][cache_rows][heads * 64] the caches; all
 * rounded to the precision's element type.  Query row i of a page sees cache rows [0, src_len[page]), cache rows tgt_base +
 * [0, tgt_len[page * nq + i]) and rows 0 .. i of the page's k / v: at most 1032 keys.  -> out fp32 [pages][nq][heads * 64]    */
int mhip_layoutreader_attention_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v, const float* kc,
                                     const float* vc, const int32_t* src_len, const int32_t* tgt_len, int pages, int nq, int heads,
                                     int cache_rows, int tgt_base, float* out);

/* ---- word-box / line geometry of the DiT box processor (host, pure functions; no ctx) --------------------------------- */
/* replaces: merge_boxes, marie/utils/overlap.py:268-330 (find_overlap_horizontal(center_y_overlap=0.5) :106-183,
 * merge_bboxes_as_block :186-204).  xyxy fp32 [n][4] -> out_xyxy fp32 (capacity n rows), *n_out rows.       */
int mhip_merge_boxes(const float* xyxy, int n, float* out_xyxy, int* n_out);
/* replaces: line_merge, marie/boxes/line_processor.py:105-171.  xywh int32 [n][4] -> merged lines sorted by y
 * (capacity n rows).  Equal-y boxes keep input order (the reference leaves ties to numpy's unstable sort).   */
int mhip_line_merge(const int32_t* xywh, int n, int32_t* out_xywh, int* n_out);
/* replaces: find_line_number per box, marie/boxes/line_processor.py:15-44.  out[i] = 1-based line, -1 if no lines. */
int mhip_find_line_numbers(const int32_t* lines_xywh, int n_lines, const int32_t* boxes_xywh, int n, int32_t* out);
/* replaces: lines_from_bboxes, marie/boxes/dit/ulim_dit_box_processor.py:201-288 (rectangle mask, horizontal
 * erode+dilate, 4-connected components with stats, size filter, line_merge) for a height x width page.
 * Returns MHIP_ENOMEM with *n_out = needed rows when cap is too small.                                       */
int mhip_lines_from_bboxes(const float* xyxy, int n, int height, int width, int32_t* out_xywh, int cap, int* n_out);

/* ---- page ingest (the step before the detector) ------------------------------------------------------------------------ */
/* replaces: the shape rule of ensure_max_page_size, marie/utils/image_utils.py:275-310, for one frame (orientation-aware
 * maximum, expanded by expand_ratio; aspect-preserving, int() truncation).  Returns 1 and the new size when the frame is
 * too large, 0 (and the old size) when it is kept.  Host only, no ctx.                                                     */
int mhip_max_page_size(int width, int height, int max_w_portrait, int max_h_portrait, double expand_ratio, int* new_w,
                       int* new_h);
/* replaces: cv2.resize(frame, (new_width, new_height), interpolation=cv2.INTER_AREA), image_utils.py:313-315 — 8-bit,
 * 1 or 3 channels, shrinking only (dh <= sh, dw <= sw).  Device buffers; src rows src_pitch bytes apart, dst packed.        */
int mhip_resize_area_u8(mhip_ctx* ctx, const uint8_t* src_dev, int sh, int sw, int cn, size_t src_pitch, uint8_t* dst_dev,
                        int dh, int dw);
/* replaces: cv2.resize(image, (new_w, new_h), interpolation=cv2.INTER_CUBIC) in resize_image's shrink branch,
 * marie/utils/resize_image.py:53-61 (small pages / region crops framed for the DiT detector,
 * marie/boxes/dit/ulim_dit_box_processor.py:524-540).  8-bit, 1 or 3 channels, any scale.                                  */
int mhip_resize_cubic_u8(mhip_ctx* ctx, const uint8_t* src_dev, int sh, int sw, int cn, size_t src_pitch,
                         uint8_t* dst_dev, int dh, int dw);
int mhip_resize_cubic_u8_host(mhip_ctx* ctx, const uint8_t* src_host, int sh, int sw, int cn, uint8_t* dst_host, int dh,
                              int dw);
/* the same on packed host buffers (stages through the context workspace). */
int mhip_resize_area_u8_host(mhip_ctx* ctx, const uint8_t* src_host, int sh, int sw, int cn, uint8_t* dst_host, int dh,
                             int dw);

#ifdef __cplusplus
}
#endif
#endif /* MARIE_HIP_H */
