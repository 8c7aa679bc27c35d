// common.h — shared host/device declarations for libmarie_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/marie_hip.h"

// ------------------------------------------------------------------ kernel ids (profiling)
enum MhipKernelId {
  MHIP_K_CONV_FIRST = 0,  // u8 -> normalise -> conv3x3(1->64)+ReLU+maxpool2x2; also cliprn_stem (cliprn_ops.hip): u8 RGB -> normalise -> conv3x3 stride 2 + BN + ReLU
  MHIP_K_CONV_IGEMM = 1,  // NHWC implicit-GEMM conv / GEMM on MFMA, fused scale/bias/ReLU/pool
  MHIP_K_LSTM_REC = 2,    // BiLSTM recurrence (persistent over T, batch-sliced)
  MHIP_K_CTC_DECODE = 3,  // wave-shuffle argmax + softmax-max + collapse
  MHIP_K_IMAGE_OPS = 4,   // resize / max-pool / bilinear up-sample (HBM-bound, 16 B per lane); also avgpool_nhwc (cliprn_ops.hip)
  MHIP_K_CCL = 5,         // score-map binarise + connected components + per-component statistics
  MHIP_K_CROP_BATCH = 6,  // fragment -> gray -> Pillow-exact bicubic to height 32 -> replicate pad
  MHIP_K_ATTN = 7,        // attention decoder pieces (context, LSTM cell, arg-max)
  MHIP_K_ATTN_FLASH = 8,  // ViT softmax attention: S^T = K Q^T -> online softmax -> O^T = V^T P^T on MFMA
  MHIP_K_VIT_OPS = 9,     // LayerNorm, patch extraction, token/map moves (HBM-bound)
  MHIP_K_DET_OPS = 10,    // detector heads: anchors/decode, top-k, NMS, ROIAlign
  MHIP_K_DEC_OPS = 11,    // text decoder steps: embedding, single-query attention over caches, beam candidates; also the
                          // LayoutReader kernels (layoutreader_ops.hip): lr_embed, lr_decode_attn, lr_pointer_scores, lr_pointer_select,
                          // and the one-query attention of the ModifiedResNet's attention pool (cliprn_attn1q, cliprn_ops.hip)
  // conv_igemm by tile shape: their launches are ALSO counted in MHIP_K_CONV_IGEMM (ProfSlot::parent), so that the fraction of
  // the MFMA peak can be recomputed per variant from a profile (names as the kernels appear in a rocprofv3 trace)
  MHIP_K_IGEMM_T64 = 12,    // conv_igemm_kernel<.., 64, ..>   512 x 64 tile
  MHIP_K_IGEMM_T128 = 13,   // conv_igemm_kernel<.., 128, ..>  256 x 128 tile
  MHIP_K_IGEMM_T256 = 14,   // conv_igemm_kernel<.., 256, ..>  256 x 256 tile
  MHIP_K_IGEMM_S128 = 15,   // conv_igemm_kernel<.., 1128, ..> 128 x 128 tile (few-row GEMMs)
  MHIP_K_IGEMM_PATCH = 16,  // conv3x3_patch_kernel            3x3 / pad 1 convolutions
  MHIP_K_CROSS_ATTN = 17,   // decoder encoder-attention over the encoder tokens themselves (absorbed K / V projections)
  MHIP_K_ATTN_BIAS = 18,    // the biased instances of the MHIP_K_ATTN_FLASH kernels (attn_flash.hip): relative-position bias and key mask
  // VQ-NNF template matching (vqnnf.hip)
  MHIP_K_VQ_ASSIGN = 19,    // nearest code of every pixel's 27 colour features
  MHIP_K_VQ_KMEANS = 20,    // codebook update of one k-means iteration (the assignment is counted in MHIP_K_VQ_ASSIGN)
  MHIP_K_VQ_HEATMAP = 21,   // Gauss-Haar box filters over per-code integral images held in LDS, and the sum of the filters
  MHIP_K_VQ_PEAKS = 22,     // arg-max and suppression per (window, template)
  MHIP_K_CLIP_COSINE = 23,  // cosine similarity of the colour features of clip pairs
  // CLIP vision tower (clip_ops.hip)
  MHIP_K_CLIPVIS_PATCHIFY = 24,  // u8 clips -> per-channel normalised patch rows
  MHIP_K_CLIPVIS_EMBED = 25,     // class / patch + position rows -> pre_layrnorm -> fp32 stream; the LayerNorms of the layers;
                                 // also cliprn_tokens: (mean row | map) + positions of the attention pool
  MHIP_K_QUICK_GELU = 26,        // x * sigmoid(1.702 x) in place
  MHIP_K_CLIPVIS_HEAD = 27,      // post_layernorm of the class row + projection; also cliprn_cproj (the attention pool's c_proj)
  MHIP_K_PAIR_COSINE = 28,       // cosine of embedding pairs by index
  // CLIP text tower (cliptext_ops.hip; the attention: attn_seq.hip)
  MHIP_K_CLIPTEXT_EMBED = 29,    // token table gather + position rows -> fp32 stream
  MHIP_K_ATTN_CAUSAL = 30,       // causal soft-max attention, one workgroup per (sequence, head), K / V^T held in LDS
  MHIP_K_LEV_NGRAMS = 31,      // edit distance of every (template text, page n-gram) pair (lev_ngrams.hip)
  // BERT sentence encoders (berttext_ops.hip; the attention: attn_seq.hip)
  MHIP_K_ATTN_SHORT = 32,        // bidirectional soft-max attention over sequences of their own length, optional ALiBi, head dim 64 / 32:
                                 // attn_short (<= 128 rows, keys held in LDS) and attn_long (<= 8192 rows, keys streamed in blocks of
                                 // 128, online soft-max) share the slot, as the post-LayerNorms share berttext_embed
  MHIP_K_BERTTEXT_EMBED = 33,    // word + type + position rows -> LayerNorm -> fp32 stream; the post-LayerNorms of the layers
                                 // (LayoutReader's row LayerNorms are counted here too)
  MHIP_K_GEGLU = 34,             // gelu(x[:, :F]) * x[:, F:]
  MHIP_K_BERTTEXT_POOL = 35,     // masked mean / cls pooling, optional L2 normalisation
  MHIP_K_COUNT = 36
};

constexpr int MHIP_ZERO_BYTES = 65536;

struct ProfSlot {
  double total_ms = 0.0;
  int64_t launches = 0;
  double flops = 0.0;     // algorithmic FLOPs of the launches timed so far (MFMA kernels only)
  int parent = -1;        // slot that also accumulates this one's time / launches / flops
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

struct mhip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // workspace (grown on demand, never inside a steady-state forward)
  void* ws = nullptr;
  size_t ws_bytes = 0;
  void* zeros = nullptr;  // MHIP_ZERO_BYTES of zeros: source of padding taps / rows beyond M, N for LDS-DMA loads
  bool profiling = false;
  ProfSlot prof[MHIP_K_COUNT];
  std::vector<hipEvent_t> event_pool;
  // pinned staging for small host temporaries that must reach the device without draining the stream (descriptor tables of a
  // call): a ring of buffers, each guarded by the event of the copy that last read it (mhip_stage_h2d)
  struct PinnedRing {
    static constexpr int N = 4;
    void* buf[N] = {nullptr, nullptr, nullptr, nullptr};
    size_t cap[N] = {0, 0, 0, 0};
    hipEvent_t ev[N] = {nullptr, nullptr, nullptr, nullptr};
    int next = 0;
  } stage;
};
// dst_dev <- src_host (bytes) on ctx->stream through pinned memory; src_host may die when the call returns, the stream is not drained
int mhip_stage_h2d(mhip_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);

int mhip_fail(mhip_ctx* ctx, int code, const char* fmt, ...);
// Teardown: wait for the device, not for ctx->stream — the caller's stream (a torch stream handed in by mhip_set_stream) may
// already be gone when an object is destroyed late (interpreter shutdown), and synchronising a dead handle aborts the process
inline void mhip_quiesce(const mhip_ctx* ctx) {
  if (ctx) (void)hipSetDevice(ctx->device);      // the device this object lives on, not whatever the calling thread last used
  (void)hipDeviceSynchronize();
}
int mhip_ensure_workspace(mhip_ctx* ctx, size_t bytes);

// Bump allocator that lays out one call's buffers: every take starts at a multiple of `align`.  With a null base it only
// counts: take() returns nullptr and `off` ends as the bytes the same takes need on a real base.
struct Carver {
  char* base;
  size_t align;
  size_t off = 0;
  explicit Carver(void* b, size_t a = 256) : base((char*)b), align(a) {}
  template <typename P = char>
  P* take(size_t bytes) {
    const size_t at = off;
    off = (off + bytes + align - 1) / align * align;
    return base ? (P*)(base + at) : nullptr;
  }
  // a nested layout with its own alignment, starting here; the caller then takes sub.off bytes
  Carver sub(size_t a) const { return Carver(base ? base + off : nullptr, a); }
};

// bytes of the layout `layout(Carver&)` carves
template <typename F>
size_t mhip_layout_bytes(F&& layout, size_t align = 256) {
  Carver c(nullptr, align);
  layout(c);
  return c.off;
}
// The one way a call gets its workspace: `layout` runs on a sizing Carver, the workspace grows to that size, and `layout` runs
// again on ctx->ws to place the buffers.  Called once per exported entry, before its first launch: a nested ensure could move
// the workspace under pointers the caller holds.
template <typename F>
int mhip_carve_workspace(mhip_ctx* ctx, F&& layout, size_t align = 256) {
  const size_t need = mhip_layout_bytes(layout, align);
  int rc = mhip_ensure_workspace(ctx, need);
  if (rc) return rc;
  Carver ws(ctx->ws, align);
  layout(ws);
  if (ws.off != need) return mhip_fail(ctx, MHIP_ESTATE, "workspace layout carved %zu bytes, sized %zu", ws.off, need);
  return MHIP_OK;
}
extern "C" int mhip_gate_signal(mhip_gate* g, mhip_ctx* ctx);   // phase_gate.hip
void mhip_prof_begin(mhip_ctx* ctx, int kid, hipEvent_t* e0);
void mhip_prof_end(mhip_ctx* ctx, int kid, hipEvent_t e0);

#define MHIP_HIP(ctx, call)                                                              \
  do {                                                                                   \
    hipError_t _e = (call);                                                              \
    if (_e != hipSuccess)                                                                \
      return mhip_fail((ctx), MHIP_EHIP, "%s failed: %s (%s:%d)", #call,                 \
                       hipGetErrorString(_e), __FILE__, __LINE__);                       \
  } while (0)

// RAII-less launch bracket: PROF_LAUNCH(ctx, kid, kernel<<<...>>>(...));
#define PROF_LAUNCH(ctx, kid, ...)                    \
  do {                                                \
    hipEvent_t _e0 = nullptr;                         \
    if ((ctx)->profiling) mhip_prof_begin((ctx), (kid), &_e0); \
    __VA_ARGS__;                                      \
    if ((ctx)->profiling) mhip_prof_end((ctx), (kid), _e0);    \
  } while (0)

// after the launch(es) of a launcher: CHECK_LAUNCH(ctx, "name");
#define CHECK_LAUNCH(ctx, what)                                                                              \
  do {                                                                                                       \
    hipError_t _e = hipGetLastError();                                                                       \
    if (_e != hipSuccess) return mhip_fail((ctx), MHIP_EHIP, what " launch: %s", hipGetErrorString(_e));    \
  } while (0)

// Grow-only device buffer owned by a model handle (staging that must not hipMalloc in steady state).
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  template <typename T = char>
  T* as() const { return (T*)p; }
  // at least `need` bytes: growing drains ctx->stream first (work in flight may read the old allocation); the size is recorded
  // only once the new allocation stands
  int ensure(mhip_ctx* ctx, size_t need) {
    if (need <= bytes) return MHIP_OK;
    MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    release();
    MHIP_HIP(ctx, hipMalloc(&p, need));
    bytes = need;
    return MHIP_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// The host entries' upload: fn(dev) on a temporary device copy of `bytes` of host memory (`what` names it in the failure
// message); ctx->stream is drained and the copy freed on every path.
template <typename F>
int mhip_with_upload(mhip_ctx* ctx, const void* host, size_t bytes, const char* what, F&& fn) {
  uint8_t* dev = nullptr;
  hipError_t e = hipMalloc((void**)&dev, bytes);
  if (e == hipSuccess) e = hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice);
  const int rc = e == hipSuccess ? fn((const uint8_t*)dev) : mhip_fail(ctx, MHIP_EHIP, "%s upload (%zu bytes): %s", what, bytes, hipGetErrorString(e));
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(dev);
  return rc;
}

// workgroups of `block` threads a grid-stride kernel over `total` items is launched with
inline int grid_for(long long total, int block) {
  const long long g = (total + block - 1) / block;
  return (int)(g < 65535LL * 4 ? g : 65535LL * 4);
}
// the grid of the image kernels of the recognizer and the detector (icr_ops.hip, image_ops.hip): blocks of 256, 1 .. 8192 of
// them (its own name: another clamp than grid_for's)
inline unsigned image_grid_for(long long total) {
  const long long g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 256 * 32 ? 256 * 32 : g));
}

// ------------------------------------------------------------------ row LayerNorm (row_ops.hip; the arithmetic: row_ops.h)
// h fp32 (null: not written) = LN(x), ht (null: not written) its copy in the precision's element type; one of the two at least.
// x: the residual stream, fp32 — or f16 (x_f16, f16 mode only), x_lo then being the low plane when the stream is kept as two f16
// planes (x = hi + lo; ConvDesc::epi) or null.  D % 64 == 0, D <= 1024.  h may be x (a wave holds its row in registers before it
// writes).  slot: the MhipKernelId the launch is counted in (the caller's tower's)
int mhip_launch_row_layernorm(mhip_ctx* ctx, int slot, int precision, const void* x, int x_f16, const void* x_lo, const float* g,
                              const float* b, float* h, void* ht, int rows, int D, float eps);

// ------------------------------------------------------------------ conv / GEMM launcher
// Implicit-GEMM convolution over NHWC activations:  out[m][n] = act( scale[n] * sum_k A[m][k] W[n][k] + bias[n] )
// with A[m][k] = in[b][y+dy-pad][x+dx-pad][c], k = (dy*KW+dx)*Cin + c, and an optional max-pool
// folded into the epilogue (rows are enumerated so that a pooling window is 4 / 2 consecutive m).
enum PoolMode { POOL_NONE = 0, POOL_2x2 = 1, POOL_2x1 = 2 };
enum ActMode { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2 };   // values of ConvDesc::relu

struct ConvDesc {
  const void* in = nullptr;     // [B][H][W][Cin]  element type T
  const void* w = nullptr;      // [N][KH*KW*Cin]  element type T (K contiguous)
  const float* scale = nullptr; // [N] or nullptr (= 1)
  const float* bias = nullptr;  // [N] or nullptr (= 0)
  void* out = nullptr;          // [B][Hp][Wp][N]  T, or fp32 if out_f32
  int B = 0, H = 0, W = 0, Cin = 0;
  int KH = 1, KW = 1, pad = 0;
  int N = 0;
  int pool = POOL_NONE;
  int relu = 0;                 // ActMode
  int out_f32 = 0;
  int sy = 1;                   // vertical stride (horizontal stride is 1)
  int pad_x = -1;               // horizontal padding; -1 = same as `pad`
  const void* res = nullptr;    // residual (same shape/type as out: fp32 when out_f32), added before the ReLU; unpooled only
  int ldc = 0;                  // output row pitch in elements; 0 = N
  int pad_cols_writable = 0;    // 1: with a pitch >= roundup(N, 8) the columns [N, roundup(N, 8)) of every output row belong to this
                                //    call and may be overwritten (with zeros): lets a ragged N take the 16-byte store path
  int row_period = 0;           // > 0 (unpooled GEMMs): output row = (q / period) * row_stride + row_offset + q % period,
  int row_stride = 0;           //      residual row = q % period (see igemm_common.h)
  int row_offset = 0;
  int dil = 1;                  // filter dilation
  const void* in2 = nullptr;    // optional second input: channels [Cin1, Cin) of a 1x1 conv over cat(in, in2)
  int Cin1 = 0;
  // ---- LayerNorm folded around a plain f16 GEMM (the ViT encoder blocks, vit_api.hip) ----
  // The residual stream x is kept as two f16 planes, x = hi + lo (hi = f16(x), lo = f16(x - hi): ~22 significant bits in the
  // bytes of one fp32).  hi IS the GEMM operand of the next product: LN(x) W^T = rstd (hi (g*W)^T - mean colsum(g*W)) + W b
  // up to the rounding of x, so no normalised copy of the stream is ever written.
  //   EPI_SPLIT    (producer: proj / fc2 / patch embedding) out = hi plane, out2 = lo plane, res / res2 the residual's planes;
  //                `stats` receives (sum, centred sum of squares) of every output row per 64-column chunk
  //   EPI_LN_ROWS  (consumer, tokens are GEMM rows: q|k, fc1)  out = act(rstd[m] acc - (mean rstd)[m] cs[n] + bias[n])
  //   EPI_LN_COLS  (consumer, tokens are GEMM columns: V^T = W_v X^T)  out = rstd[n] acc - (mean rstd)[n] cs[m] + row_bias[m]
  int epi = 0;
  const float* ln_a = nullptr;
  const float* ln_b = nullptr;
  const float* ln_cs = nullptr;
  const float* row_bias = nullptr;
  void* out2 = nullptr;
  const void* res2 = nullptr;
  float* stats = nullptr;
  int stats_ld = 0;
};
enum { EPI_NONE = 0, EPI_LN_ROWS = 1, EPI_LN_COLS = 2, EPI_SPLIT = 3 };
// precision: MHIP_PREC_F16 / MHIP_PREC_F32.  Returns 0 or negative error.
int mhip_launch_conv_igemm(mhip_ctx* ctx, int precision, const ConvDesc& d);
// the plain GEMM of it:  out [M][N] = act(scale[n] * in [M][K] w [N][K]^T + bias[n] (+ res))
inline int mhip_gemm(mhip_ctx* ctx, int prec, const void* in, const void* w, long long M, int N, int K, const float* scale,
                     const float* bias, void* out, int act, int out_f32, const void* res = nullptr, int ldc = 0,
                     int pad_cols_writable = 0) {
  ConvDesc c;
  c.in = in; c.w = w; c.scale = scale; c.bias = bias; c.out = out;
  c.B = 1; c.H = 1; c.W = (int)M; c.Cin = K; c.N = N;
  c.relu = act; c.out_f32 = out_f32; c.res = res; c.ldc = ldc; c.pad_cols_writable = pad_cols_writable;
  return mhip_launch_conv_igemm(ctx, prec, c);
}
double mhip_conv_flops(const ConvDesc& d);

// first layer: u8 [B][H][W] -> normalise -> conv3x3 pad1 (1->64) + bias + ReLU + maxpool 2x2 -> [B][H/2][W/2][64] T
int mhip_launch_conv_first(mhip_ctx* ctx, int precision, const uint8_t* crops, const float* w9x64,
                           const float* bias64, void* out, int B, int H, int W);

// BiLSTM recurrence.  xproj fp32 [B][T][2][1024] with each direction's 1024 columns ordered
// [wave][u][unit16][gate] (see mhip_lstm_xproj_row; input projection incl. both biases),
// wpack = W_hh of both directions in MFMA fragment order, hseq out [B][T][512] T.
int mhip_launch_lstm_rec(mhip_ctx* ctx, int precision, const float* xproj, const void* wpack, void* hseq,
                         int B, int T);
size_t mhip_lstm_wpack_bytes(int precision);
// PyTorch gate-matrix row that lands in (per-direction) xproj column `col` (gate-interleaved layout)
int mhip_lstm_xproj_row(int col);
// host-side packing of W_hh (fwd, bwd: [1024][256] fp32, gate order i,f,g,o) into fragment order
void mhip_lstm_pack_whh(int precision, const float* whh_fwd, const float* whh_bwd, void* dst);
// host-side packing of one bidirectional BidirectionalLSTM block (`prefix` "SequenceModeling.<j>."; CRNN and ICR):
// W_ih rows permuted to the xproj column order at `precision` [2][1024][in], b_ih + b_hh fp32 [2][1024], W_hh via
// mhip_lstm_pack_whh, and the linear layer ([256][512] at `precision`, bias fp32 [256])
struct TensorStore;
int mhip_lstm_pack_bilstm(mhip_ctx* ctx, const TensorStore& st, const std::string& prefix, int in, int precision,
                          char* ih_w, float* ih_b, char* hh_pack, char* lin_w, float* lin_b);

// greedy CTC decode
int mhip_launch_ctc_decode(mhip_ctx* ctx, const float* logits, int n, int T, int C, int32_t* argmax,
                           int32_t* tokens, int32_t* lengths, float* conf);

// ------------------------------------------------------------------ detector image ops (image_ops.hip)
void mhip_resize_linear_tables(int src, int dst, std::vector<int>& ofs, std::vector<short>& coef);
int mhip_launch_resize_linear_u8(mhip_ctx* ctx, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw,
                                 const int* xofs, const short* xa, const int* yofs, const short* yb);
int mhip_launch_conv_rgb_first(mhip_ctx* ctx, int precision, const uint8_t* img, int th, int tw, int H, int W,
                               const float* w27x64, const float* scale, const float* bias, void* out);
int mhip_launch_maxpool(mhip_ctx* ctx, int precision, int k, const void* in, void* out, int B, int H, int W, int C);
int mhip_launch_score_head(mhip_ctx* ctx, int precision, const void* in, int in_stride, const float* w1,
                           const float* b1, const float* w2, const float* b2, float* scores, long long npix);
int mhip_launch_upsample_bilinear(mhip_ctx* ctx, int precision, const void* in, void* out, int B, int Hi, int Wi,
                                  int C, int Ho, int Wo);

// ------------------------------------------------------------------ score-map post-processing (ccl.hip)
// scores fp32 [H][W][2] (text, link) -> flags u8 (bit0 text > low_text, bit1 link > link_thr), labels int32
// (0 = background, components numbered in raster order of their first pixel), n_labels (incl. background) and
// per-component stats int32 [n][6] = {left, top, right, bottom, area, max text score as ordered int bits}.
struct CclBuffers {
  uint8_t* flags;   // [H*W]
  int* parent;      // [H*W]  union-find forest, then root index per pixel
  int* labels;      // [H*W]
  int* blocksum;    // [ceil(H*W/2048) + 1]
  int* stats;       // [max_labels][6]
  int* n_labels;    // [1]
};
void mhip_ccl_carve(Carver& ws, int H, int W, CclBuffers* out);
int mhip_launch_ccl(mhip_ctx* ctx, const float* scores, int H, int W, float low_text, float link_thr,
                    const CclBuffers& b);
float mhip_ordered_bits_to_float(int bits);

// ------------------------------------------------------------------ crop batcher (crop_batch.hip)
int mhip_crop_resized_width(int w, int h, int img_h, int img_w);
size_t mhip_crop_scratch_bytes(const mhip_crop_desc* descs, int n, int img_h, int img_w);
int mhip_launch_crop_batch(mhip_ctx* ctx, const uint8_t* base_dev, const mhip_crop_desc* descs, int n, int img_h,
                           int img_w, void* scratch_dev, uint8_t* out_dev);

// ------------------------------------------------------------------ production ICR recognizer ops (icr_ops.hip)
int mhip_launch_conv_gray_first(mhip_ctx* ctx, int precision, int in_is_u8, const void* img, int B, int H, int W,
                                int C, const float* w9xC, const float* scale, const float* bias, void* out);
int mhip_launch_maxpool_s21_p01(mhip_ctx* ctx, int precision, const void* in, void* out, int B, int H, int W, int C);
int mhip_launch_avgpool_hw(mhip_ctx* ctx, int precision, const void* in, void* out, int B, int HW, int C);
int mhip_launch_tps_sample(mhip_ctx* ctx, const uint8_t* crops, const float* cprime, const float* inv_delta_c,
                           const float* p_hat, float* out, int B, int H, int W, int F);
int mhip_launch_attn_context(mhip_ctx* ctx, int precision, const float* hproj, const float* hp, int ld_hp,
                             const float* score_w, const void* H, void* ctx_out, int B, int Tn);
int mhip_launch_attn_cell(mhip_ctx* ctx, int precision, const float* gctx, const float* ghid, int ld_hp,
                          const float* w_onehot, const int* chars, float* c, void* h, int B);
int mhip_launch_argmax_rows(mhip_ctx* ctx, const float* logits, int ld, int C, int* idx, int B);
int mhip_launch_rowmax_softmax(mhip_ctx* ctx, const float* logits, int rows, int C, int* idx, float* pmax);

// ------------------------------------------------------------------ ViT encoder ops (vit_ops.hip)
// the split stream (two f16 planes + row statistics per 64-column chunk, stats[(chunk * stats_ld + row) * 2]):
int mhip_launch_token_init_split(mhip_ctx* ctx, void* hi, void* lo, const float* cls_row, const float* cls_stats, float* stats,
                                 int stats_ld, int B, int npad, int n_tok, int D);
int mhip_launch_ln_finalize(mhip_ctx* ctx, const float* stats, int chunks, int ld, float* rstd, float* mur, int rows, int D, float eps);
int mhip_launch_split_f16(mhip_ctx* ctx, const float* in, void* hi, void* lo, long long n);
int mhip_launch_join_f16(mhip_ctx* ctx, const void* hi, const void* lo, float* out, long long n);
// (attn_flash.hip) softmax(Q K^T) V for `images` x `heads` independent (head_dim 64) problems; q is pre-scaled by head_dim^-0.5 * log2(e).
// The last 128-query block / 64-key tile of an image may read up to 127 rows past it (and masks them): q and k — and the codes
// of AttnBiasDesc — need ATTN_SLACK_ROWS finite rows past the last image, vt 64 finite elements (carved as ATTN_SLACK_ROWS).
// The same holds inside an image: its padding rows n_keys .. npad_k - 1 of k and their V^T columns are read and take a
// probability of exactly 0, so they must be finite (0 x NaN would reach the output), whatever else they hold; a code that is
// read — padding and slack rows included — must index inside its table (p <= 2 dp + 1, x and y <= dx).  Output rows n_queries ..
// npad_q - 1 inside a launched 128-query block are written (with the results of the padding queries); nothing else is.
constexpr int ATTN_SLACK_ROWS = 128;
struct AttnDesc {
  const void* q = nullptr;    // [images*npad_q][ldq] T, head h at column h*64
  const void* k = nullptr;    // [images*npad_k][ldk] T
  const void* vt = nullptr;   // [heads*64][ldv] T: V transposed, column = image*npad_k + key
  void* out = nullptr;        // [images*npad_q][ldo] T
  int ldq = 0, ldk = 0, ldv = 0, ldo = 0;
  int images = 0, heads = 0;
  int npad_q = 0, npad_k = 0;  // rows per image (npad_k % 8 == 0)
  int n_queries = 0, n_keys = 0;
};
int mhip_launch_attention(mhip_ctx* ctx, int precision, const AttnDesc& d);
double mhip_attention_flops(const AttnDesc& d);
int mhip_launch_patchify(mhip_ctx* ctx, int precision, const uint8_t* imgs, int B, int th, int tw, int hp, int wp, int P,
                         int swap_rb, float mean, float stdv, void* out, int ld);
int mhip_launch_token_init(mhip_ctx* ctx, void* x, const float* cls_row, int B, int npad, int n_tok, int D, int x_f16 = 0);
int mhip_launch_tokens_to_map(mhip_ctx* ctx, int precision, const void* x, void* out, int B, int npad, int np, int D, int x_f16 = 0);
int mhip_launch_posemb_bicubic(mhip_ctx* ctx, const float* tab, int gh, int gw, float* out, int hp, int wp, int D);
int mhip_launch_convert_rows(mhip_ctx* ctx, int precision, const void* in, float* out, int rows, int D);
int mhip_launch_narrow_f16(mhip_ctx* ctx, const float* in, void* out, long long n);
int mhip_launch_unnest(mhip_ctx* ctx, int precision, const void* in, const void* coarse, void* out, int out_f32, int B,
                       int H, int W, int C, int nest);

// ------------------------------------------------------------------ Pillow-exact resize (pil_resize.hip)
bool mhip_pil_filter_ok(int filter);      // MHIP_PIL_LANCZOS / _BILINEAR / _BICUBIC
size_t mhip_pil_resize_scratch_bytes(int sh, int sw, int dh, int dw, int filter);
int mhip_launch_pil_resize_rgb(mhip_ctx* ctx, const uint8_t* src, int sh, int sw, size_t src_stride, uint8_t* dst, int dh,
                               int dw, int filter, void* scratch);

// ------------------------------------------------------------------ detector heads (det_ops.hip)
void mhip_rpn_cell_anchors(const float sizes[5], const float ratios[3], float out[5][3][4]);
struct RpnDesc {
  const float* head[5];       // per level fp32 [images][H*W][16]: 3 objectness logits, 3 x 4 deltas, 1 pad
  int H[5], W[5], stride[5];
  float cell[5][3][4];
  int images = 1;
  int img_h = 0, img_w = 0;   // resized image size (proposal clip)
  float nms_thr = 0.7f;
  int post_topk = 1000;       // <= 1000
  float* lvl_boxes = nullptr;   // scratch [images][5][1000][4]
  float* lvl_scores = nullptr;  // scratch [images][5][1000]
  int* lvl_counts = nullptr;    // scratch [images][5]
  float* out_boxes = nullptr;   // [images][post_topk][4]
  float* out_scores = nullptr;  // [images][post_topk]
  int* out_counts = nullptr;    // [images]
};
int mhip_launch_rpn_proposals(mhip_ctx* ctx, const RpnDesc& d);
struct RoiDesc {
  const void* feat[4];   // p2..p5 NHWC T [images][H][W][C]
  int H[4], W[4];
  float scale[4];
  const float* rois = nullptr;   // [images][max_rois][4]
  const int* counts = nullptr;
  int images = 1, max_rois = 1000, C = 256;
  void* out = nullptr;           // [images][max_rois][49*C] T
};
int mhip_launch_roi_align(mhip_ctx* ctx, int precision, const RoiDesc& d);
struct DetFinalDesc {
  const float* head = nullptr;   // [images][max_rois][8]
  const float* rois = nullptr;
  const int* counts = nullptr;
  int images = 1, max_rois = 1000;
  int img_h = 0, img_w = 0, out_h = 0, out_w = 0;
  float score_thr = 0.05f, nms_thr = 0.5f;
  int max_det = 2000;
  float* out_boxes = nullptr;    // [images][max_rois][4]
  float* out_scores = nullptr;   // [images][max_rois]
  int* out_count = nullptr;      // [images]
};
int mhip_launch_det_final(mhip_ctx* ctx, const DetFinalDesc& d);
// the K-class final stage (K = num_classes > 1): head [images][max_rois][ld] = K + 1 logits (background last), 4K deltas
constexpr int DET_MAX_CLASSES = 16;
struct DetFinalMultiDesc {
  const float* head = nullptr;
  int ld = 0, num_classes = 2;
  const float* rois = nullptr;
  const int* counts = nullptr;
  int images = 1, max_rois = 1000;
  int img_h = 0, img_w = 0, out_h = 0, out_w = 0;
  float score_thr = 0.05f, nms_thr = 0.5f;
  int max_det = 100;             // <= 1000
  unsigned long long* cls_keys = nullptr;   // scratch [images][K][1000]
  float* cls_boxes = nullptr;               // scratch [images][K][1000][4]
  int* cls_counts = nullptr;                // scratch [images][K]
  float* out_boxes = nullptr;    // [images][max_rois][4]
  float* out_scores = nullptr;   // [images][max_rois]
  int* out_classes = nullptr;    // [images][max_rois]
  int* out_count = nullptr;      // [images]
};
int mhip_launch_det_final_multi(mhip_ctx* ctx, const DetFinalMultiDesc& d);
int mhip_launch_blackout(mhip_ctx* ctx, uint8_t* page, int H, int W, const int* boxes_dev, int n, int* changed_dev);
int mhip_launch_subsample2(mhip_ctx* ctx, int precision, const void* in, void* out, int B, int H, int W, int C);

// ------------------------------------------------------------------ TrOCR decoder steps (trocr_ops.hip)
// y_f32 (may be x) = LN(x), y_t its copy in the precision's element type; D % 256 == 0.  The post-LayerNorm of the TrOCR decoder and
// of the LayoutLMv3 layers: not mhip_launch_row_layernorm, whose variance rounds differently in a row's first group (DESIGN.md §3,
// "The row kernels of the towers")
int mhip_launch_layernorm2(mhip_ctx* ctx, int precision, const float* x, const float* g, const float* b, float* y_f32,
                           void* y_t, int rows, int D, float eps);
int mhip_launch_embed_step(mhip_ctx* ctx, int precision, const int* tokens, const void* emb, const float* pos_row, float scale,
                           const float* g, const float* b, float* x, void* xt, int rows, int D, float eps);
constexpr int DEC_ATTN_MAX_KEYS = 640;   // longest history / encoder sequence decode attention runs (its (4, 640) instantiation)
struct DecAttnDesc {
  const void* q = nullptr;   // [groups*nq][ldq] T, pre-scaled
  const void* k = nullptr;
  const void* v = nullptr;
  void* out = nullptr;       // [groups*nq][ldo] T
  const int* anc = nullptr;  // self-attention: [rows][anc_ld] cache slot per past step (k/v laid out [step][slots][ldk])
  int anc_ld = 0, slots = 0;
  int kv_rows = 0;           // cross-attention: k/v rows per group
  int ldq = 0, ldk = 0, ldo = 0;
  int heads = 0, groups = 0, nq = 1, n_keys = 0;
  int force_generic = 0;     // skip the f16 short-history self-attention kernel (what MARIE_HIP_GENERIC_SELF_ATTN does per process)
};
int mhip_launch_decode_attention(mhip_ctx* ctx, int precision, const DecAttnDesc& d);
// Encoder-attention of one decoder layer with the key / value projections absorbed (cross_attn.hip; f16 only):
// q [crops*beam][ldq] (pre-scaled) -> qt = W_k,h^T q_h -> attention over E -> ct -> ao = W_v,h ct_h + b_v.
struct CrossAbsorbDesc {
  const void* q = nullptr;     // [crops*beam][ldq] f16
  int ldq = 0;
  const void* E = nullptr;     // [crops][kv_rows][enc_dim] f16 encoder tokens
  int kv_rows = 0, n_keys = 0, enc_dim = 0;
  const void* wkt = nullptr;   // [heads][enc_dim][64] f16: W_k[h*64 + j][d] * log2(e) at [h][d][j]
  const void* wv = nullptr;    // [heads*64][enc_dim] f16 (the checkpoint's layout)
  const float* bv = nullptr;   // [heads*64]
  void* qt = nullptr;          // scratch [crops*beam][16][enc_dim] f16
  void* ct = nullptr;          // scratch [crops*beam][16][enc_dim] f16
  void* ao = nullptr;          // [crops*beam][ldo] f16
  int ldo = 0;
  int crops = 0, beam = 1, heads = 0;
};
// finite rows E needs behind its last crop: the kernel walks a crop's keys in tiles of up to 32 rows (TK, cross_attn.hip) and reads,
// masked, past n_keys; two tiles' worth
constexpr int CROSS_ATTN_SLACK_ROWS = 64;
bool mhip_cross_absorb_supported(int enc_dim, int beam, int heads);
int mhip_launch_cross_absorbed(mhip_ctx* ctx, const CrossAbsorbDesc& d);
struct BeamCandDesc {
  const void* logits = nullptr;    // [bsz*beam][ld], fp32 or f16
  int logits_f16 = 0;
  int ld = 0, vocab = 0, beam = 1, bsz = 0;
  const float* cum = nullptr;      // [bsz*beam]
  int step = 0, max_len = 0, min_len = 1, pad = 1, eos = 2;
  float* cand_scores = nullptr;    // [bsz][2*beam]
  int* cand_tokens = nullptr;
  int* cand_beams = nullptr;
};
int mhip_launch_beam_candidates(mhip_ctx* ctx, const BeamCandDesc& d);
int mhip_launch_ancestry(mhip_ctx* ctx, const int* anc_old, int* anc_new, const int* parent, int rows, int ld, int step);
// Generator bookkeeping of one beam-search step on the device (TextRecognitionGenerator._generate, generator.py:208-362:
// finalize_hypos over the eos candidates among the first `beam`, the `beam` best live candidates become the next rows).
// One thread per crop; finished crops keep their rows (no batch compaction).  All arrays live in HBM.
struct BeamState {
  int bsz = 0, beam = 1, max_len = 0, pad = 1, eos = 2;
  const float* cand_scores = nullptr;   // [bsz][2*beam] (mhip_launch_beam_candidates)
  const int* cand_tokens = nullptr;
  const int* cand_beams = nullptr;
  int* tokens[2] = {nullptr, nullptr};  // [bsz*beam][max_len + 2] hypothesis tokens incl. the leading eos; read [cur], written [cur^1]
  int* last_tok = nullptr;              // [bsz*beam] token every row feeds to the next step
  int* parent = nullptr;                // [bsz*beam] row of the previous step a row continues
  float* cum = nullptr;                 // [bsz*beam] cumulative log-probability of a row
  unsigned char* ignore = nullptr;      // [bsz*beam] cands_to_ignore
  unsigned char* finished = nullptr;    // [bsz]
  int* fin_count = nullptr;             // [bsz] finalized hypotheses so far
  int* fin_tokens = nullptr;            // [bsz][beam][max_len + 1]
  int* fin_len = nullptr;               // [bsz][beam]
  float* fin_score = nullptr;           // [bsz][beam] normalised scores, in finalisation order
  int* remaining = nullptr;             // [1] crops not finished yet
};
// the state's arrays from `ws` (beam <= 4: the generator's limit, checked when the model is created)
void mhip_beam_state_carve(Carver& ws, int bsz, int beam, int max_len, int pad, int eos, BeamState* st);
int mhip_launch_beam_init(mhip_ctx* ctx, const BeamState& st, int* anc0, int anc_ld);
int mhip_launch_beam_select(mhip_ctx* ctx, const BeamState& st, int cur, int step);
// best hypothesis per crop -> tokens_out [bsz][max_len + 1] (padded), lengths_out [bsz], scores_out [bsz] (device arrays)
int mhip_launch_beam_best(mhip_ctx* ctx, const BeamState& st, int* tokens_out, int* lengths_out, float* scores_out);
// ------------------------------------------------------------------ LayoutLMv3 ops (layoutlmv3_ops.hip)
// Attention with a learned relative-position bias and a key mask (attn_flash.hip).  Every token carries a code p | x << 12 | y << 22 (p: 1-d
// position, x: x0, y: y1 of its box); a score takes tab[h][kp + dp - qp] + tab[h][off_x + kx + dx - qx] + tab[h][off_y + ky + dx - qy]
// (already scaled as the pre-scaled q is).  A masked key carries p = 2 dp + 1 in kcode: entries [2 dp + 1, 3 dp + 1] of the 1-d
// table hold MHIP_ATTN_MASKED, so the mask costs no instruction of its own.
constexpr float MHIP_ATTN_MASKED = -1024.f;    // log2 units: exp2 of it is 0 in fp32 beside any score a LayerNormed model produces
struct AttnBiasDesc {
  AttnDesc a;
  const uint32_t* qcode = nullptr;   // [images*npad_q + ATTN_SLACK_ROWS]
  const uint32_t* kcode = nullptr;   // [images*npad_k + ATTN_SLACK_ROWS]
  const float* tab = nullptr;        // [heads][mhip_attn_bias_table_len(dp, dx)] fp32
  int dp = 0, dx = 0;                // largest |p_j - p_i| (<= 1023) and |x_j - x_i|, |y_j - y_i| (<= 1023)
};
inline int mhip_attn_bias_table_len(int dp, int dx) { return 3 * dp + 2 + 2 * (2 * dx + 1); }
int mhip_launch_attention_bias(mhip_ctx* ctx, int precision, const AttnBiasDesc& d);
// tab[h] from the three head-major bias matrices (w1 [heads][bins_1d], wx / wy [heads][bins_2d]), scaled by `scale`
void mhip_attn_bias_fold(const float* w1, const float* wx, const float* wy, int heads, int bins_1d, int max_1d, int bins_2d,
                         int max_2d, int dp, int dx, float scale, float* tab);
int mhip_relative_position_bucket(int relative_position, int num_buckets, int max_distance);
struct Lmv3EmbedDesc {
  const int* tok = nullptr;          // [pages*max_text][8]: id, position id, x0, y0, x1, y1, h, w (clipped)
  const int* win_page = nullptr;     // [pages]: the page image whose patch rows a window of text takes (identity: one window a page)
  const void* word = nullptr;        // [vocab][D] T
  const float *type0 = nullptr, *pos = nullptr, *xe = nullptr, *ye = nullptr, *he = nullptr, *we = nullptr;
  const float *g_text = nullptr, *b_text = nullptr;      // embeddings.LayerNorm
  const float* patches = nullptr;    // [page images*(n_vis - 1)][D] fp32: patch projection + bias + position rows 1..
  const float* cls = nullptr;        // [D]: cls_token + position row 0
  const float *g_vis = nullptr, *b_vis = nullptr;        // norm (eps_vis)
  const float *g_all = nullptr, *b_all = nullptr;        // LayoutLMv3Model.LayerNorm
  float* h = nullptr;                // [pages*npad][D] fp32
  void* ht = nullptr;                // the same rows as T
  int pages = 0, max_text = 0, n_vis = 0, npad = 0, D = 0, coord = 0, shape = 0;
  float eps = 1e-5f, eps_vis = 1e-6f;
};
int mhip_launch_lmv3_embed(mhip_ctx* ctx, int precision, const Lmv3EmbedDesc& d);
// logits[page] = out_proj(tanh(dense(h[page*npad]))), fp32 weights
int mhip_launch_lmv3_head(mhip_ctx* ctx, const float* h, int pages, int npad, int D, const float* dw, const float* db,
                          const float* ow, const float* ob, int labels, float* logits);
// The token-classification head and its decision: row r of `rows` is x[(r / seg) * seg_stride + r % seg] (seg text rows out of
// every seg_stride rows); logits = W_o f(x) + b_o with f = tanh (use_tanh: x is the dense product + bias) or the identity;
// label[r] = lowest index of the maximum, score[r] = its soft-max probability, logits[r][L] only when asked for.  All fp32.
struct TokenHeadDesc {
  const float* x = nullptr;          // [..][D]
  const float *w = nullptr, *b = nullptr;      // [L][D], [L]
  int* label = nullptr;              // [rows]
  float* score = nullptr;            // [rows]
  float* logits = nullptr;           // [rows][L] or nullptr
  int rows = 0, seg = 1, seg_stride = 1, D = 0, L = 0, use_tanh = 0;
};
int mhip_token_head_max_labels(int D);
int mhip_launch_token_head(mhip_ctx* ctx, const TokenHeadDesc& d);
// ------------------------------------------------------------------ CLIP vision tower ops (clip_ops.hip)
// Row kernels: D % 64 == 0, D <= 1024.  Token rows as the ViT's: npad rows an image, row 0 the class token.
// clips u8 [B][S][S][3] -> out [B * (S/P)^2][ld] T, column (c * P + y) * P + x = (pixel / 255 - mean[c]) / stdv[c]; P % 8 == 0
int mhip_launch_clipvis_patchify(mhip_ctx* ctx, int precision, const uint8_t* imgs, int B, int S, int P, int swap_rb,
                                 const float mean[3], const float stdv[3], void* out, int ld);
// h [B*npad][D] fp32 = LN(class + pos[0]) | LN(patches [B*(n_tok-1)][D] + pos[1..]) | zeros
int mhip_launch_clipvis_embed(mhip_ctx* ctx, const float* patches, const float* cls, const float* pos, const float* g, const float* b,
                              float* h, int B, int npad, int n_tok, int D, float eps);
// x [n] T in place; n a multiple of 16 bytes' worth of elements
int mhip_launch_quick_gelu(mhip_ctx* ctx, int precision, void* x, long long n);
// emb [B][E] fp32 = LN(h[img * npad + row_of[img]]) proj_t^T, proj_t [E][D] fp32; row_of (device, [B]) null: row 0 of every block
int mhip_launch_clipvis_head(mhip_ctx* ctx, const float* h, int B, int npad, int D, const float* g, const float* b, float eps,
                             const float* proj_t, int E, float* emb, const int* row_of = nullptr);
// out[p] = cos(emb[pair_a[p]], emb[pair_b[p]]), emb [..][E] fp32; the indices are the caller's to check
int mhip_launch_pair_cosine(mhip_ctx* ctx, const float* emb, int E, const int* pair_a, const int* pair_b, int n_pairs, float* out);
// ------------------------------------------------------------------ CLIP ModifiedResNet tower ops (cliprn_ops.hip)
// NHWC activations of the precision's element type.  clips u8 [B][S][S][3], S even -> out [B][S/2][S/2][Cp]: the 3 x 3, stride 2,
// pad 1 convolution of the normalised clip (zero outside it), out = relu(scale * acc + bias); w27 fp32 [(dy*3 + dx)*3 + c][Cp],
// Cp a multiple of 8 up to 64
int mhip_launch_cliprn_stem(mhip_ctx* ctx, int precision, const uint8_t* imgs, int B, int S, int swap_rb, const float mean[3],
                            const float stdv[3], const float* w27, const float* scale, const float* bias, void* out, int Cp);
// in [B][H][W][C] -> out [B][H/k][W/k][C]: the mean of every k x k window (k = 2; H, W multiples of k; C of 16 bytes' worth)
int mhip_launch_avgpool_nhwc(mhip_ctx* ctx, int precision, int k, const void* in, void* out, int B, int H, int W, int C);
// the attention pool's limits: HW + 1 <= 257 keys, E a multiple of 64 up to 4096
bool mhip_cliprn_attnpool_ok(int HW, int E, int P);
// x [B][HW][E] -> tok [B][HW + 1][E] = (mean row | x) + pos, xq [B][E] = the mean rows; pos fp32 [HW + 1][E]
int mhip_launch_cliprn_tokens(mhip_ctx* ctx, int precision, const void* x, const float* pos, void* tok, void* xq, int B, int HW, int E);
// ao fp32 [B][E] = soft-max(q_h . k_h) v_h per head of 64; q fp32 [B][E] pre-scaled, kv fp32 [B * NT][2 E] (k | v)
int mhip_launch_cliprn_attn1q(mhip_ctx* ctx, const float* q, const float* kv, float* ao, int B, int NT, int E);
// emb fp32 [B][P] = ao w^T + bias; w fp32 [P][E]
int mhip_launch_cliprn_cproj(mhip_ctx* ctx, const float* ao, int B, int E, const float* w, const float* bias, int P, float* emb);
// ------------------------------------------------------------------ CLIP text tower ops (cliptext_ops.hip)
// h [B*npad][D] fp32 = table[ids[row]] + pos[row % npad]; table [vocab][D], pos [>= npad][D] fp32; the ids are the caller's to check
int mhip_launch_cliptext_embed(mhip_ctx* ctx, const float* table, const float* pos, const int* ids, float* h, int B, int npad, int D);
// ------------------------------------------------------------------ per-sequence attention of the text towers (attn_seq.hip)
// causal softmax(Q K^T) V over AttnDesc's layout (query row t sees keys 0 .. t): npad_q == npad_k <= 128, a multiple of 8; every
// row < npad is written, nothing past a sequence's rows is read (no slack needed)
int mhip_launch_attention_causal(mhip_ctx* ctx, int precision, const AttnDesc& d);
// softmax(Q K^T [- slope |i - j|]) V over AttnDesc's layout with heads of head_dim (64 or 32) columns, sequence b attending to its
// first len[b] keys (device, 1 .. npad; n_queries / n_keys of `a` are not used): npad_q == npad_k <= 128, a multiple of 8; every
// row < npad is written, nothing past a sequence's rows is read (no slack needed).  slopes (device, [heads], in the log2 units of
// q) or null: no bias term.  rel_table (device, fp32 [heads][2 rel_radius + 1] in the same log2 units, finite) or null: with it the
// score of (query i, key j) gets rel_table[head][clamp(i - j, -rel_radius, rel_radius) + rel_radius] (MPNet's relative attention
// bias).  Slopes and a table together are MHIP_EINVAL
struct AttnShortDesc {
  AttnDesc a;
  const int* len = nullptr;
  const float* slopes = nullptr;
  int head_dim = 64;
  const float* rel_table = nullptr;
  int rel_radius = 0;
};
int mhip_launch_attention_short(mhip_ctx* ctx, int precision, const AttnShortDesc& d);
// the same attention with the keys streamed through LDS in blocks of 128 and an online soft-max: npad_q == npad_k, a multiple of 8,
// 8 .. 8192 (128 rows and fewer are taken too: one block through the streamed code).  One workgroup per (sequence, head, 64
// queries); a sequence's key walk is a function of len[b] alone, every row < npad is written (query blocks that start at or past
// len[b] as zeros), nothing past a sequence's rows is read (no slack needed).  Counted in MHIP_K_ATTN_SHORT
int mhip_launch_attention_long(mhip_ctx* ctx, int precision, const AttnShortDesc& d);
// Longformer's attention of the local queries over the same layout (head_dim 64, no bias term): query i of sequence b sees key 0
// (the global token, once) and the keys max(1, i - w) .. min(len[b] - 1, i + w), w the one-sided window, 1 .. ATTN_WINDOW_MAX.  One
// workgroup per (sequence, head, 64 queries) that stages only the keys of its band; every row < npad is written (row 0 and the
// rows >= len[b] finite values nobody reads), nothing past a sequence's rows is read.  Counted in MHIP_K_ATTN_SHORT
constexpr int ATTN_WINDOW_MAX = 512;
int mhip_launch_attention_window(mhip_ctx* ctx, int precision, const AttnShortDesc& d, int w);
// Longformer's attention of the global token: out row b * out_rows = softmax(q_g[b] . k_g[b][j], j < len[b]) v_g[b] + bias, per head
// of 64 columns.  q_g fp32 in the log2 units of the other entries, k / v rows of the precision's element type (k: 16-byte rows),
// bias fp32 [heads * 64] or null.  One workgroup per (sequence, head), online soft-max in fp32.  Counted in MHIP_K_ATTN_SHORT
struct AttnGlobalRowDesc {
  const float* qg = nullptr;      // [seqs][ldq]
  const void* k = nullptr;        // [seqs * npad][ldk]
  const void* v = nullptr;        // [seqs * npad][ldv]
  const float* bias = nullptr;
  void* out = nullptr;            // [..][ldo]
  const int* len = nullptr;       // device, 1 .. npad
  int ldq = 0, ldk = 0, ldv = 0, ldo = 0, npad = 0, heads = 0, seqs = 0;
  long long out_rows = 1;
};
int mhip_launch_attention_global_row(mhip_ctx* ctx, int precision, const AttnGlobalRowDesc& d);
// ------------------------------------------------------------------ BERT sentence encoder ops (berttext_ops.hip)
// h [B*npad][D] fp32 = LN((word[ids[row]] + type0) + pos[pos_offset + row % npad]), ht (null: not written) its copy in the
// precision's element type; word [vocab][D], type0 [D] or null (no token types), pos [>= pos_offset + npad][D] or null (no position
// table) fp32; the ids are the caller's to check
int mhip_launch_berttext_embed(mhip_ctx* ctx, int precision, const float* word, const float* type0, const float* pos, const float* g,
                               const float* b, float eps, const int* ids, float* h, void* ht, int B, int npad, int D, int pos_offset = 0);
// x [R][2 F] -> out [R][F] = gelu_erf(x[:, :F]) * x[:, F:], in the precision's element type; F % 8 == 0
int mhip_launch_geglu(mhip_ctx* ctx, int precision, const void* x, void* out, long long R, int F);
// emb [B][D] fp32: the mean of rows < len[b] of h [B][npad][D] (cls: row 0; len may be null), divided by max(norm, 1e-12) with normalize
int mhip_launch_berttext_pool(mhip_ctx* ctx, const float* h, const int* len, int B, int npad, int D, int cls, int normalize, float* emb);
// out [B][N] fp32 = bias + x W^T over row b * x_rows of x [..][K] (the precision's element type), W [N][K] of the same type: the
// global token's query projection, a wave per output.  K % 8 == 0, 16-byte rows
int mhip_launch_first_row_linear(mhip_ctx* ctx, int precision, const void* x, long long x_rows, const void* w, const float* bias, float* out,
                                 int B, int N, int K);
// the classification head on row b * h_rows of the fp32 stream h [..][D]: logits [B][L] = out_w tanh(dense_w h + dense_b) + out_b,
// scores [B][L] = the logits (function 0), their soft-max (1) or their sigmoid (2).  fp32 weights and arithmetic, one launch, one
// workgroup a text.  D % 4 == 0, D <= 1024, L <= CLS_HEAD_MAX_LABELS
constexpr int CLS_HEAD_MAX_LABELS = 1024;
int mhip_launch_cls_head(mhip_ctx* ctx, const float* h, long long h_rows, const float* dense_w, const float* dense_b, const float* out_w,
                         const float* out_b, int B, int D, int L, int function, float* logits, float* scores);
// ------------------------------------------------------------------ LayoutReader ops (layoutreader_ops.hip)
// A row of the layout-only embedding is 8 ints in HBM: x0, y0, x1, y1, position id, type id, two spare.
constexpr int LR_TOK_INTS = 8;
// h [rows][D] fp32 = LN(pos[p] + x[x0] + y[y0] + x[x1] + y[y1] + h[y1 - y0] + w[x1 - x0] + type[t]), ht (null: not written) its
// copy in the precision's element type; the tables are fp32 [..][D], an index outside its table is clamped into it
struct LrEmbedDesc {
  const int* tok = nullptr;          // [rows][LR_TOK_INTS], device
  const float *pos = nullptr, *xe = nullptr, *ye = nullptr, *he = nullptr, *we = nullptr, *type = nullptr;
  const float *g = nullptr, *b = nullptr;
  float* h = nullptr;
  void* ht = nullptr;
  int rows = 0, D = 0, max_position = 0, max_2d = 0, type_vocab = 0;
  float eps = 1e-5f;
};
int mhip_launch_lr_embed(mhip_ctx* ctx, int precision, const LrEmbedDesc& d);
// Attention of the nq (1 or 2) rows a decode step feeds per page over that page's caches, head dim 64, q scaled by
// head_dim^-0.5 * log2(e).  Query row i of a page sees cache rows [0, src_len[page]), cache rows tgt_base + [0, tgt_len[page * nq
// + i]) and the step's own rows 0 .. i of the page (k / v below): at most LR_ATTN_MAX_KEYS keys.  keep: the own rows 0 .. nq - 2
// are written to the cache rows tgt_base + max(tgt_len of the page) + row (the caller keeps them inside cache_rows).  Rows of the
// caches beyond these lengths are not read.
constexpr int LR_ATTN_MAX_KEYS = 1032;
struct LrDecAttnDesc {
  const void *q = nullptr, *k = nullptr, *v = nullptr;   // [pages * nq][ld] T, head h at column h * 64
  void *kc = nullptr, *vc = nullptr;                     // [pages][cache_rows][heads * 64] T
  void* out = nullptr;                                   // [pages * nq][ldo] T
  const int* src_len = nullptr;                          // [pages], device
  const int* tgt_len = nullptr;                          // [pages * nq], device
  int ld = 0, ldo = 0, pages = 0, heads = 0, nq = 1, cache_rows = 0, tgt_base = 0, keep = 0;
};
int mhip_launch_lr_decode_attention(mhip_ctx* ctx, int precision, const LrDecAttnDesc& d);
// sc[page * sc_stride + j] = LN(x[page * nq + nq - 1]) . E[page][j] + bias[j] for j < S; x [pages * nq][D], E [pages][e_rows][D] fp32
int mhip_launch_lr_pointer_scores(mhip_ctx* ctx, const float* x, int nq, const float* g, const float* b, float eps, const float* E,
                                  int e_rows, const float* bias, int S, int D, int pages, float* sc, long long sc_stride);
// decisions[page][t] = arg-max of sc[page] (lowest index on ties); next_tok [pages][2][LR_TOK_INTS] = the rows of step t + 1: the box
// of source row forced[page][t] (forced null: the decision) of src_tok [pages][e_rows][LR_TOK_INTS] at position src_len[page] + t, and
// the mask row (box 0) at the position after it, both of type tgt_type
int mhip_launch_lr_pointer_select(mhip_ctx* ctx, const float* sc, long long sc_stride, int S, const int* forced, int t, int T,
                                  const int* src_tok, int e_rows, const int* src_len, int tgt_type, int pages, int* decisions,
                                  int* next_tok);
size_t mhip_pil_resize_fragments_scratch(const mhip_crop_desc* descs, int n, int dh, int dw, int filter);
int mhip_pil_resize_fragments(mhip_ctx* ctx, const uint8_t* base_dev, const mhip_crop_desc* descs, int n, uint8_t* dst, int dh,
                              int dw, int filter, void* scratch, size_t scratch_bytes);
