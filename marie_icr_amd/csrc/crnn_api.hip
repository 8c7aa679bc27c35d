// crnn_api.hip — the CRNN-family recognizer (None-VGG-BiLSTM-CTC) behind
// the C ABI of include/marie_hip.h.  Host-side counterpart of Model(opt) in
// marie/models/icr/model.py:25-92 and of CraftOcrProcessor's forward/decode loop in
// marie/document/craft_ocr_processor.py:184-286.
#include <math.h>

#include <memory>

#include "weights_util.h"

// ======================================================================= conv primitive
extern "C" int mhip_conv2d_nhwc(mhip_ctx* ctx, int precision, const mhip_conv_desc* d, const void* in,
                                const void* in2, const void* w, const float* scale, const float* bias, void* out) {
  if (!ctx || !d) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32)
    return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (d->B < 1 || d->H < 1 || d->W < 1 || d->N < 1 || d->KH < 1 || d->KW < 1 || d->pad < 0 || d->pool < 0 ||
      d->pool > 2)
    return mhip_fail(ctx, MHIP_EINVAL, "conv2d: bad descriptor");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  ConvDesc c;
  c.in = in; c.w = w; c.scale = scale; c.bias = bias; c.out = out;
  c.B = d->B; c.H = d->H; c.W = d->W; c.Cin = d->Cin;
  c.KH = d->KH; c.KW = d->KW; c.pad = d->pad;
  c.N = d->N; c.pool = d->pool; c.relu = d->relu; c.out_f32 = d->out_f32;
  c.dil = d->dil > 0 ? d->dil : 1;
  c.in2 = in2; c.Cin1 = d->Cin1;
  c.ldc = d->ldc; c.pad_cols_writable = d->pad_cols_writable;
  return mhip_launch_conv_igemm(ctx, precision, c);
}

// the same primitive with every option of the plain epilogue the model paths use (icr_api.hip's `conv`, the patch embedding of
// vit_api.hip): vertical stride, horizontal padding of its own, residual, periodic output rows
extern "C" int mhip_conv2d_nhwc_ex(mhip_ctx* ctx, int precision, const mhip_conv_ex_desc* d, const void* in,
                                   const void* in2, const void* w, const float* scale, const float* bias, void* out) {
  if (!ctx || !d) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32)
    return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (d->B < 1 || d->H < 1 || d->W < 1 || d->N < 1 || d->KH < 1 || d->KW < 1 || d->pad < 0 || d->pool < 0 ||
      d->pool > 2 || d->sy < 0 || d->pad_x < -1 || d->row_period < 0 || d->row_offset < 0)
    return mhip_fail(ctx, MHIP_EINVAL, "conv2d_ex: bad descriptor");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  ConvDesc c;
  c.in = in; c.w = w; c.scale = scale; c.bias = bias; c.out = out;
  c.B = d->B; c.H = d->H; c.W = d->W; c.Cin = d->Cin;
  c.KH = d->KH; c.KW = d->KW; c.pad = d->pad;
  c.N = d->N; c.pool = d->pool; c.relu = d->relu; c.out_f32 = d->out_f32;
  c.dil = d->dil > 0 ? d->dil : 1;
  c.in2 = in2; c.Cin1 = d->Cin1;
  c.ldc = d->ldc; c.pad_cols_writable = d->pad_cols_writable;
  c.sy = d->sy > 0 ? d->sy : 1;
  c.pad_x = d->pad_x;
  c.res = d->res_dev;
  c.row_period = d->row_period; c.row_stride = d->row_stride; c.row_offset = d->row_offset;
  c.epi = EPI_NONE;
  return mhip_launch_conv_igemm(ctx, precision, c);
}

// ======================================================================= CRNN model
namespace {

struct ConvSpec {
  const char* key;
  int co, ci, kh, kw;
  bool has_bias;
  const char* bn;  // BatchNorm key prefix or nullptr
};
// reference: marie/models/icr/modules/feature_extraction.py:13-25
const ConvSpec kConvs[7] = {
    {"FeatureExtraction.ConvNet.0", 64, 1, 3, 3, true, nullptr},
    {"FeatureExtraction.ConvNet.3", 128, 64, 3, 3, true, nullptr},
    {"FeatureExtraction.ConvNet.6", 256, 128, 3, 3, true, nullptr},
    {"FeatureExtraction.ConvNet.8", 256, 256, 3, 3, true, nullptr},
    {"FeatureExtraction.ConvNet.11", 512, 256, 3, 3, false, "FeatureExtraction.ConvNet.12"},
    {"FeatureExtraction.ConvNet.14", 512, 512, 3, 3, false, "FeatureExtraction.ConvNet.15"},
    {"FeatureExtraction.ConvNet.18", 512, 512, 2, 2, true, nullptr},
};

// byte offsets of the weight blocks in the device arena
struct Layout {
  size_t conv0_w = 0, conv0_b = 0;
  size_t conv_w[7] = {0}, conv_scale[7] = {0}, conv_bias[7] = {0};
  size_t ih_w[2] = {0}, ih_b[2] = {0}, hh_pack[2] = {0}, lin_w[2] = {0}, lin_b[2] = {0};
  size_t pred_w = 0, pred_b = 0;
};

}  // namespace

struct mhip_crnn {
  mhip_ctx* ctx = nullptr;
  int precision = MHIP_PREC_F16;
  int num_class = 0;
  TensorStore store;
  Layout lay;
  Arena arena;
  bool ready = false;
  size_t esz() const { return precision == MHIP_PREC_F16 ? 2 : 4; }
};

namespace {

void build_layout(mhip_crnn* m) {
  Layout& L = m->lay;
  Arena& a = m->arena;
  const size_t es = m->esz();
  L.conv0_w = a.take("conv0_w", 9 * 64 * 4);
  L.conv0_b = a.take("conv0_b", 64 * 4);
  for (int i = 1; i < 7; ++i) {
    const ConvSpec& c = kConvs[i];
    const std::string k = c.key;
    L.conv_w[i] = a.take(k + ".w", (size_t)c.co * c.ci * c.kh * c.kw * es);
    L.conv_scale[i] = a.take(k + ".s", (size_t)c.co * 4);
    L.conv_bias[i] = a.take(k + ".b", (size_t)c.co * 4);
  }
  for (int j = 0; j < 2; ++j) {
    const int in = j == 0 ? 512 : 256;
    const std::string p = "lstm" + std::to_string(j);
    L.ih_w[j] = a.take(p + ".ih_w", (size_t)2048 * in * es);
    L.ih_b[j] = a.take(p + ".ih_b", 2048 * 4);
    L.hh_pack[j] = a.take(p + ".hh_pack", mhip_lstm_wpack_bytes(m->precision));
    L.lin_w[j] = a.take(p + ".lin_w", (size_t)256 * 512 * es);
    L.lin_b[j] = a.take(p + ".lin_b", 256 * 4);
  }
  L.pred_w = a.take("pred_w", (size_t)m->num_class * 256 * es);
  L.pred_b = a.take("pred_b", (size_t)m->num_class * 4);
}

}  // namespace

extern "C" int mhip_crnn_create(mhip_ctx* ctx, int precision, int num_class, mhip_crnn** out) {
  if (!ctx || !out) return MHIP_EINVAL;
  *out = nullptr;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32)
    return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (num_class < 2 || num_class > 256) return mhip_fail(ctx, MHIP_EINVAL, "num_class %d not in [2,256]", num_class);
  mhip_crnn* m = new mhip_crnn();
  m->ctx = ctx;
  m->precision = precision;
  m->num_class = num_class;
  build_layout(m);
  *out = m;
  return MHIP_OK;
}

extern "C" int mhip_crnn_destroy(mhip_crnn* m) {
  if (!m) return MHIP_OK;
  if (m->arena.dev) mhip_quiesce(m->ctx);
  m->arena.release();
  delete m;
  return MHIP_OK;
}

extern "C" int mhip_crnn_set_tensor(mhip_crnn* m, const char* key, const float* data, const int64_t* shape,
                                    int ndim) {
  if (!m || !key) return MHIP_EINVAL;
  return set_conv_model_tensor(m->ctx, m->store, m->ready, key,
                               {"FeatureExtraction.ConvNet.", "SequenceModeling.", "Prediction."}, data, shape, ndim);
}

extern "C" int mhip_crnn_alloc_arena(mhip_crnn* m) {
  if (!m) return MHIP_EINVAL;
  int rc = m->arena.alloc(m->ctx);
  if (rc) return rc;
  m->ready = true;  // contents are the caller's responsibility (RCCL broadcast)
  return MHIP_OK;
}

extern "C" int mhip_crnn_arena(mhip_crnn* m, void** dev, size_t* bytes) {
  if (!m) return MHIP_EINVAL;
  if (dev) *dev = m->arena.dev;
  if (bytes) *bytes = m->arena.bytes;
  return MHIP_OK;
}

extern "C" int mhip_crnn_finalize(mhip_crnn* m) {
  if (!m) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  const TensorStore& st = m->store;
  const Layout& L = m->lay;
  const int prec = m->precision;
  m->arena.begin_fill();
  char* h = m->arena.host.data();

  // conv0: [64][1][3][3] -> tap-major [9][64] fp32
  {
    const HostTensor* w = st.find(ctx, std::string(kConvs[0].key) + ".weight", {64, 1, 3, 3});
    const HostTensor* b = st.find(ctx, std::string(kConvs[0].key) + ".bias", {64});
    if (!w || !b) return MHIP_ESTATE;
    pack_first_conv_weight((float*)(h + L.conv0_w), *w, 64, 1, 9);
    memcpy(h + L.conv0_b, b->data.data(), 64 * 4);
  }
  // conv1..6: [Co][Ci][kh][kw] -> [Co][kh][kw][Ci]; BN folded to per-channel scale/shift (fp32 epilogue)
  for (int i = 1; i < 7; ++i) {
    const ConvSpec& c = kConvs[i];
    const HostTensor* w = st.find(ctx, std::string(c.key) + ".weight", {c.co, c.ci, c.kh, c.kw});
    if (!w) return MHIP_ESTATE;
    pack_conv_weight(prec, h + L.conv_w[i], *w, c.co, c.ci, c.kh * c.kw, c.co, c.ci);
    if (fold_conv_bn(ctx, st, c.key, c.has_bias, c.bn, c.co, c.co, (float*)(h + L.conv_scale[i]),
                     (float*)(h + L.conv_bias[i])))
      return MHIP_ESTATE;
  }
  for (int j = 0; j < 2; ++j)
    if (mhip_lstm_pack_bilstm(ctx, st, "SequenceModeling." + std::to_string(j) + ".", j == 0 ? 512 : 256, prec,
                              h + L.ih_w[j], (float*)(h + L.ih_b[j]), h + L.hh_pack[j], h + L.lin_w[j],
                              (float*)(h + L.lin_b[j])))
      return MHIP_ESTATE;
  {
    const HostTensor* w = st.find(ctx, "Prediction.weight", {m->num_class, 256});
    const HostTensor* b = st.find(ctx, "Prediction.bias", {m->num_class});
    if (!w || !b) return MHIP_ESTATE;
    Arena::put(prec, h + L.pred_w, w->data.data(), (size_t)m->num_class * 256);
    memcpy(h + L.pred_b, b->data.data(), (size_t)m->num_class * 4);
  }
  m->ready = false;
  int rc = m->arena.upload(ctx);
  if (rc) return rc;
  m->ready = true;
  m->store.t.clear();  // host copies are no longer needed
  return MHIP_OK;
}

extern "C" int mhip_crnn_seq_len(int w) { return w / 4 - 1; }

namespace {

constexpr size_t CRNN_ALIGN = 4096;   // every CRNN layout: buffers on 4 KiB boundaries

// the forward's buffers, in layout order
struct CrnnBufs {
  char* act[7];   // outputs of conv layers 0..6
  char *xproj, *hseq, *lin[2], *logits;
};

void crnn_carve(const mhip_crnn* m, Carver& ws, int n, int w, CrnnBufs* b) {
  const size_t es = m->esz();
  const int w2 = w / 2, w4 = w / 4, T = w4 - 1;
  b->act[0] = ws.take((size_t)n * 16 * w2 * 64 * es);
  b->act[1] = ws.take((size_t)n * 8 * w4 * 128 * es);
  b->act[2] = ws.take((size_t)n * 8 * w4 * 256 * es);
  b->act[3] = ws.take((size_t)n * 4 * w4 * 256 * es);
  b->act[4] = ws.take((size_t)n * 4 * w4 * 512 * es);
  b->act[5] = ws.take((size_t)n * 2 * w4 * 512 * es);
  b->act[6] = ws.take((size_t)n * T * 512 * es);
  b->xproj = ws.take((size_t)n * T * 2048 * 4);
  b->hseq = ws.take((size_t)n * T * 512 * es);
  b->lin[0] = ws.take((size_t)n * T * 256 * es);
  b->lin[1] = ws.take((size_t)n * T * 256 * es);
  b->logits = ws.take((size_t)n * T * m->num_class * 4);
}

// device copies of the outputs of the host entries
struct CrnnOut {
  float *logits, *conf;
  int32_t *argmax, *tokens, *lengths;
};

void crnn_out_carve(Carver& ws, int n, int T, int C, bool logits, CrnnOut* o) {
  o->logits = ws.take<float>(logits ? (size_t)n * T * C * 4 : 16);
  o->argmax = ws.take<int32_t>((size_t)n * T * 4);
  o->tokens = ws.take<int32_t>((size_t)n * T * 4);
  o->lengths = ws.take<int32_t>((size_t)n * 4);
  o->conf = ws.take<float>((size_t)n * 4);
}

int crnn_download(mhip_ctx* ctx, const CrnnOut& o, int n, int T, int C, float* logits_h, int32_t* argmax_h, int32_t* tokens_h,
                  int32_t* lengths_h, float* conf_h) {
  const size_t it_b = (size_t)n * T * 4;
  if (logits_h) MHIP_HIP(ctx, hipMemcpyAsync(logits_h, o.logits, it_b * C, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(argmax_h, o.argmax, it_b, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(tokens_h, o.tokens, it_b, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(lengths_h, o.lengths, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(conf_h, o.conf, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

int check_call(mhip_crnn* m, int n, int w) {
  if (!m) return MHIP_EINVAL;
  if (n < 1 || w < 8 || (w % 4) != 0)
    return mhip_fail(m->ctx, MHIP_EINVAL, "crnn: need n >= 1 and w >= 8 with w %% 4 == 0 (got n=%d w=%d)", n, w);
  if ((long long)n * 16 * (w / 2) * 4 > 0x7ffffff0LL)
    return mhip_fail(m->ctx, MHIP_EINVAL, "crnn: batch of %d x %d exceeds one launch; split it", n, w);
  if (!m->ready || !m->arena.dev) return mhip_fail(m->ctx, MHIP_ESTATE, "crnn: weights not finalized");
  return MHIP_OK;
}

// the forward on carved buffers; logits_out NULL: the logits stay in the workspace
int crnn_forward(mhip_crnn* m, const CrnnBufs& p, const uint8_t* crops, int n, int w, float* logits_out, int32_t* argmax,
                 int32_t* tokens, int32_t* lengths, float* conf) {
  mhip_ctx* ctx = m->ctx;
  const Layout& L = m->lay;
  const char* A = m->arena.dev;
  const int prec = m->precision;
  const int w2 = w / 2, w4 = w / 4, T = w4 - 1;

  int rc = mhip_launch_conv_first(ctx, prec, crops, (const float*)(A + L.conv0_w), (const float*)(A + L.conv0_b),
                                  p.act[0], n, 32, w);
  if (rc) return rc;

  struct LayerShape { int H, W, pool; };
  const LayerShape shp[7] = {{0, 0, 0}, {16, w2, POOL_2x2}, {8, w4, POOL_NONE}, {8, w4, POOL_2x1},
                             {4, w4, POOL_NONE}, {4, w4, POOL_2x1}, {2, w4, POOL_NONE}};
  for (int i = 1; i < 7; ++i) {
    const ConvSpec& c = kConvs[i];
    ConvDesc d;
    d.in = p.act[i - 1];
    d.w = A + L.conv_w[i];
    d.scale = c.bn ? (const float*)(A + L.conv_scale[i]) : nullptr;
    d.bias = (const float*)(A + L.conv_bias[i]);
    d.out = p.act[i];
    d.B = n; d.H = shp[i].H; d.W = shp[i].W; d.Cin = c.ci;
    d.KH = c.kh; d.KW = c.kw; d.pad = (c.kh == 3) ? 1 : 0;
    d.N = c.co;
    d.pool = shp[i].pool;
    d.relu = 1;
    rc = mhip_launch_conv_igemm(ctx, prec, d);
    if (rc) return rc;
  }
  // AdaptiveAvgPool2d((None,1)) over H is the identity here: the VGG stack reduces imgH = 32 to H = 1
  // (marie/models/icr/model.py:77-78), so act[6] is already the [n*T][512] sequence.
  const void* seq_in = p.act[6];
  int seq_ch = 512;
  for (int j = 0; j < 2; ++j) {
    ConvDesc g;
    g.in = seq_in; g.w = A + L.ih_w[j]; g.bias = (const float*)(A + L.ih_b[j]); g.out = p.xproj;
    g.B = n * T; g.H = 1; g.W = 1; g.Cin = seq_ch; g.N = 2048; g.out_f32 = 1;
    rc = mhip_launch_conv_igemm(ctx, prec, g);
    if (rc) return rc;
    rc = mhip_launch_lstm_rec(ctx, prec, (const float*)p.xproj, A + L.hh_pack[j], p.hseq, n, T);
    if (rc) return rc;
    ConvDesc l;
    l.in = p.hseq; l.w = A + L.lin_w[j]; l.bias = (const float*)(A + L.lin_b[j]); l.out = p.lin[j];
    l.B = n * T; l.H = 1; l.W = 1; l.Cin = 512; l.N = 256;
    rc = mhip_launch_conv_igemm(ctx, prec, l);
    if (rc) return rc;
    seq_in = p.lin[j];
    seq_ch = 256;
  }
  float* logits = logits_out ? logits_out : (float*)p.logits;
  {
    ConvDesc g;
    g.in = seq_in; g.w = A + L.pred_w; g.bias = (const float*)(A + L.pred_b); g.out = logits;
    g.B = n * T; g.H = 1; g.W = 1; g.Cin = 256; g.N = m->num_class; g.out_f32 = 1;
    rc = mhip_launch_conv_igemm(ctx, prec, g);
    if (rc) return rc;
  }
  return mhip_launch_ctc_decode(ctx, logits, n, T, m->num_class, argmax, tokens, lengths, conf);
}

}  // namespace

extern "C" size_t mhip_crnn_workspace_bytes(mhip_crnn* m, int n, int w) {
  if (!m || n < 1 || w < 8) return 0;
  CrnnBufs b;
  return mhip_layout_bytes([&](Carver& ws) { crnn_carve(m, ws, n, w, &b); }, CRNN_ALIGN);
}

extern "C" double mhip_crnn_kernel_flops(mhip_crnn* m, int kid, int n, int w) {
  if (!m || n < 1 || w < 8) return 0.0;
  const double T = w / 4 - 1, w2 = w / 2, w4 = w / 4;
  switch (kid) {
    case MHIP_K_CONV_FIRST:
      return 2.0 * n * 32 * w * 64 * 9;
    case MHIP_K_CONV_IGEMM: {
      double f = 0;
      f += 2.0 * n * 16 * w2 * 128 * (9 * 64);
      f += 2.0 * n * 8 * w4 * 256 * (9 * 128);
      f += 2.0 * n * 8 * w4 * 256 * (9 * 256);
      f += 2.0 * n * 4 * w4 * 512 * (9 * 256);
      f += 2.0 * n * 4 * w4 * 512 * (9 * 512);
      f += 2.0 * n * T * 512 * (4 * 512);
      f += 2.0 * n * T * 2048 * 512 + 2.0 * n * T * 256 * 512;   // BiLSTM-0 input projection + linear
      f += 2.0 * n * T * 2048 * 256 + 2.0 * n * T * 256 * 512;   // BiLSTM-1
      f += 2.0 * n * T * m->num_class * 256;                     // prediction
      return f;
    }
    case MHIP_K_LSTM_REC:
      return 2.0 * (2.0 * n * T * 2 * 1024 * 256);
    default:
      return 0.0;
  }
}

extern "C" int mhip_crnn_forward(mhip_crnn* m, const uint8_t* crops, int n, int w, float* logits_out,
                                 int32_t* argmax, int32_t* tokens, int32_t* lengths, float* conf) {
  int rc = check_call(m, n, w);
  if (rc) return rc;
  mhip_ctx* ctx = m->ctx;
  if (!crops || !argmax || !tokens || !lengths || !conf) return mhip_fail(ctx, MHIP_EINVAL, "crnn: null buffer");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  CrnnBufs b;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { crnn_carve(m, ws, n, w, &b); }, CRNN_ALIGN))) return rc;
  return crnn_forward(m, b, crops, n, w, logits_out, argmax, tokens, lengths, conf);
}

extern "C" int mhip_crnn_forward_host(mhip_crnn* m, const uint8_t* crops_h, int n, int w, float* logits_h,
                                      int32_t* argmax_h, int32_t* tokens_h, int32_t* lengths_h, float* conf_h) {
  int rc = check_call(m, n, w);
  if (rc) return rc;
  mhip_ctx* ctx = m->ctx;
  if (!crops_h || !argmax_h || !tokens_h || !lengths_h || !conf_h)
    return mhip_fail(ctx, MHIP_EINVAL, "crnn: null host buffer");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const int T = w / 4 - 1, C = m->num_class;
  const size_t in_b = (size_t)n * 32 * w;
  CrnnBufs b;
  uint8_t* in = nullptr;
  CrnnOut o;
  rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    crnn_carve(m, ws, n, w, &b);   // I/O staging lives behind the forward's buffers
    in = ws.take<uint8_t>(in_b);
    crnn_out_carve(ws, n, T, C, logits_h != nullptr, &o);
  }, CRNN_ALIGN);
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(in, crops_h, in_b, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = crnn_forward(m, b, in, n, w, logits_h ? o.logits : nullptr, o.argmax, o.tokens, o.lengths, o.conf))) return rc;
  return crnn_download(ctx, o, n, T, C, logits_h, argmax_h, tokens_h, lengths_h, conf_h);
}

// ======================================================================= crop batcher + composite entries
extern "C" int mhip_crop_batch(mhip_ctx* ctx, const uint8_t* base_dev, const mhip_crop_desc* descs, int n, int img_w,
                               uint8_t* out_dev) {
  if (!ctx || !descs || n < 1 || img_w < 1) return MHIP_EINVAL;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  void* scratch = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) { scratch = ws.take(mhip_crop_scratch_bytes(descs, n, 32, img_w)); });
  if (rc) return rc;
  return mhip_launch_crop_batch(ctx, base_dev, descs, n, 32, img_w, scratch, out_dev);
}

namespace {

int forward_crops_impl(mhip_crnn* m, const uint8_t* base_dev, const uint8_t* packed_host, size_t packed_bytes,
                       const mhip_crop_desc* descs, int n, int img_w, float* logits_h, int32_t* argmax_h,
                       int32_t* tokens_h, int32_t* lengths_h, float* conf_h) {
  int rc = check_call(m, n, img_w);
  if (rc) return rc;
  mhip_ctx* ctx = m->ctx;
  if (!descs || !argmax_h || !tokens_h || !lengths_h || !conf_h) return mhip_fail(ctx, MHIP_EINVAL, "crnn: null buffer");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const int T = img_w / 4 - 1, C = m->num_class;
  CrnnBufs b;
  uint8_t* crops = nullptr;
  void* scratch = nullptr;
  CrnnOut o;
  uint8_t* packed = nullptr;
  rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    crnn_carve(m, ws, n, img_w, &b);
    crops = ws.take<uint8_t>((size_t)n * 32 * img_w);
    scratch = ws.take(mhip_crop_scratch_bytes(descs, n, 32, img_w));
    crnn_out_carve(ws, n, T, C, logits_h != nullptr, &o);
    if (packed_host) packed = ws.take<uint8_t>(packed_bytes);
  }, CRNN_ALIGN);
  if (rc) return rc;
  if (packed_host) {
    MHIP_HIP(ctx, hipMemcpyAsync(packed, packed_host, packed_bytes, hipMemcpyHostToDevice, ctx->stream));
    base_dev = packed;
  }
  rc = mhip_launch_crop_batch(ctx, base_dev, descs, n, 32, img_w, scratch, crops);
  if (rc) return rc;
  if ((rc = crnn_forward(m, b, crops, n, img_w, logits_h ? o.logits : nullptr, o.argmax, o.tokens, o.lengths, o.conf))) return rc;
  return crnn_download(ctx, o, n, T, C, logits_h, argmax_h, tokens_h, lengths_h, conf_h);
}

}  // namespace
extern "C" int mhip_crnn_forward_crops(mhip_crnn* m, const uint8_t* base_dev, const mhip_crop_desc* descs, int n,
                                       int img_w, float* logits_h, int32_t* argmax_h, int32_t* tokens_h,
                                       int32_t* lengths_h, float* conf_h) {
  if (!m || !base_dev) return MHIP_EINVAL;
  return forward_crops_impl(m, base_dev, nullptr, 0, descs, n, img_w, logits_h, argmax_h, tokens_h, lengths_h, conf_h);
}

extern "C" int mhip_crnn_forward_fragments_host(mhip_crnn* m, const uint8_t* packed_host, size_t packed_bytes,
                                                const mhip_crop_desc* descs, int n, int img_w, float* logits_h,
                                                int32_t* argmax_h, int32_t* tokens_h, int32_t* lengths_h,
                                                float* conf_h) {
  if (!m || !packed_host || !packed_bytes) return MHIP_EINVAL;
  return forward_crops_impl(m, nullptr, packed_host, packed_bytes, descs, n, img_w, logits_h, argmax_h, tokens_h,
                            lengths_h, conf_h);
}
