// cliprn_api.hip — CLIP's ModifiedResNet vision tower (RN50 / RN101 / RN50x4: the snippet embeddings of the template matchers'
// default model, marie/clip-snippet-rn50x4) behind the C ABI.
//
// Host-side counterpart of clip/model.py: ModifiedResNet.forward (the three-convolution stem, four layers of Bottleneck blocks
// whose strides are average pools, AttentionPool2d) behind CLIP.encode_image, as OpenAIEmbeddings.get_single_image_embedding
// drives it (marie/embeddings/openai/openai_embeddings.py:146-157).  One object = one weight arena + the launch sequence.
//
// Layout: activations are NHWC in the mode's element type with every channel count rounded up to what conv_igemm takes (64
// f16 / 32 f32 channels: 40 -> 64, 80 -> 128 / 96, 160 -> 192 / 160); weight rows and columns, scales and biases are padded
// with zeros, so a padding channel is 0 * x + 0 = 0 after every convolution, ReLU, pool and residual add.  Every BatchNorm is
// folded into the scale / bias of its convolution.  A Bottleneck is
//   t1 = relu(bn1(conv1 x))   t2 = relu(bn2(conv2 t1))   [t2 = avgpool(t2)]
//   id = x, or bn(conv(avgpool(x)))                      out = relu(bn3(conv3 t2) + id)      (the add is conv3's residual epilogue)
// and the attention pool: tokens = (mean | map) + positions -> q (one row a clip) and k | v (one GEMM, N = 2 embed_dim) ->
// one-query attention per (clip, head) -> c_proj.
#include <math.h>

#include "weights_util.h"

struct mhip_cliprn {
  mhip_ctx* ctx = nullptr;
  int precision = MHIP_PREC_F16;
  mhip_cliprn_config cfg{};
  TensorStore store;
  Arena arena;
  bool ready = false;
  size_t esz() const { return precision == MHIP_PREC_F16 ? 2 : 4; }
  int cp(int c) const { const int q = 128 / (int)esz(); return (c + q - 1) / q * q; }      // channels as the conv primitive takes them
  int embed_dim() const { return 32 * cfg.width; }
  int grid() const { return cfg.image_size / 32; }
  int n_tok() const { return grid() * grid() + 1; }
};

namespace {

const float CLIP_MEAN[3] = {0.48145466f, 0.4578275f, 0.40821073f};
const float CLIP_STD[3] = {0.26862954f, 0.26130258f, 0.27577711f};
constexpr int MAX_CLIPS = 1024, MAX_WIDTH = 128, MAX_BLOCKS = 64, N_TAPS = 6;

struct RnBlock {
  std::string name;      // arena prefix, "l<layer>.<index>."
  std::string key;       // checkpoint prefix, "visual.layer<layer>.<index>."
  int cin, planes, stride, H;      // input channels and (square) input map
  bool down, last;       // has a downsample path; the last block of its layer
};

std::vector<RnBlock> rn_blocks(const mhip_cliprn_config& c) {
  std::vector<RnBlock> out;
  int cin = c.width, H = c.image_size / 4;
  for (int l = 0; l < 4; ++l) {
    const int planes = c.width << l;
    for (int i = 0; i < c.layers[l]; ++i) {
      RnBlock b;
      b.name = "l" + std::to_string(l + 1) + "." + std::to_string(i) + ".";
      b.key = "visual.layer" + std::to_string(l + 1) + "." + std::to_string(i) + ".";
      b.cin = cin; b.planes = planes; b.stride = (i == 0 && l > 0) ? 2 : 1; b.H = H;
      b.down = b.stride > 1 || cin != 4 * planes;
      b.last = i == c.layers[l] - 1;
      out.push_back(b);
      cin = 4 * planes;
      H /= b.stride;
    }
  }
  return out;
}

// tap i: 0 the stem after its pool, 1 .. 4 the layers, 5 the embedding -> (H, W, C)
void rn_tap_shape(const mhip_cliprn_config& c, int i, int32_t shape[3]) {
  if (i == 5) { shape[0] = shape[1] = 1; shape[2] = c.proj_dim; return; }
  const int H = i == 0 ? c.image_size / 4 : (c.image_size / 4) >> (i - 1);
  shape[0] = shape[1] = H;
  shape[2] = i == 0 ? c.width : (4 * c.width) << (i - 1);
}

// the buffers of one call of B clips (and n_pairs cosines)
struct RnRun {
  uint8_t* clips = nullptr;
  int *pair_a = nullptr, *pair_b = nullptr;
  float* cos = nullptr;
  char *x[2] = {nullptr, nullptr};      // block input / output, alternating; the stem's maps
  char *t1 = nullptr, *t2 = nullptr, *t3 = nullptr, *xi = nullptr, *id = nullptr;      // conv1, conv2, pooled conv2, pooled input, downsample
  char *tok = nullptr, *xq = nullptr;
  float *q = nullptr, *kv = nullptr, *ao = nullptr, *emb = nullptr;
  float* tap = nullptr;                 // fp32 copy of a tapped map, padded channels included (taps only)
};

void cliprn_carve(const mhip_cliprn* m, Carver& ws, int B, int n_pairs, bool taps, RnRun* r) {
  const mhip_cliprn_config& c = m->cfg;
  const size_t es = m->esz(), S = c.image_size, E = m->embed_dim(), NT = m->n_tok();
  const size_t S2 = S / 2, S4 = S / 4;
  size_t x = std::max(S2 * S2 * (size_t)std::max(m->cp(c.width / 2), m->cp(c.width)), S4 * S4 * (size_t)m->cp(c.width));
  size_t t = 0, t3 = 0, xi = 0, id = 0, tap = S4 * S4 * (size_t)m->cp(c.width);
  for (const RnBlock& b : rn_blocks(c)) {
    const size_t H = b.H, Ho = b.H / b.stride;
    x = std::max(x, std::max(H * H * m->cp(b.cin), Ho * Ho * m->cp(4 * b.planes)));
    t = std::max(t, H * H * m->cp(b.planes));
    if (b.stride > 1) { t3 = std::max(t3, Ho * Ho * m->cp(b.planes)); xi = std::max(xi, Ho * Ho * m->cp(b.cin)); }
    if (b.down) id = std::max(id, Ho * Ho * m->cp(4 * b.planes));
    tap = std::max(tap, Ho * Ho * (size_t)m->cp(4 * b.planes));
  }
  r->clips = ws.take<uint8_t>((size_t)B * S * S * 3);
  r->pair_a = n_pairs ? ws.take<int>((size_t)n_pairs * 4) : nullptr;
  r->pair_b = n_pairs ? ws.take<int>((size_t)n_pairs * 4) : nullptr;
  r->cos = n_pairs ? ws.take<float>((size_t)n_pairs * 4) : nullptr;
  r->x[0] = ws.take(B * x * es);
  r->x[1] = ws.take(B * x * es);
  r->t1 = ws.take(B * t * es);
  r->t2 = ws.take(B * t * es);
  r->t3 = t3 ? ws.take(B * t3 * es) : nullptr;
  r->xi = xi ? ws.take(B * xi * es) : nullptr;
  r->id = id ? ws.take(B * id * es) : nullptr;
  r->tok = ws.take(B * NT * E * es);
  r->xq = ws.take(B * E * es);
  r->q = ws.take<float>(B * E * 4);
  r->kv = ws.take<float>(B * NT * 2 * E * 4);
  r->ao = ws.take<float>(B * E * 4);
  r->emb = ws.take<float>((size_t)B * c.proj_dim * 4);
  r->tap = taps ? ws.take<float>(B * tap * 4) : nullptr;
}

// one convolution of the tower through the conv primitive: `name`_w / _s / _b of the arena, k x k, pad k / 2
int rn_conv(mhip_cliprn* m, const std::string& name, const void* in, int B, int H, int cin_p, int k, int n_p, bool relu, const void* res,
            void* out) {
  const Arena& a = m->arena;
  ConvDesc cd;
  cd.in = in; cd.w = a.d(name + "_w"); cd.scale = a.d<float>(name + "_s"); cd.bias = a.d<float>(name + "_b"); cd.out = out;
  cd.B = B; cd.H = H; cd.W = H; cd.Cin = cin_p; cd.KH = cd.KW = k; cd.pad = k / 2; cd.N = n_p;
  cd.relu = relu ? ACT_RELU : ACT_NONE;
  cd.res = res;
  return mhip_launch_conv_igemm(m->ctx, m->precision, cd);
}

// clips staged in run.clips -> embeddings in run.emb.  taps (host, or null): the stem after its pool and the four layers, fp32
// NHWC with the checkpoint's channel counts, one after another
int cliprn_forward(mhip_cliprn* m, int B, int swap_rb, const RnRun& run, float* taps) {
  mhip_ctx* ctx = m->ctx;
  const mhip_cliprn_config& c = m->cfg;
  const int prec = m->precision, S = c.image_size, E = m->embed_dim(), NT = m->n_tok();
  const int c0 = m->cp(c.width / 2), c1 = m->cp(c.width);
  const Arena& a = m->arena;
  int rc;
  float* tap_at = taps;
  auto tap = [&](const void* map, int H, int C) -> int {      // C: the checkpoint's channel count of the map
    if (!taps) return MHIP_OK;
    const int Cp = m->cp(C);
    const size_t rows = (size_t)B * H * H;
    int r = mhip_launch_convert_rows(ctx, prec, map, run.tap, (int)rows, Cp);
    if (r) return r;
    MHIP_HIP(ctx, hipMemcpy2DAsync(tap_at, (size_t)C * 4, run.tap, (size_t)Cp * 4, (size_t)C * 4, rows, hipMemcpyDeviceToHost, ctx->stream));
    MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // run.tap is reused by the next tap
    tap_at += rows * C;
    return MHIP_OK;
  };
  if ((rc = mhip_launch_cliprn_stem(ctx, prec, run.clips, B, S, swap_rb, CLIP_MEAN, CLIP_STD, a.d<float>("s1_w"), a.d<float>("s1_s"),
                                    a.d<float>("s1_b"), run.x[0], c0)))
    return rc;
  if ((rc = rn_conv(m, "s2", run.x[0], B, S / 2, c0, 3, c0, true, nullptr, run.x[1]))) return rc;
  if ((rc = rn_conv(m, "s3", run.x[1], B, S / 2, c0, 3, c1, true, nullptr, run.x[0]))) return rc;
  if ((rc = mhip_launch_avgpool_nhwc(ctx, prec, 2, run.x[0], run.x[1], B, S / 2, S / 2, c1))) return rc;
  if ((rc = tap(run.x[1], S / 4, c.width))) return rc;
  int cur = 1;
  for (const RnBlock& b : rn_blocks(c)) {
    const int H = b.H, Ho = H / b.stride, cin = m->cp(b.cin), pp = m->cp(b.planes), co = m->cp(4 * b.planes);
    const char* x = run.x[cur];
    if ((rc = rn_conv(m, b.name + "c1", x, B, H, cin, 1, pp, true, nullptr, run.t1))) return rc;
    if ((rc = rn_conv(m, b.name + "c2", run.t1, B, H, pp, 3, pp, true, nullptr, run.t2))) return rc;
    const char* t = run.t2;
    if (b.stride > 1) {
      if ((rc = mhip_launch_avgpool_nhwc(ctx, prec, 2, run.t2, run.t3, B, H, H, pp))) return rc;
      t = run.t3;
    }
    const char* idn = x;
    if (b.down) {
      const char* xi = x;
      if (b.stride > 1) {
        if ((rc = mhip_launch_avgpool_nhwc(ctx, prec, 2, x, run.xi, B, H, H, cin))) return rc;
        xi = run.xi;
      }
      if ((rc = rn_conv(m, b.name + "ds", xi, B, Ho, cin, 1, co, false, nullptr, run.id))) return rc;
      idn = run.id;
    }
    if ((rc = rn_conv(m, b.name + "c3", t, B, Ho, pp, 1, co, true, idn, run.x[cur ^ 1]))) return rc;
    cur ^= 1;
    if (b.last && (rc = tap(run.x[cur], Ho, 4 * b.planes))) return rc;
  }
  // the attention pool: the last map is [B][NT - 1][E], E = 32 width has no padding channels
  if ((rc = mhip_launch_cliprn_tokens(ctx, prec, run.x[cur], a.d<float>("pos"), run.tok, run.xq, B, NT - 1, E))) return rc;
  if ((rc = mhip_gemm(ctx, prec, run.xq, a.d("q_w"), B, E, E, a.d<float>("q_s"), a.d<float>("q_b"), run.q, ACT_NONE, 1))) return rc;
  if ((rc = mhip_gemm(ctx, prec, run.tok, a.d("kv_w"), (long long)B * NT, 2 * E, E, nullptr, a.d<float>("kv_b"), run.kv, ACT_NONE, 1))) return rc;
  if ((rc = mhip_launch_cliprn_attn1q(ctx, run.q, run.kv, run.ao, B, NT, E))) return rc;
  return mhip_launch_cliprn_cproj(ctx, run.ao, B, E, a.d<float>("c_w"), a.d<float>("c_b"), c.proj_dim, run.emb);
}

int cliprn_check_call(mhip_cliprn* m, const uint8_t* clips, int B) {
  if (!m->ready) return mhip_fail(m->ctx, MHIP_ESTATE, "cliprn: weights not finalized");
  if (!clips || B < 1 || B > MAX_CLIPS) return mhip_fail(m->ctx, MHIP_EINVAL, "cliprn: bad arguments (%d clips; 1 .. %d)", B, MAX_CLIPS);
  return MHIP_OK;
}

int cliprn_upload(mhip_cliprn* m, const uint8_t* clips_host, int B, const RnRun& run) {
  const size_t S = m->cfg.image_size;
  MHIP_HIP(m->ctx, hipMemcpyAsync(run.clips, clips_host, (size_t)B * S * S * 3, hipMemcpyHostToDevice, m->ctx->stream));
  return MHIP_OK;
}

// an eval-mode BatchNorm (`bn` prefix) as the scale / bias of the convolution in front of it; `np` entries, the padding 1 / 0
bool fold_bn(mhip_ctx* ctx, const TensorStore& st, const std::string& bn, int co, int np, float eps, float* scale, float* bias) {
  const HostTensor* g = st.find(ctx, bn + ".weight", {co});
  const HostTensor* be = st.find(ctx, bn + ".bias", {co});
  const HostTensor* mu = st.find(ctx, bn + ".running_mean", {co});
  const HostTensor* va = st.find(ctx, bn + ".running_var", {co});
  if (!g || !be || !mu || !va) return false;
  std::fill(scale, scale + np, 1.f);
  std::fill(bias, bias + np, 0.f);
  for (int o = 0; o < co; ++o) {
    const float s = g->data[o] / sqrtf(va->data[o] + eps);
    scale[o] = s;
    bias[o] = be->data[o] - mu->data[o] * s;
  }
  return true;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- lifecycle
extern "C" int mhip_cliprn_create(mhip_ctx* ctx, int precision, const mhip_cliprn_config* cfg, mhip_cliprn** out) {
  if (!ctx || !out || !cfg) return MHIP_EINVAL;
  *out = nullptr;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  const mhip_cliprn_config& c = *cfg;
  if (c.image_size < 32 || c.image_size % 32 || c.image_size > 512)
    return mhip_fail(ctx, MHIP_EINVAL, "cliprn: image_size %d (a multiple of 32 up to 512: the attention pool takes up to 257 tokens)", c.image_size);
  if (c.width < 2 || c.width % 2)
    return mhip_fail(ctx, MHIP_EINVAL, "cliprn: width %d is odd: the attention pool's heads (embed_dim %d over %d heads) are not 64 wide",
                     c.width, 32 * c.width, c.width * 32 / 64);
  if (c.width > MAX_WIDTH)
    return mhip_fail(ctx, MHIP_EINVAL, "cliprn: width %d (up to %d: the stem kernel takes 64 channels, the attention pool 4096)", c.width, MAX_WIDTH);
  for (int l = 0; l < 4; ++l)
    if (c.layers[l] < 1 || c.layers[l] > MAX_BLOCKS)
      return mhip_fail(ctx, MHIP_EINVAL, "cliprn: layers[%d] = %d (1 .. %d blocks)", l, c.layers[l], MAX_BLOCKS);
  if (c.proj_dim < 1 || c.proj_dim > 65536) return mhip_fail(ctx, MHIP_EINVAL, "cliprn: proj_dim %d", c.proj_dim);
  if (!(c.bn_eps > 0.f)) return mhip_fail(ctx, MHIP_EINVAL, "cliprn: bn_eps");
  mhip_cliprn* m = new mhip_cliprn();
  m->ctx = ctx;
  m->precision = precision;
  m->cfg = c;
  const size_t es = m->esz(), E = m->embed_dim();
  if (!mhip_cliprn_attnpool_ok(m->n_tok() - 1, (int)E, c.proj_dim)) {
    delete m;
    return mhip_fail(ctx, MHIP_EINVAL, "cliprn: the attention pool does not take %d tokens of %zu", m->n_tok(), E);
  }
  Arena& a = m->arena;
  auto conv = [&](const std::string& name, int cin, int k, int co) {
    a.take(name + "_w", (size_t)m->cp(co) * k * k * m->cp(cin) * es);
    a.take(name + "_s", (size_t)m->cp(co) * 4);
    a.take(name + "_b", (size_t)m->cp(co) * 4);
  };
  const int c0 = m->cp(c.width / 2);
  a.take("s1_w", (size_t)27 * c0 * 4); a.take("s1_s", (size_t)c0 * 4); a.take("s1_b", (size_t)c0 * 4);
  conv("s2", c.width / 2, 3, c.width / 2);
  conv("s3", c.width / 2, 3, c.width);
  for (const RnBlock& b : rn_blocks(c)) {
    conv(b.name + "c1", b.cin, 1, b.planes);
    conv(b.name + "c2", b.planes, 3, b.planes);
    conv(b.name + "c3", b.planes, 1, 4 * b.planes);
    if (b.down) conv(b.name + "ds", b.cin, 1, 4 * b.planes);
  }
  a.take("pos", (size_t)m->n_tok() * E * 4);
  a.take("q_w", E * E * es); a.take("q_s", E * 4); a.take("q_b", E * 4);
  a.take("kv_w", 2 * E * E * es); a.take("kv_b", 2 * E * 4);
  a.take("c_w", (size_t)c.proj_dim * E * 4); a.take("c_b", (size_t)c.proj_dim * 4);
  *out = m;
  return MHIP_OK;
}

extern "C" int mhip_cliprn_destroy(mhip_cliprn* m) {
  if (!m) return MHIP_OK;
  mhip_quiesce(m->ctx);
  m->arena.release();
  delete m;
  return MHIP_OK;
}

extern "C" int mhip_cliprn_set_tensor(mhip_cliprn* m, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!m || !key) return MHIP_EINVAL;
  return set_conv_model_tensor(m->ctx, m->store, m->ready, key, {"visual."}, data, shape, ndim);
}

extern "C" int mhip_cliprn_alloc_arena(mhip_cliprn* m) {
  if (!m) return MHIP_EINVAL;
  int rc = m->arena.alloc(m->ctx);
  if (rc) return rc;
  m->ready = true;
  return MHIP_OK;
}

extern "C" int mhip_cliprn_arena(mhip_cliprn* m, void** dev, size_t* bytes) {
  if (!m) return MHIP_EINVAL;
  if (dev) *dev = m->arena.dev;
  if (bytes) *bytes = m->arena.bytes;
  return MHIP_OK;
}

extern "C" int mhip_cliprn_finalize(mhip_cliprn* m) {
  if (!m) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  const mhip_cliprn_config& c = m->cfg;
  const int prec = m->precision, E = m->embed_dim(), NT = m->n_tok(), P = c.proj_dim, w2 = c.width / 2;
  Arena& a = m->arena;
  const TensorStore& st = m->store;
  a.begin_fill();
  // `conv`.weight [co][cin][k][k] + the BatchNorm `bn` -> `name`_w / _s / _b
  auto conv = [&](const std::string& name, const std::string& key, const std::string& bn, int cin, int k, int co) -> bool {
    const HostTensor* w = st.find(ctx, key + ".weight", {co, cin, k, k});
    if (!w) return false;
    pack_conv_weight(prec, a.h(name + "_w"), *w, co, cin, k * k, m->cp(co), m->cp(cin));
    return fold_bn(ctx, st, bn, co, m->cp(co), c.bn_eps, (float*)a.h(name + "_s"), (float*)a.h(name + "_b"));
  };
  {
    const HostTensor* w = st.find(ctx, "visual.conv1.weight", {w2, 3, 3, 3});
    if (!w) return MHIP_ESTATE;
    const int c0 = m->cp(w2);
    float* dst = (float*)a.h("s1_w");      // [(dy * 3 + dx) * 3 + c][c0]
    for (int o = 0; o < w2; ++o)
      for (int ch = 0; ch < 3; ++ch)
        for (int t = 0; t < 9; ++t) dst[(size_t)(t * 3 + ch) * c0 + o] = w->data[((size_t)o * 3 + ch) * 9 + t];
    if (!fold_bn(ctx, st, "visual.bn1", w2, c0, c.bn_eps, (float*)a.h("s1_s"), (float*)a.h("s1_b"))) return MHIP_ESTATE;
  }
  if (!conv("s2", "visual.conv2", "visual.bn2", w2, 3, w2)) return MHIP_ESTATE;
  if (!conv("s3", "visual.conv3", "visual.bn3", w2, 3, c.width)) return MHIP_ESTATE;
  for (const RnBlock& b : rn_blocks(c)) {
    if (!conv(b.name + "c1", b.key + "conv1", b.key + "bn1", b.cin, 1, b.planes)) return MHIP_ESTATE;
    if (!conv(b.name + "c2", b.key + "conv2", b.key + "bn2", b.planes, 3, b.planes)) return MHIP_ESTATE;
    if (!conv(b.name + "c3", b.key + "conv3", b.key + "bn3", b.planes, 1, 4 * b.planes)) return MHIP_ESTATE;
    if (b.down && !conv(b.name + "ds", b.key + "downsample.0", b.key + "downsample.1", b.cin, 1, 4 * b.planes)) return MHIP_ESTATE;
  }
  const std::string ap = "visual.attnpool.";
  const HostTensor* pos = st.find(ctx, ap + "positional_embedding", {NT, E});
  const HostTensor* qw = st.find(ctx, ap + "q_proj.weight", {E, E});
  const HostTensor* qb = st.find(ctx, ap + "q_proj.bias", {E});
  const HostTensor* kw = st.find(ctx, ap + "k_proj.weight", {E, E});
  const HostTensor* kb = st.find(ctx, ap + "k_proj.bias", {E});
  const HostTensor* vw = st.find(ctx, ap + "v_proj.weight", {E, E});
  const HostTensor* vb = st.find(ctx, ap + "v_proj.bias", {E});
  const HostTensor* cw = st.find(ctx, ap + "c_proj.weight", {P, E});
  const HostTensor* cb = st.find(ctx, ap + "c_proj.bias", {P});
  if (!pos || !qw || !qb || !kw || !kb || !vw || !vb || !cw || !cb) return MHIP_ESTATE;
  memcpy(a.h("pos"), pos->data.data(), pos->numel() * 4);
  const size_t es = m->esz(), EE = (size_t)E * E;
  Arena::put(prec, a.h("q_w"), qw->data.data(), EE);
  Arena::put(prec, a.h("kv_w"), kw->data.data(), EE);
  Arena::put(prec, a.h("kv_w") + EE * es, vw->data.data(), EE);
  float *qs = (float*)a.h("q_s"), *qbias = (float*)a.h("q_b"), *kvb = (float*)a.h("kv_b");
  for (int i = 0; i < E; ++i) {      // q = (x Wq^T + bq) * 64^-0.5
    qs[i] = 0.125f; qbias[i] = qb->data[i] * 0.125f;
    kvb[i] = kb->data[i]; kvb[E + i] = vb->data[i];
  }
  memcpy(a.h("c_w"), cw->data.data(), cw->numel() * 4);
  memcpy(a.h("c_b"), cb->data.data(), (size_t)P * 4);
  int rc = a.upload(ctx);
  if (rc) return rc;
  m->ready = true;
  m->store.t.clear();
  return MHIP_OK;
}

extern "C" size_t mhip_cliprn_workspace_bytes(mhip_cliprn* m, int B) {
  if (!m || B < 1 || B > MAX_CLIPS) return 0;
  RnRun run;
  return mhip_layout_bytes([&](Carver& ws) { cliprn_carve(m, ws, B, 0, false, &run); });
}

extern "C" int mhip_cliprn_tap_shape(mhip_cliprn* m, int i, int32_t shape[3]) {
  if (!m || !shape) return MHIP_EINVAL;
  if (i < 0 || i >= N_TAPS) return mhip_fail(m->ctx, MHIP_EINVAL, "cliprn: tap %d (0 the stem, 1 .. 4 the layers, 5 the embedding)", i);
  rn_tap_shape(m->cfg, i, shape);
  return MHIP_OK;
}

// ---------------------------------------------------------------------------------------------------- forward
extern "C" int mhip_cliprn_embed_host(mhip_cliprn* m, const uint8_t* clips_host, int B, int swap_rb, float* emb_out) {
  if (!m || !emb_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = cliprn_check_call(m, clips_host, B);
  if (rc) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  RnRun run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { cliprn_carve(m, ws, B, 0, false, &run); }))) return rc;
  if ((rc = cliprn_upload(m, clips_host, B, run))) return rc;
  if ((rc = cliprn_forward(m, B, swap_rb, run, nullptr))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(emb_out, run.emb, (size_t)B * m->cfg.proj_dim * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_cliprn_embed_pairs_host(mhip_cliprn* m, const uint8_t* clips_host, int n_clips, const int32_t* pair_a,
                                            const int32_t* pair_b, int n_pairs, float* emb_out, float* cos_out) {
  if (!m || !pair_a || !pair_b || !cos_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = cliprn_check_call(m, clips_host, n_clips);
  if (rc) return rc;
  if (n_pairs < 1 || n_pairs > (1 << 24)) return mhip_fail(ctx, MHIP_EINVAL, "cliprn: %d pairs", n_pairs);
  for (int p = 0; p < n_pairs; ++p)
    if (pair_a[p] < 0 || pair_a[p] >= n_clips || pair_b[p] < 0 || pair_b[p] >= n_clips)
      return mhip_fail(ctx, MHIP_EINVAL, "cliprn: pair %d names clips %d and %d of %d", p, pair_a[p], pair_b[p], n_clips);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  RnRun run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { cliprn_carve(m, ws, n_clips, n_pairs, false, &run); }))) return rc;
  if ((rc = cliprn_upload(m, clips_host, n_clips, run))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.pair_a, pair_a, (size_t)n_pairs * 4))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.pair_b, pair_b, (size_t)n_pairs * 4))) return rc;
  if ((rc = cliprn_forward(m, n_clips, 1, run, nullptr))) return rc;      // the matcher's clips are BGR
  if ((rc = mhip_launch_pair_cosine(ctx, run.emb, m->cfg.proj_dim, run.pair_a, run.pair_b, n_pairs, run.cos))) return rc;
  if (emb_out) MHIP_HIP(ctx, hipMemcpyAsync(emb_out, run.emb, (size_t)n_clips * m->cfg.proj_dim * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(cos_out, run.cos, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_cliprn_debug_taps_host(mhip_cliprn* m, const uint8_t* clips_host, int B, int swap_rb, float* taps_out,
                                           float* emb_out) {
  if (!m || !taps_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = cliprn_check_call(m, clips_host, B);
  if (rc) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  RnRun run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { cliprn_carve(m, ws, B, 0, true, &run); }))) return rc;
  if ((rc = cliprn_upload(m, clips_host, B, run))) return rc;
  if ((rc = cliprn_forward(m, B, swap_rb, run, taps_out))) return rc;
  if (emb_out) MHIP_HIP(ctx, hipMemcpyAsync(emb_out, run.emb, (size_t)B * m->cfg.proj_dim * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

// ---------------------------------------------------------------------------------------------------- the kernels alone
extern "C" int mhip_cliprn_stem_host(mhip_ctx* ctx, int precision, const uint8_t* clips, int B, int S, int swap_rb, const float* w,
                                     const float* scale, const float* bias, int C0, float* out) {
  if (!ctx || !clips || !w || !scale || !bias || !out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (B < 1 || B > MAX_CLIPS || S < 2 || S % 2 || S > 512 || C0 < 1 || C0 > 64)
    return mhip_fail(ctx, MHIP_EINVAL, "cliprn_stem: B=%d S=%d (even, up to 512) C0=%d (up to 64)", B, S, C0);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t es = precision == MHIP_PREC_F16 ? 2 : 4, Cp = (C0 + 7) / 8 * 8, rows = (size_t)B * (S / 2) * (S / 2);
  std::vector<float> pack(29 * Cp, 0.f);      // the weights [(dy * 3 + dx) * 3 + c][Cp], then scale and bias; padding 0 / 1 / 0
  for (size_t o = 0; o < Cp; ++o) pack[27 * Cp + o] = 1.f;
  for (int o = 0; o < C0; ++o) {
    for (int ch = 0; ch < 3; ++ch)
      for (int t = 0; t < 9; ++t) pack[(size_t)(t * 3 + ch) * Cp + o] = w[((size_t)o * 3 + ch) * 9 + t];
    pack[27 * Cp + o] = scale[o];
    pack[28 * Cp + o] = bias[o];
  }
  uint8_t* dclips = nullptr;
  float *dpack = nullptr, *dout = nullptr;
  char* dact = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dclips = ws.take<uint8_t>((size_t)B * S * S * 3); dpack = ws.take<float>(pack.size() * 4);
    dact = ws.take(rows * Cp * es); dout = ws.take<float>(rows * Cp * 4);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dclips, clips, (size_t)B * S * S * 3, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dpack, pack.data(), pack.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // pack is a host temporary in pageable memory
  if ((rc = mhip_launch_cliprn_stem(ctx, precision, dclips, B, S, swap_rb, CLIP_MEAN, CLIP_STD, dpack, dpack + 27 * Cp, dpack + 28 * Cp, dact, (int)Cp)))
    return rc;
  if ((rc = mhip_launch_convert_rows(ctx, precision, dact, dout, (int)rows, (int)Cp))) return rc;
  MHIP_HIP(ctx, hipMemcpy2DAsync(out, (size_t)C0 * 4, dout, Cp * 4, (size_t)C0 * 4, rows, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_avgpool_nhwc_host(mhip_ctx* ctx, int precision, const float* x, int B, int H, int W, int C, int k, float* out) {
  if (!ctx || !x || !out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (B < 1 || H < 1 || W < 1 || C < 1 || k < 1 || (long long)B * H * W * C > (1LL << 28))
    return mhip_fail(ctx, MHIP_EINVAL, "avgpool_nhwc: B=%d H=%d W=%d C=%d k=%d", B, H, W, C, k);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t es = precision == MHIP_PREC_F16 ? 2 : 4, n = (size_t)B * H * W * C, no = (size_t)B * (H / k) * (W / k) * C;
  char *din = nullptr, *dact = nullptr;
  float* dout = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) { din = ws.take(n * es); dact = ws.take((no + 8) * es); dout = ws.take<float>((no + 8) * 4); });
  if (rc) return rc;
  std::vector<char> xt(n * es);
  Arena::put(precision, xt.data(), x, n);
  MHIP_HIP(ctx, hipMemcpyAsync(din, xt.data(), xt.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // xt is a host temporary in pageable memory
  if ((rc = mhip_launch_avgpool_nhwc(ctx, precision, k, din, dact, B, H, W, C))) return rc;
  if ((rc = mhip_launch_convert_rows(ctx, precision, dact, dout, 1, (int)no))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(out, dout, no * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_cliprn_attnpool_host(mhip_ctx* ctx, int precision, const float* x, const float* pos, const float* wq, const float* bq,
                                         const float* wk, const float* bk, const float* wv, const float* bv, const float* wc,
                                         const float* bc, int B, int HW, int E, int P, float* emb_out) {
  if (!ctx || !x || !pos || !wq || !bq || !wk || !bk || !wv || !bv || !wc || !bc || !emb_out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (B < 1 || B > MAX_CLIPS || !mhip_cliprn_attnpool_ok(HW, E, P) || P > 65536)
    return mhip_fail(ctx, MHIP_EINVAL, "cliprn_attnpool: B=%d HW=%d (up to 256) E=%d (a multiple of 64 up to 4096) P=%d", B, HW, E, P);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t es = precision == MHIP_PREC_F16 ? 2 : 4, NT = (size_t)HW + 1, EE = (size_t)E * E, XN = (size_t)B * HW * E;
  char *dx = nullptr, *dwq = nullptr, *dwkv = nullptr, *dtok = nullptr, *dxq = nullptr;
  float *dpos = nullptr, *dqs = nullptr, *dqb = nullptr, *dkvb = nullptr, *dwc = nullptr, *dbc = nullptr, *dq = nullptr, *dkv = nullptr,
        *dao = nullptr, *demb = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dx = ws.take(XN * es); dwq = ws.take(EE * es); dwkv = ws.take(2 * EE * es); dtok = ws.take(B * NT * E * es); dxq = ws.take((size_t)B * E * es);
    dpos = ws.take<float>(NT * E * 4); dqs = ws.take<float>((size_t)E * 4); dqb = ws.take<float>((size_t)E * 4); dkvb = ws.take<float>((size_t)2 * E * 4);
    dwc = ws.take<float>((size_t)P * E * 4); dbc = ws.take<float>((size_t)P * 4); dq = ws.take<float>((size_t)B * E * 4);
    dkv = ws.take<float>(B * NT * 2 * E * 4); dao = ws.take<float>((size_t)B * E * 4); demb = ws.take<float>((size_t)B * P * 4);
  });
  if (rc) return rc;
  std::vector<char> xt(XN * es), wqt(EE * es), wkvt(2 * EE * es);
  std::vector<float> qs(E, 0.125f), qb(E), kvb(2 * (size_t)E);
  Arena::put(precision, xt.data(), x, XN);
  Arena::put(precision, wqt.data(), wq, EE);
  Arena::put(precision, wkvt.data(), wk, EE);
  Arena::put(precision, wkvt.data() + EE * es, wv, EE);
  for (int i = 0; i < E; ++i) { qb[i] = bq[i] * 0.125f; kvb[i] = bk[i]; kvb[E + i] = bv[i]; }
  MHIP_HIP(ctx, hipMemcpyAsync(dx, xt.data(), xt.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dwq, wqt.data(), wqt.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dwkv, wkvt.data(), wkvt.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dpos, pos, NT * E * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dqs, qs.data(), (size_t)E * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dqb, qb.data(), (size_t)E * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dkvb, kvb.data(), (size_t)2 * E * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dwc, wc, (size_t)P * E * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dbc, bc, (size_t)P * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the sources are host temporaries in pageable memory
  if ((rc = mhip_launch_cliprn_tokens(ctx, precision, dx, dpos, dtok, dxq, B, HW, E))) return rc;
  if ((rc = mhip_gemm(ctx, precision, dxq, dwq, B, E, E, dqs, dqb, dq, ACT_NONE, 1))) return rc;
  if ((rc = mhip_gemm(ctx, precision, dtok, dwkv, (long long)B * NT, 2 * E, E, nullptr, dkvb, dkv, ACT_NONE, 1))) return rc;
  if ((rc = mhip_launch_cliprn_attn1q(ctx, dq, dkv, dao, B, (int)NT, E))) return rc;
  if ((rc = mhip_launch_cliprn_cproj(ctx, dao, B, E, dwc, dbc, P, demb))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(emb_out, demb, (size_t)B * P * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}
