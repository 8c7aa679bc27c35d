// clip_api.hip — the CLIP vision tower (image embeddings of the template matcher's snippet score) behind the C ABI.
//
// Host-side counterpart of CLIPVisionModelWithProjection.forward (transformers/models/clip/modeling_clip.py:
// CLIPVisionEmbeddings, CLIPVisionTransformer, CLIPEncoderLayer, visual_projection) — the same arithmetic as
// clip/model.py: VisionTransformer.forward behind CLIP.encode_image — as OpenAIEmbeddings.get_single_image_embedding drives it
// (marie/embeddings/openai/openai_embeddings.py:146-157), and of the cosine VQNNFTemplateMatcher.score takes of two embeddings
// (marie/components/template_matching/vqnnf_template_matching.py:335-347).  One object = one weight arena + the launch sequence.
//
// Row layout: every clip owns `npad` rows (class + patches rounded up to 8), the residual stream h is fp32.  A pre-LN layer is
//   ht = LN1(h)   q|k = ht Wqk^T + b   V^T = Wv ht^T          (the value bias moves into the output projection: soft-max rows sum to 1)
//   ao = attention(q, k, V^T)          h += ao Wo^T + (bo + Wo bv)
//   ht = LN2(h)   hid = quick_gelu(ht W1^T + b1)              h += hid W2^T + b2
#include <math.h>

#include "encoder_block.h"

struct mhip_clipvis {
  mhip_ctx* ctx = nullptr;
  int precision = MHIP_PREC_F16;
  mhip_clipvis_config cfg{};
  TensorStore store;
  Arena arena;
  bool ready = false;
  size_t esz() const { return precision == MHIP_PREC_F16 ? 2 : 4; }
  int grid() const { return cfg.image_size / cfg.patch; }
  int n_tok() const { return grid() * grid() + 1; }
  int npad() const { return (n_tok() + 7) / 8 * 8; }
};

namespace {

// the image processor's Normalize (OPENAI_CLIP_MEAN / OPENAI_CLIP_STD), RGB
const float CLIP_MEAN[3] = {0.48145466f, 0.4578275f, 0.40821073f};
const float CLIP_STD[3] = {0.26862954f, 0.26130258f, 0.27577711f};
constexpr int MAX_CLIPS = 4096;

// the buffers of one call of B clips (and n_pairs cosines)
struct ClipRun {
  uint8_t* clips = nullptr;
  int *pair_a = nullptr, *pair_b = nullptr;
  float *pe = nullptr, *h = nullptr, *emb = nullptr, *cos = nullptr;
  EncoderWs w;      // w.hid is also the patch matrix (B * patches rows, fewer than R)
};

void clipvis_carve(const mhip_clipvis* m, Carver& ws, int B, int n_pairs, ClipRun* r) {
  const mhip_clipvis_config& c = m->cfg;
  const size_t es = m->esz(), D = c.dim, R = (size_t)B * m->npad(), S = c.image_size, NPAT = m->n_tok() - 1, K0 = 3 * c.patch * c.patch;
  r->clips = ws.take<uint8_t>((size_t)B * S * S * 3);
  r->pair_a = n_pairs ? ws.take<int>((size_t)n_pairs * 4) : nullptr;
  r->pair_b = n_pairs ? ws.take<int>((size_t)n_pairs * 4) : nullptr;
  r->cos = n_pairs ? ws.take<float>((size_t)n_pairs * 4) : nullptr;
  r->pe = ws.take<float>((size_t)B * NPAT * D * 4);
  r->h = ws.take<float>(R * D * 4);
  r->emb = ws.take<float>((size_t)B * c.proj_dim * 4);
  encoder_ws_carve(ws, R, D, c.ffn, K0, es, &r->w);
}

// clips staged in run.clips -> embeddings in run.emb.  taps (host, or null): h after the embedding kernel and after every layer,
// [depth + 1][B][n_tok][D]
int clipvis_forward(mhip_clipvis* m, int B, int swap_rb, const ClipRun& run, float* taps) {
  mhip_ctx* ctx = m->ctx;
  const mhip_clipvis_config& c = m->cfg;
  const int D = c.dim, F = c.ffn, prec = m->precision, NP = m->npad(), NT = m->n_tok(), P = c.patch, S = c.image_size;
  const size_t es = m->esz(), R = (size_t)B * NP;
  const Arena& a = m->arena;
  const EncoderWs& w = run.w;
  int rc;
  if ((rc = encoder_ws_clear_slack(ctx, w, R, D, es))) return rc;
  // the fp32 attention writes the token rows only: the padding rows of ao start as zeros
  MHIP_HIP(ctx, hipMemsetAsync(w.ao, 0, R * D * es, ctx->stream));
  const int K0 = 3 * P * P, np = NT - 1;
  if ((rc = mhip_launch_clipvis_patchify(ctx, prec, run.clips, B, S, P, swap_rb, CLIP_MEAN, CLIP_STD, w.hid, K0))) return rc;
  {
    ConvDesc cd;      // the patch convolution has no bias
    cd.in = w.hid; cd.w = a.d("pe_w"); cd.out = run.pe;
    cd.B = 1; cd.H = 1; cd.W = B * np; cd.Cin = K0; cd.N = D; cd.out_f32 = 1;
    if ((rc = mhip_launch_conv_igemm(ctx, prec, cd))) return rc;
  }
  if ((rc = mhip_launch_clipvis_embed(ctx, run.pe, a.d<float>("cls"), a.d<float>("pos"), a.d<float>("ln_pre_g"), a.d<float>("ln_pre_b"),
                                      run.h, B, NP, NT, D, c.ln_eps)))
    return rc;
  const size_t tap_bytes = (size_t)NT * D * 4;
  auto tap = [&](int i) -> int {
    if (!taps) return MHIP_OK;
    MHIP_HIP(ctx, hipMemcpy2DAsync(taps + (size_t)i * B * NT * D, tap_bytes, run.h, (size_t)NP * D * 4, tap_bytes, B, hipMemcpyDeviceToHost, ctx->stream));
    return MHIP_OK;
  };
  if ((rc = tap(0))) return rc;
  const AttnDesc ad = encoder_attn_desc(w.qk, w.vt, w.ao, D, es, B, c.heads, NP, NT);
  if ((rc = clip_encoder_layers(ctx, prec, a, c.depth, D, F, c.ln_eps, R, run.h, w, ad, tap))) return rc;
  return mhip_launch_clipvis_head(ctx, run.h, B, NP, D, a.d<float>("ln_post_g"), a.d<float>("ln_post_b"), c.ln_eps, a.d<float>("proj_t"),
                                  c.proj_dim, run.emb);
}

int clipvis_check_call(mhip_clipvis* m, const uint8_t* clips, int B) {
  if (!m->ready) return mhip_fail(m->ctx, MHIP_ESTATE, "clipvis: weights not finalized");
  if (!clips || B < 1 || B > MAX_CLIPS) return mhip_fail(m->ctx, MHIP_EINVAL, "clipvis: bad arguments (%d clips; 1 .. %d)", B, MAX_CLIPS);
  return MHIP_OK;
}

int clipvis_upload(mhip_clipvis* m, const uint8_t* clips_host, int B, const ClipRun& run) {
  const size_t S = m->cfg.image_size;
  MHIP_HIP(m->ctx, hipMemcpyAsync(run.clips, clips_host, (size_t)B * S * S * 3, hipMemcpyHostToDevice, m->ctx->stream));
  return MHIP_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- lifecycle
extern "C" int mhip_clipvis_create(mhip_ctx* ctx, int precision, const mhip_clipvis_config* cfg, mhip_clipvis** out) {
  if (!ctx || !out || !cfg) return MHIP_EINVAL;
  *out = nullptr;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  const mhip_clipvis_config& c = *cfg;
  if (c.heads < 1 || c.dim != c.heads * 64)
    return mhip_fail(ctx, MHIP_EINVAL, "clipvis: head dimension %d (dim %d, heads %d): the attention kernel has heads of 64", c.heads > 0 ? c.dim / c.heads : 0, c.dim, c.heads);
  if (c.dim > 1024 || c.depth < 1 || c.ffn < 64 || c.ffn % 64 || c.proj_dim < 1 || c.proj_dim > 65536)
    return mhip_fail(ctx, MHIP_EINVAL, "clipvis: unsupported width (dim %d up to 1024, depth %d, ffn %d a multiple of 64, proj_dim %d)", c.dim, c.depth, c.ffn, c.proj_dim);
  if (c.patch < 8 || c.patch % 8 || c.image_size < 2 * c.patch || c.image_size % c.patch || c.image_size > 4096)
    return mhip_fail(ctx, MHIP_EINVAL, "clipvis: unsupported image geometry (image %d, patch %d: a patch a multiple of 8 that divides the image)", c.image_size, c.patch);
  if (!(c.ln_eps > 0.f)) return mhip_fail(ctx, MHIP_EINVAL, "clipvis: ln_eps");
  mhip_clipvis* m = new mhip_clipvis();
  m->ctx = ctx;
  m->precision = precision;
  m->cfg = c;
  const size_t es = m->esz(), D = c.dim, F = c.ffn, K0 = 3 * (size_t)c.patch * c.patch;
  Arena& a = m->arena;
  a.take("pe_w", D * K0 * es);
  a.take("cls", D * 4);
  a.take("pos", (size_t)m->n_tok() * D * 4);
  a.take("ln_pre_g", D * 4); a.take("ln_pre_b", D * 4);
  for (int i = 0; i < c.depth; ++i) encoder_block_take(a, i, D, F, es);
  a.take("ln_post_g", D * 4); a.take("ln_post_b", D * 4);
  a.take("proj_t", (size_t)c.proj_dim * D * 4);
  *out = m;
  return MHIP_OK;
}

extern "C" int mhip_clipvis_destroy(mhip_clipvis* m) {
  if (!m) return MHIP_OK;
  mhip_quiesce(m->ctx);
  m->arena.release();
  delete m;
  return MHIP_OK;
}

extern "C" int mhip_clipvis_set_tensor(mhip_clipvis* m, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!m || !key) return MHIP_EINVAL;
  std::string k(key);
  if (k.rfind("visual.", 0) != 0) return mhip_fail(m->ctx, MHIP_EINVAL, "unknown state_dict key %s", key);
  m->ready = false;
  return m->store.set(m->ctx, k, data, shape, ndim);
}

extern "C" int mhip_clipvis_alloc_arena(mhip_clipvis* m) {
  if (!m) return MHIP_EINVAL;
  int rc = m->arena.alloc(m->ctx);
  if (rc) return rc;
  m->ready = true;
  return MHIP_OK;
}

extern "C" int mhip_clipvis_arena(mhip_clipvis* m, void** dev, size_t* bytes) {
  if (!m) return MHIP_EINVAL;
  if (dev) *dev = m->arena.dev;
  if (bytes) *bytes = m->arena.bytes;
  return MHIP_OK;
}

extern "C" int mhip_clipvis_finalize(mhip_clipvis* m) {
  if (!m) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  const mhip_clipvis_config& c = m->cfg;
  const int D = c.dim, F = c.ffn, prec = m->precision, NT = m->n_tok(), E = c.proj_dim, P = c.patch;
  Arena& a = m->arena;
  const TensorStore& st = m->store;
  a.begin_fill();
  const HostTensor* pw = st.find(ctx, "visual.conv1.weight", {D, 3, P, P});
  const HostTensor* cls = st.find(ctx, "visual.class_embedding", {D});
  const HostTensor* pos = st.find(ctx, "visual.positional_embedding", {NT, D});
  const HostTensor* g0 = st.find(ctx, "visual.ln_pre.weight", {D});
  const HostTensor* b0 = st.find(ctx, "visual.ln_pre.bias", {D});
  const HostTensor* g9 = st.find(ctx, "visual.ln_post.weight", {D});
  const HostTensor* b9 = st.find(ctx, "visual.ln_post.bias", {D});
  const HostTensor* pj = st.find(ctx, "visual.proj", {D, E});
  if (!pw || !cls || !pos || !g0 || !b0 || !g9 || !b9 || !pj) return MHIP_ESTATE;
  Arena::put(prec, a.h("pe_w"), pw->data.data(), pw->numel());
  memcpy(a.h("cls"), cls->data.data(), (size_t)D * 4);
  memcpy(a.h("pos"), pos->data.data(), pos->numel() * 4);
  memcpy(a.h("ln_pre_g"), g0->data.data(), (size_t)D * 4); memcpy(a.h("ln_pre_b"), b0->data.data(), (size_t)D * 4);
  memcpy(a.h("ln_post_g"), g9->data.data(), (size_t)D * 4); memcpy(a.h("ln_post_b"), b9->data.data(), (size_t)D * 4);
  float* pt = (float*)a.h("proj_t");
  for (int k = 0; k < D; ++k)
    for (int j = 0; j < E; ++j) pt[(size_t)j * D + k] = pj->data[(size_t)k * E + j];
  for (int i = 0; i < c.depth; ++i) {
    EncoderBlockWeights w;
    if (!clip_resblock_weights(ctx, st, "visual.transformer.resblocks.", i, D, F, &w)) return MHIP_ESTATE;
    encoder_block_fill(a, prec, i, D, F, w);
  }
  int rc = a.upload(ctx);
  if (rc) return rc;
  m->ready = true;
  m->store.t.clear();
  return MHIP_OK;
}

extern "C" size_t mhip_clipvis_workspace_bytes(mhip_clipvis* m, int B) {
  if (!m || B < 1 || B > MAX_CLIPS) return 0;
  ClipRun run;
  return mhip_layout_bytes([&](Carver& ws) { clipvis_carve(m, ws, B, 0, &run); });
}

// ---------------------------------------------------------------------------------------------------- forward
extern "C" int mhip_clipvis_embed_host(mhip_clipvis* m, const uint8_t* clips_host, int B, int swap_rb, float* emb_out) {
  if (!m || !emb_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = clipvis_check_call(m, clips_host, B);
  if (rc) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  ClipRun run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { clipvis_carve(m, ws, B, 0, &run); }))) return rc;
  if ((rc = clipvis_upload(m, clips_host, B, run))) return rc;
  if ((rc = clipvis_forward(m, B, swap_rb, run, nullptr))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(emb_out, run.emb, (size_t)B * m->cfg.proj_dim * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_clipvis_embed_pairs_host(mhip_clipvis* m, const uint8_t* clips_host, int n_clips, const int32_t* pair_a,
                                             const int32_t* pair_b, int n_pairs, float* emb_out, float* cos_out) {
  if (!m || !pair_a || !pair_b || !cos_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = clipvis_check_call(m, clips_host, n_clips);
  if (rc) return rc;
  if (n_pairs < 1 || n_pairs > (1 << 24)) return mhip_fail(ctx, MHIP_EINVAL, "clipvis: %d pairs", n_pairs);
  for (int p = 0; p < n_pairs; ++p)
    if (pair_a[p] < 0 || pair_a[p] >= n_clips || pair_b[p] < 0 || pair_b[p] >= n_clips)
      return mhip_fail(ctx, MHIP_EINVAL, "clipvis: pair %d names clips %d and %d of %d", p, pair_a[p], pair_b[p], n_clips);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  ClipRun run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { clipvis_carve(m, ws, n_clips, n_pairs, &run); }))) return rc;
  if ((rc = clipvis_upload(m, clips_host, n_clips, run))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.pair_a, pair_a, (size_t)n_pairs * 4))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.pair_b, pair_b, (size_t)n_pairs * 4))) return rc;
  if ((rc = clipvis_forward(m, n_clips, 1, run, nullptr))) return rc;      // the matcher's clips are BGR
  if ((rc = mhip_launch_pair_cosine(ctx, run.emb, m->cfg.proj_dim, run.pair_a, run.pair_b, n_pairs, run.cos))) return rc;
  if (emb_out) MHIP_HIP(ctx, hipMemcpyAsync(emb_out, run.emb, (size_t)n_clips * m->cfg.proj_dim * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(cos_out, run.cos, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_clipvis_debug_taps_host(mhip_clipvis* m, const uint8_t* clips_host, int B, int swap_rb, float* taps_out,
                                            float* emb_out) {
  if (!m || !taps_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = clipvis_check_call(m, clips_host, B);
  if (rc) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  ClipRun run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { clipvis_carve(m, ws, B, 0, &run); }))) return rc;
  if ((rc = clipvis_upload(m, clips_host, B, run))) return rc;
  if ((rc = clipvis_forward(m, B, swap_rb, run, taps_out))) return rc;
  if (emb_out) MHIP_HIP(ctx, hipMemcpyAsync(emb_out, run.emb, (size_t)B * m->cfg.proj_dim * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

// ---------------------------------------------------------------------------------------------------- the kernels alone
extern "C" int mhip_clipvis_quick_gelu_host(mhip_ctx* ctx, int precision, const float* x, int n, float* out) {
  if (!ctx || !x || !out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (n < 1 || n > (1 << 26) || n % 8) return mhip_fail(ctx, MHIP_EINVAL, "quick_gelu: n=%d (a multiple of 8 up to 2^26)", n);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t es = precision == MHIP_PREC_F16 ? 2 : 4;
  char* dx = nullptr;
  float* dout = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) { dx = ws.take((size_t)n * es); dout = ws.take<float>((size_t)n * 4); });
  if (rc) return rc;
  std::vector<char> xt((size_t)n * es);
  Arena::put(precision, xt.data(), x, n);
  MHIP_HIP(ctx, hipMemcpyAsync(dx, xt.data(), xt.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the source is a host temporary in pageable memory
  if ((rc = mhip_launch_quick_gelu(ctx, precision, dx, n))) return rc;
  if ((rc = mhip_launch_convert_rows(ctx, precision, dx, dout, 1, n))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_clipvis_embed_rows_host(mhip_ctx* ctx, const float* patches, const float* cls, const float* pos, const float* g,
                                            const float* b, int B, int n_tok, int D, float eps, float* h_out) {
  if (!ctx || !patches || !cls || !pos || !g || !b || !h_out) return MHIP_EINVAL;
  if (B < 1 || B > MAX_CLIPS || n_tok < 2 || n_tok > 65536 || D < 64 || D % 64 || D > 1024)
    return mhip_fail(ctx, MHIP_EINVAL, "clipvis_embed: B=%d tokens=%d D=%d", B, n_tok, D);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npad = ((size_t)n_tok + 7) / 8 * 8, NPD = (size_t)B * (n_tok - 1) * D;
  float *dp = nullptr, *dc = nullptr, *dpos = nullptr, *dg = nullptr, *db = nullptr, *dh = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dp = ws.take<float>(NPD * 4); dc = ws.take<float>((size_t)D * 4); dpos = ws.take<float>((size_t)n_tok * D * 4);
    dg = ws.take<float>((size_t)D * 4); db = ws.take<float>((size_t)D * 4); dh = ws.take<float>((size_t)B * npad * D * 4);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dp, patches, NPD * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dc, cls, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dpos, pos, (size_t)n_tok * D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dg, g, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(db, b, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_launch_clipvis_embed(ctx, dp, dc, dpos, dg, db, dh, B, (int)npad, n_tok, D, eps))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(h_out, dh, (size_t)B * npad * D * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_clipvis_head_host(mhip_ctx* ctx, const float* h, int B, int npad, int D, const float* g, const float* b, float eps,
                                      const float* proj, int E, float* emb_out) {
  if (!ctx || !h || !g || !b || !proj || !emb_out) return MHIP_EINVAL;
  if (B < 1 || B > MAX_CLIPS || npad < 1 || npad > 65536 || D < 64 || D % 64 || D > 1024 || E < 1 || E > 65536)
    return mhip_fail(ctx, MHIP_EINVAL, "clipvis_head: B=%d npad=%d D=%d E=%d", B, npad, D, E);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t HN = (size_t)B * npad * D;
  float *dh = nullptr, *dg = nullptr, *db = nullptr, *dpt = nullptr, *de = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dh = ws.take<float>(HN * 4); dg = ws.take<float>((size_t)D * 4); db = ws.take<float>((size_t)D * 4);
    dpt = ws.take<float>((size_t)E * D * 4); de = ws.take<float>((size_t)B * E * 4);
  });
  if (rc) return rc;
  std::vector<float> pt((size_t)E * D);      // [D][E] as the checkpoint holds it -> [E][D]
  for (int k = 0; k < D; ++k)
    for (int j = 0; j < E; ++j) pt[(size_t)j * D + k] = proj[(size_t)k * E + j];
  MHIP_HIP(ctx, hipMemcpyAsync(dh, h, HN * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dg, g, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(db, b, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dpt, pt.data(), pt.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // pt is a host temporary in pageable memory
  if ((rc = mhip_launch_clipvis_head(ctx, dh, B, npad, D, dg, db, eps, dpt, E, de))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(emb_out, de, (size_t)B * E * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_clipvis_pair_cosine_host(mhip_ctx* ctx, const float* emb, int n, int E, const int32_t* pair_a, const int32_t* pair_b,
                                             int n_pairs, float* cos_out) {
  if (!ctx || !emb || !pair_a || !pair_b || !cos_out) return MHIP_EINVAL;
  if (n < 1 || n > (1 << 20) || E < 1 || E > 65536 || n_pairs < 1 || n_pairs > (1 << 24))
    return mhip_fail(ctx, MHIP_EINVAL, "pair_cosine: n=%d E=%d pairs=%d", n, E, n_pairs);
  for (int p = 0; p < n_pairs; ++p)
    if (pair_a[p] < 0 || pair_a[p] >= n || pair_b[p] < 0 || pair_b[p] >= n)
      return mhip_fail(ctx, MHIP_EINVAL, "pair_cosine: pair %d names rows %d and %d of %d", p, pair_a[p], pair_b[p], n);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  float *de = nullptr, *dc = nullptr;
  int *da = nullptr, *db = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    de = ws.take<float>((size_t)n * E * 4); da = ws.take<int>((size_t)n_pairs * 4); db = ws.take<int>((size_t)n_pairs * 4);
    dc = ws.take<float>((size_t)n_pairs * 4);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(de, emb, (size_t)n * E * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(da, pair_a, (size_t)n_pairs * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(db, pair_b, (size_t)n_pairs * 4, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_launch_pair_cosine(ctx, de, E, da, db, n_pairs, dc))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(cos_out, dc, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}
