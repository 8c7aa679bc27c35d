// cliptext_api.hip — the CLIP text tower (text embeddings of OpenAIEmbeddings.get_embeddings without an image) behind the C ABI.
//
// Host-side counterpart of CLIPTextModelWithProjection.forward (transformers/models/clip/modeling_clip.py: CLIPTextEmbeddings,
// CLIPTextTransformer under the causal mask, final_layer_norm, the row of the end-of-text token, text_projection) — the same
// arithmetic as clip/model.py: CLIP.encode_text — as OpenAIEmbeddings.get_text_embedding drives it
// (marie/embeddings/openai/openai_embeddings.py:122-129,159-164).  One object = one weight arena + the launch sequence.
//
// Row layout: every sequence owns `npad` rows (a multiple of 8, the same for the whole call), the residual stream h is fp32, and
// every row of every sequence is computed: a padding token is an ordinary token that no earlier row can see, so no lengths reach
// the kernels.  The layers are the vision tower's (clip_encoder_layers) with causal attention; there is no pre-LayerNorm.  The
// token table stays fp32 in both precision modes: it is a gather of B * npad rows, not a GEMM operand.
#include <math.h>

#include "encoder_block.h"

struct mhip_cliptext {
  mhip_ctx* ctx = nullptr;
  int precision = MHIP_PREC_F16;
  mhip_cliptext_config cfg{};
  TensorStore store;
  Arena arena;
  bool ready = false;
  size_t esz() const { return precision == MHIP_PREC_F16 ? 2 : 4; }
  int max_npad() const { return (cfg.context + 7) / 8 * 8; }
};

namespace {

constexpr int MAX_TEXTS = 4096, MAX_CONTEXT = 128;

// the buffers of one call of B sequences (and n_pairs cosines)
struct TextRun {
  int *ids = nullptr, *eot = nullptr, *pair_a = nullptr, *pair_b = nullptr;
  float *h = nullptr, *emb = nullptr, *cos = nullptr;
  EncoderWs w;
};

void cliptext_carve(const mhip_cliptext* m, Carver& ws, int B, int npad, int n_pairs, TextRun* r) {
  const mhip_cliptext_config& c = m->cfg;
  const size_t D = c.dim, R = (size_t)B * npad;
  r->ids = ws.take<int>(R * 4);
  r->eot = ws.take<int>((size_t)B * 4);
  r->pair_a = n_pairs ? ws.take<int>((size_t)n_pairs * 4) : nullptr;
  r->pair_b = n_pairs ? ws.take<int>((size_t)n_pairs * 4) : nullptr;
  r->cos = n_pairs ? ws.take<float>((size_t)n_pairs * 4) : nullptr;
  r->h = ws.take<float>(R * D * 4);
  r->emb = ws.take<float>((size_t)B * c.proj_dim * 4);
  encoder_ws_carve(ws, R, D, c.ffn, 0, m->esz(), &r->w);
}

bool npad_ok(int npad, int max_npad) { return npad >= 8 && npad % 8 == 0 && npad <= max_npad; }

int cliptext_check_call(mhip_cliptext* m, const int32_t* ids, const int32_t* eot, int B, int npad) {
  mhip_ctx* ctx = m->ctx;
  if (!m->ready) return mhip_fail(ctx, MHIP_ESTATE, "cliptext: weights not finalized");
  if (!ids || !eot || B < 1 || B > MAX_TEXTS) return mhip_fail(ctx, MHIP_EINVAL, "cliptext: bad arguments (%d texts; 1 .. %d)", B, MAX_TEXTS);
  if (!npad_ok(npad, m->max_npad()))
    return mhip_fail(ctx, MHIP_EINVAL, "cliptext: %d rows a text (a multiple of 8 up to %d)", npad, m->max_npad());
  for (size_t e = 0; e < (size_t)B * npad; ++e)
    if (ids[e] < 0 || ids[e] >= m->cfg.vocab)
      return mhip_fail(ctx, MHIP_EINVAL, "cliptext: id %d at text %zu, position %zu is outside the vocabulary of %d", ids[e], e / npad, e % npad, m->cfg.vocab);
  for (int b = 0; b < B; ++b)
    if (eot[b] < 1 || eot[b] >= npad) return mhip_fail(ctx, MHIP_EINVAL, "cliptext: end-of-text row %d of text %d (1 .. %d)", eot[b], b, npad - 1);
  return MHIP_OK;
}

int cliptext_upload(mhip_cliptext* m, const int32_t* ids, const int32_t* eot, int B, int npad, const TextRun& run) {
  int rc = mhip_stage_h2d(m->ctx, run.ids, ids, (size_t)B * npad * 4);
  return rc ? rc : mhip_stage_h2d(m->ctx, run.eot, eot, (size_t)B * 4);
}

// ids / eot staged in run -> embeddings in run.emb.  taps (host, or null): h after the embedding kernel and after every layer,
// [depth + 1][B][npad][D]
int cliptext_forward(mhip_cliptext* m, int B, int npad, const TextRun& run, float* taps) {
  mhip_ctx* ctx = m->ctx;
  const mhip_cliptext_config& c = m->cfg;
  const int D = c.dim, prec = m->precision;
  const size_t es = m->esz(), R = (size_t)B * npad;
  const Arena& a = m->arena;
  const EncoderWs& w = run.w;
  int rc;
  if ((rc = encoder_ws_clear_slack(ctx, w, R, D, es))) return rc;
  if ((rc = mhip_launch_cliptext_embed(ctx, a.d<float>("tok"), a.d<float>("pos"), run.ids, run.h, B, npad, D))) return rc;
  auto tap = [&](int i) -> int {
    if (!taps) return MHIP_OK;
    MHIP_HIP(ctx, hipMemcpyAsync(taps + (size_t)i * R * D, run.h, R * D * 4, hipMemcpyDeviceToHost, ctx->stream));
    return MHIP_OK;
  };
  if ((rc = tap(0))) return rc;
  AttnCausalDesc cd;
  cd.a = encoder_attn_desc(w.qk, w.vt, w.ao, D, es, B, c.heads, npad, npad);
  if ((rc = clip_encoder_layers(ctx, prec, a, c.depth, D, c.ffn, c.ln_eps, R, run.h, w, cd, tap))) return rc;
  return mhip_launch_clipvis_head(ctx, run.h, B, npad, D, a.d<float>("ln_final_g"), a.d<float>("ln_final_b"), c.ln_eps, a.d<float>("proj_t"),
                                  c.proj_dim, run.emb, run.eot);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- lifecycle
extern "C" int mhip_cliptext_create(mhip_ctx* ctx, int precision, const mhip_cliptext_config* cfg, mhip_cliptext** out) {
  if (!ctx || !out || !cfg) return MHIP_EINVAL;
  *out = nullptr;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  const mhip_cliptext_config& c = *cfg;
  if (c.heads < 1 || c.dim % 64 || c.dim != c.heads * 64)
    return mhip_fail(ctx, MHIP_EINVAL, "cliptext: head dimension %d (dim %d, heads %d): the attention kernel has heads of 64", c.heads > 0 ? c.dim / c.heads : 0, c.dim, c.heads);
  if (c.dim > 1024 || c.depth < 1 || c.ffn < 64 || c.ffn % 64 || c.proj_dim < 1 || c.proj_dim > 65536)
    return mhip_fail(ctx, MHIP_EINVAL, "cliptext: unsupported width (dim %d up to 1024, depth %d, ffn %d a multiple of 64, proj_dim %d)", c.dim, c.depth, c.ffn, c.proj_dim);
  if (c.context < 2 || c.context > MAX_CONTEXT) return mhip_fail(ctx, MHIP_EINVAL, "cliptext: context length %d (2 .. %d: a sequence's keys are held in LDS)", c.context, MAX_CONTEXT);
  if (c.vocab < 2 || c.vocab > (1 << 24)) return mhip_fail(ctx, MHIP_EINVAL, "cliptext: vocabulary of %d", c.vocab);
  if (!(c.ln_eps > 0.f)) return mhip_fail(ctx, MHIP_EINVAL, "cliptext: ln_eps");
  mhip_cliptext* m = new mhip_cliptext();
  m->ctx = ctx;
  m->precision = precision;
  m->cfg = c;
  const size_t es = m->esz(), D = c.dim;
  Arena& a = m->arena;
  a.take("tok", (size_t)c.vocab * D * 4);
  a.take("pos", (size_t)m->max_npad() * D * 4);      // rows past the context (padding rows only) are zeros
  for (int i = 0; i < c.depth; ++i) encoder_block_take(a, i, D, c.ffn, es);
  a.take("ln_final_g", D * 4); a.take("ln_final_b", D * 4);
  a.take("proj_t", (size_t)c.proj_dim * D * 4);
  *out = m;
  return MHIP_OK;
}

extern "C" int mhip_cliptext_destroy(mhip_cliptext* m) {
  if (!m) return MHIP_OK;
  mhip_quiesce(m->ctx);
  m->arena.release();
  delete m;
  return MHIP_OK;
}

extern "C" int mhip_cliptext_set_tensor(mhip_cliptext* m, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!m || !key) return MHIP_EINVAL;
  std::string k(key);
  if (k != "token_embedding.weight" && k != "positional_embedding" && k != "text_projection" && k.rfind("transformer.resblocks.", 0) != 0 &&
      k.rfind("ln_final.", 0) != 0)
    return mhip_fail(m->ctx, MHIP_EINVAL, "unknown state_dict key %s", key);
  m->ready = false;
  return m->store.set(m->ctx, k, data, shape, ndim);
}

extern "C" int mhip_cliptext_alloc_arena(mhip_cliptext* m) {
  if (!m) return MHIP_EINVAL;
  int rc = m->arena.alloc(m->ctx);
  if (rc) return rc;
  m->ready = true;
  return MHIP_OK;
}

extern "C" int mhip_cliptext_arena(mhip_cliptext* m, void** dev, size_t* bytes) {
  if (!m) return MHIP_EINVAL;
  if (dev) *dev = m->arena.dev;
  if (bytes) *bytes = m->arena.bytes;
  return MHIP_OK;
}

extern "C" int mhip_cliptext_finalize(mhip_cliptext* m) {
  if (!m) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  const mhip_cliptext_config& c = m->cfg;
  const int D = c.dim, F = c.ffn, prec = m->precision, E = c.proj_dim;
  Arena& a = m->arena;
  const TensorStore& st = m->store;
  a.begin_fill();
  const HostTensor* tok = st.find(ctx, "token_embedding.weight", {c.vocab, D});
  const HostTensor* pos = st.find(ctx, "positional_embedding", {c.context, D});
  const HostTensor* g9 = st.find(ctx, "ln_final.weight", {D});
  const HostTensor* b9 = st.find(ctx, "ln_final.bias", {D});
  const HostTensor* pj = st.find(ctx, "text_projection", {D, E});
  if (!tok || !pos || !g9 || !b9 || !pj) return MHIP_ESTATE;
  memcpy(a.h("tok"), tok->data.data(), tok->numel() * 4);
  memcpy(a.h("pos"), pos->data.data(), pos->numel() * 4);
  memcpy(a.h("ln_final_g"), g9->data.data(), (size_t)D * 4); memcpy(a.h("ln_final_b"), b9->data.data(), (size_t)D * 4);
  float* pt = (float*)a.h("proj_t");
  for (int k = 0; k < D; ++k)
    for (int j = 0; j < E; ++j) pt[(size_t)j * D + k] = pj->data[(size_t)k * E + j];
  for (int i = 0; i < c.depth; ++i) {
    EncoderBlockWeights w;
    if (!clip_resblock_weights(ctx, st, "transformer.resblocks.", i, D, F, &w)) return MHIP_ESTATE;
    encoder_block_fill(a, prec, i, D, F, w);
  }
  int rc = a.upload(ctx);
  if (rc) return rc;
  m->ready = true;
  m->store.t.clear();
  return MHIP_OK;
}

extern "C" size_t mhip_cliptext_workspace_bytes(mhip_cliptext* m, int B, int npad) {
  if (!m || B < 1 || B > MAX_TEXTS || !npad_ok(npad, m->max_npad())) return 0;
  TextRun run;
  return mhip_layout_bytes([&](Carver& ws) { cliptext_carve(m, ws, B, npad, 0, &run); });
}

// ---------------------------------------------------------------------------------------------------- forward
extern "C" int mhip_cliptext_embed_host(mhip_cliptext* m, const int32_t* ids, const int32_t* eot, int B, int npad, float* emb_out) {
  if (!m || !emb_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = cliptext_check_call(m, ids, eot, B, npad);
  if (rc) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  TextRun run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { cliptext_carve(m, ws, B, npad, 0, &run); }))) return rc;
  if ((rc = cliptext_upload(m, ids, eot, B, npad, run))) return rc;
  if ((rc = cliptext_forward(m, B, npad, run, nullptr))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(emb_out, run.emb, (size_t)B * m->cfg.proj_dim * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_cliptext_embed_pairs_host(mhip_cliptext* m, const int32_t* ids, const int32_t* eot, int B, int npad,
                                              const int32_t* pair_a, const int32_t* pair_b, int n_pairs, float* cos_out, float* emb_out) {
  if (!m || !pair_a || !pair_b || !cos_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = cliptext_check_call(m, ids, eot, B, npad);
  if (rc) return rc;
  if (n_pairs < 1 || n_pairs > (1 << 24)) return mhip_fail(ctx, MHIP_EINVAL, "cliptext: %d pairs", n_pairs);
  for (int p = 0; p < n_pairs; ++p)
    if (pair_a[p] < 0 || pair_a[p] >= B || pair_b[p] < 0 || pair_b[p] >= B)
      return mhip_fail(ctx, MHIP_EINVAL, "cliptext: pair %d names texts %d and %d of %d", p, pair_a[p], pair_b[p], B);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  TextRun run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { cliptext_carve(m, ws, B, npad, n_pairs, &run); }))) return rc;
  if ((rc = cliptext_upload(m, ids, eot, B, npad, run))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.pair_a, pair_a, (size_t)n_pairs * 4))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.pair_b, pair_b, (size_t)n_pairs * 4))) return rc;
  if ((rc = cliptext_forward(m, B, npad, run, nullptr))) return rc;
  if ((rc = mhip_launch_pair_cosine(ctx, run.emb, m->cfg.proj_dim, run.pair_a, run.pair_b, n_pairs, run.cos))) return rc;
  if (emb_out) MHIP_HIP(ctx, hipMemcpyAsync(emb_out, run.emb, (size_t)B * m->cfg.proj_dim * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(cos_out, run.cos, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_cliptext_debug_taps_host(mhip_cliptext* m, const int32_t* ids, const int32_t* eot, int B, int npad, float* taps_out,
                                             float* emb_out) {
  if (!m || !taps_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = cliptext_check_call(m, ids, eot, B, npad);
  if (rc) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  TextRun run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { cliptext_carve(m, ws, B, npad, 0, &run); }))) return rc;
  if ((rc = cliptext_upload(m, ids, eot, B, npad, run))) return rc;
  if ((rc = cliptext_forward(m, B, npad, run, taps_out))) return rc;
  if (emb_out) MHIP_HIP(ctx, hipMemcpyAsync(emb_out, run.emb, (size_t)B * m->cfg.proj_dim * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

// ---------------------------------------------------------------------------------------------------- the kernels alone
extern "C" int mhip_cliptext_embed_rows_host(mhip_ctx* ctx, const float* table, const float* pos, const int32_t* ids, int B, int npad,
                                             int vocab, int D, float* h_out) {
  if (!ctx || !table || !pos || !ids || !h_out) return MHIP_EINVAL;
  if (B < 1 || B > MAX_TEXTS || !npad_ok(npad, MAX_CONTEXT) || vocab < 1 || vocab > (1 << 24) || D < 64 || D % 64 || D > 1024)
    return mhip_fail(ctx, MHIP_EINVAL, "cliptext_embed: B=%d npad=%d vocab=%d D=%d", B, npad, vocab, D);
  const size_t R = (size_t)B * npad;
  for (size_t e = 0; e < R; ++e)
    if (ids[e] < 0 || ids[e] >= vocab) return mhip_fail(ctx, MHIP_EINVAL, "cliptext_embed: id %d outside the vocabulary of %d", ids[e], vocab);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  float *dt = nullptr, *dp = nullptr, *dh = nullptr;
  int* di = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dt = ws.take<float>((size_t)vocab * D * 4); dp = ws.take<float>((size_t)npad * D * 4); di = ws.take<int>(R * 4);
    dh = ws.take<float>(R * D * 4);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dt, table, (size_t)vocab * D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dp, pos, (size_t)npad * D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(di, ids, R * 4, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_launch_cliptext_embed(ctx, dt, dp, di, dh, B, npad, D))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(h_out, dh, R * D * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_cliptext_attention_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v, int B, int heads,
                                            int npad, float* out) {
  if (!ctx || !q || !k || !v || !out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (B < 1 || B > MAX_TEXTS || heads < 1 || heads > 16 || !npad_ok(npad, MAX_CONTEXT))
    return mhip_fail(ctx, MHIP_EINVAL, "cliptext_attention: B=%d heads=%d npad=%d", B, heads, npad);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  return encoder_attention_host(ctx, precision, q, k, v, B, heads, 64, npad, out, [](Carver&) {},
                                [&](const AttnDesc& ad) { return mhip_launch_attention_causal(ctx, precision, ad); });
}

extern "C" int mhip_cliptext_head_host(mhip_ctx* ctx, const float* h, int B, int npad, int D, const float* g, const float* b, float eps,
                                       const float* proj, int E, const int32_t* row_of, float* emb_out) {
  if (!ctx || !h || !g || !b || !proj || !row_of || !emb_out) return MHIP_EINVAL;
  if (B < 1 || B > MAX_TEXTS || npad < 1 || npad > 65536 || D < 64 || D % 64 || D > 1024 || E < 1 || E > 65536)
    return mhip_fail(ctx, MHIP_EINVAL, "cliptext_head: B=%d npad=%d D=%d E=%d", B, npad, D, E);
  for (int i = 0; i < B; ++i)
    if (row_of[i] < 0 || row_of[i] >= npad) return mhip_fail(ctx, MHIP_EINVAL, "cliptext_head: row %d of block %d (0 .. %d)", row_of[i], i, npad - 1);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t HN = (size_t)B * npad * D;
  float *dh = nullptr, *dg = nullptr, *db = nullptr, *dpt = nullptr, *de = nullptr;
  int* dr = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dh = ws.take<float>(HN * 4); dg = ws.take<float>((size_t)D * 4); db = ws.take<float>((size_t)D * 4);
    dpt = ws.take<float>((size_t)E * D * 4); de = ws.take<float>((size_t)B * E * 4); dr = ws.take<int>((size_t)B * 4);
  });
  if (rc) return rc;
  std::vector<float> pt((size_t)E * D);      // [D][E] as the checkpoint holds it -> [E][D]
  for (int k = 0; k < D; ++k)
    for (int j = 0; j < E; ++j) pt[(size_t)j * D + k] = proj[(size_t)k * E + j];
  MHIP_HIP(ctx, hipMemcpyAsync(dh, h, HN * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dg, g, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(db, b, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dr, row_of, (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dpt, pt.data(), pt.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // pt is a host temporary in pageable memory
  if ((rc = mhip_launch_clipvis_head(ctx, dh, B, npad, D, dg, db, eps, dpt, E, de, dr))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(emb_out, de, (size_t)B * E * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}
