// trocr_api.hip — the TrOCR recognizer (image encoder + autoregressive text decoder + beam search) behind the C ABI.
//
// Host-side counterpart of TrOcrProcessor's model path (marie/document/trocr_ocr_processor.py:116-180,251-367):
//   preprocess_image: PIL bicubic resize of the fragment to 384 x 384, /255, (x - 0.5) / 0.5        (:116-125)
//   TrOCREncoder.forward -> AdaptedVisionTransformer.forward_features (trocr_models.py:508-524; deit.py:105-146)
//   TextRecognitionGenerator._generate (generator.py:11-374) over fairseq's TransformerDecoder
//   (trocr_models.py:137-147,180-186): beam 3 (trocr_ocr_processor.py:228), max_len = min(200, max_positions - 1),
//   cand_size = 2 * beam, length-normalised scores; the top hypothesis per fragment is returned.
// fairseq is third-party and absent from the reference tree: decoder layer, incremental state, BeamSearch.step and
// finalize_hypos follow fairseq's published v0.12 behaviour.
//
// MI355X shape of the problem: the encoder (577 tokens x 12 layers per fragment) is >= 85 % of the FLOPs and runs on
// the ViT MFMA path; a decoder step is GEMMs with M = fragments x beams rows plus two HBM-bound attentions.  The
// self-attention cache is never re-ordered: an ancestry table maps (hypothesis, past step) -> cache slot.
#include <math.h>

#include "vit_internal.h"

struct mhip_trocr {
  mhip_ctx* ctx = nullptr;
  int precision = MHIP_PREC_F16;
  mhip_trocr_config cfg{};
  mhip_vit* vit = nullptr;
  TensorStore store;
  Arena arena;
  bool ready = false;
  // grow-only staging of generate_fragments (resized crops + resize scratch): no hipMalloc in steady state
  DevBuf frag_crops, frag_scratch;
  bool absorb = false;       // encoder-attention with absorbed K / V projections (f16 mode)
  mhip_gate* decode_gate = nullptr;   // signalled where the decode phase of a generate call starts in the stream
  // "crops not finished yet" after every step, copied to pinned memory; the host reads it two steps late (never drains the stream)
  int* h_remaining = nullptr;
  hipEvent_t rem_ev[2] = {nullptr, nullptr};
  // encoder tokens of the crops encoded since mhip_trocr_encode_begin (the encoder runs per batch of fragments as the page
  // batches come out of the detector; the autoregressive decoder then runs once over all of them):
  // [enc_cap * npad + CROSS_ATTN_SLACK_ROWS][enc_dim] T (enc_store_bytes)
  DevBuf enc_store;
  int enc_cap = 0, enc_count = 0;
  size_t esz() const { return precision == MHIP_PREC_F16 ? 2 : 4; }
};

namespace {

const char* kEncPrefix = "encoder.deit.";
constexpr float DEC_LN_EPS = 1e-5f;

std::string lay(int l, const char* s) { return "L" + std::to_string(l) + "." + s; }

}  // namespace

extern "C" int mhip_trocr_default_config(int model, mhip_trocr_config* c) {
  if (!c || model < 0 || model > 1) return MHIP_EINVAL;
  // trocr_base (beit_base_patch16_384) / trocr_large (beit_large_patch16_384): trocr_models.py:423-447
  c->enc_dim = model ? 1024 : 768; c->enc_depth = model ? 24 : 12; c->enc_heads = model ? 16 : 12;
  c->dec_dim = 1024; c->dec_layers = 12; c->dec_heads = 16; c->dec_ffn = 4096;
  c->vocab = 50265;            // fairseq Dictionary over gpt2_with_mask.dict.txt (file not in the reference tree)
  c->max_positions = 512;
  c->beam = 3; c->max_len_b = 200; c->min_len = 1;
  c->pad = 1; c->eos = 2;
  c->embed_scale = 1.0f;       // RoBERTa arguments: no_scale_embedding
  c->img_size = 384;
  return MHIP_OK;
}

// the absorbed W_k of the encoder-attention (cross_attn.hip): out[h][d][j] = wk[h * 64 + j][d] * log2(e), f16
static void pack_ca_kt(const float* wk, int heads, int enc_dim, _Float16* out) {
  const float log2e = 1.4426950408889634f;
  for (int h = 0; h < heads; ++h)
    for (int d = 0; d < enc_dim; ++d)
      for (int j = 0; j < 64; ++j) out[((size_t)h * enc_dim + d) * 64 + j] = (_Float16)(wk[(size_t)(h * 64 + j) * enc_dim + d] * log2e);
}

static int trocr_max_len(const mhip_trocr_config& c) { return std::min(c.max_len_b, c.max_positions - 1); }

extern "C" int mhip_trocr_create(mhip_ctx* ctx, int precision, const mhip_trocr_config* cfg, mhip_trocr** out) {
  if (!ctx || !cfg || !out) return MHIP_EINVAL;
  *out = nullptr;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  const mhip_trocr_config& c = *cfg;
  if (c.dec_dim != c.dec_heads * 64 || c.dec_dim % 256 || c.dec_dim > 1024 || c.dec_ffn % 64 || c.dec_layers < 1 ||
      c.vocab < 8 || c.beam < 1 || c.beam > 4 || c.img_size % 16 || c.max_len_b < 1 || c.max_positions < 2 ||
      c.pad < 0 || c.eos < 0 || c.pad >= c.vocab || c.eos >= c.vocab)
    return mhip_fail(ctx, MHIP_EINVAL, "trocr: unsupported configuration");
  // the last step of a search attends over max_len + 1 keys of history: refuse here what would fail halfway through a search
  if (trocr_max_len(c) + 1 > DEC_ATTN_MAX_KEYS)
    return mhip_fail(ctx, MHIP_EINVAL, "trocr: max_len %d needs %d keys of self-attention history, decode attention runs at most %d",
                     trocr_max_len(c), trocr_max_len(c) + 1, DEC_ATTN_MAX_KEYS);
  // the generator's own assertion (generator.py:63): with min_len above it, eos is still masked at the forced last step and every
  // line would come back empty with score -inf
  if (c.min_len > trocr_max_len(c))
    return mhip_fail(ctx, MHIP_EINVAL, "trocr: min_len %d exceeds max_len %d (min of max_len_b and max_positions - 1)", c.min_len, trocr_max_len(c));
  mhip_vit_config vc{};
  vc.dim = c.enc_dim; vc.depth = c.enc_depth; vc.heads = c.enc_heads; vc.patch = 16;
  vc.pos_h = vc.pos_w = c.img_size / 16;
  vc.layer_scale = 0; vc.qkv_bias = 0; vc.final_norm = 1; vc.fpn = 0; vc.ln_eps = 1e-6f;
  mhip_vit* vit = nullptr;
  int rc = mhip_vit_create(ctx, precision, &vc, &vit);
  if (rc) return rc;
  mhip_trocr* m = new mhip_trocr();
  m->ctx = ctx; m->precision = precision; m->cfg = c; m->vit = vit;
  // f16 mode: encoder-attention over the encoder tokens themselves (cross_attn.hip); MARIE_HIP_NO_ABSORB=1 keeps the projected
  // K / V path (A/B measurements)
  m->absorb = precision == MHIP_PREC_F16 && mhip_cross_absorb_supported(c.enc_dim, c.beam, c.dec_heads) && !getenv("MARIE_HIP_NO_ABSORB");
  const size_t es = m->esz(), D = c.dec_dim, E = c.enc_dim, F = c.dec_ffn;
  Arena& a = m->arena;
  a.take("emb", (size_t)c.vocab * D * es);
  a.take("out_w", (size_t)c.vocab * D * es);
  a.take("pos", (size_t)(c.max_positions + c.pad + 1) * D * 4);
  a.take("lne_g", D * 4); a.take("lne_b", D * 4);
  for (int l = 0; l < c.dec_layers; ++l) {
    // the three self-attention input projections sit back to back — one [3 D][D] weight and one [3 D] bias for a single GEMM per
    // layer and step (q | k | v of a step are one row of the history, below)
    for (const char* n : {"sa_q", "sa_k", "sa_v"}) a.take(lay(l, n) + "_w", D * D * es);
    for (const char* n : {"sa_q", "sa_k", "sa_v"}) a.take(lay(l, n) + "_b", D * 4);
    for (const char* n : {"sa_o", "ca_q", "ca_o"}) { a.take(lay(l, n) + "_w", D * D * es); a.take(lay(l, n) + "_b", D * 4); }
    // absorbed encoder-attention: W_k lives only as ca_kt and b_k drops out of the soft-max — no ca_k slots in the arena
    for (const char* n : {"ca_k", "ca_v"}) {
      if (m->absorb && !strcmp(n, "ca_k")) continue;
      a.take(lay(l, n) + "_w", D * E * es); a.take(lay(l, n) + "_b", D * 4);
    }
    if (m->absorb) a.take(lay(l, "ca_kt"), D * E * 2);     // W_k per head, transposed, x log2(e): [heads][E][64] f16
    a.take(lay(l, "fc1_w"), F * D * es); a.take(lay(l, "fc1_b"), F * 4);
    a.take(lay(l, "fc2_w"), D * F * es); a.take(lay(l, "fc2_b"), D * 4);
    for (const char* n : {"sa_ln", "ca_ln", "fin_ln"}) { a.take(lay(l, n) + "_g", D * 4); a.take(lay(l, n) + "_b", D * 4); }
  }
  hipError_t he = hipHostMalloc((void**)&m->h_remaining, (size_t)(c.max_positions + 2) * sizeof(int));
  for (int i = 0; i < 2 && he == hipSuccess; ++i) he = hipEventCreateWithFlags(&m->rem_ev[i], hipEventDisableTiming);
  if (he != hipSuccess) {
    mhip_trocr_destroy(m);
    return mhip_fail(ctx, MHIP_EHIP, "trocr: pinned step counter: %s", hipGetErrorString(he));
  }
  *out = m;
  return MHIP_OK;
}

extern "C" int mhip_trocr_destroy(mhip_trocr* m) {
  if (!m) return MHIP_OK;
  mhip_quiesce(m->ctx);
  if (m->h_remaining) (void)hipHostFree(m->h_remaining);
  for (auto e : m->rem_ev)
    if (e) (void)hipEventDestroy(e);
  mhip_vit_destroy(m->vit);
  m->arena.release();
  m->frag_crops.release();
  m->frag_scratch.release();
  m->enc_store.release();
  delete m;
  return MHIP_OK;
}

extern "C" int mhip_trocr_set_tensor(mhip_trocr* m, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!m || !key) return MHIP_EINVAL;
  std::string k(key);
  if (k.rfind(kEncPrefix, 0) == 0) {
    const std::string sub = k.substr(strlen(kEncPrefix));
    if (sub.rfind("head.", 0) == 0 || sub.rfind("head_dist.", 0) == 0 || sub == "dist_token") return MHIP_OK;   // classifier heads: unused
    return mhip_vit_set_tensor(m->vit, sub.c_str(), data, shape, ndim);
  }
  if (k == "decoder.version" || k == "encoder.version" || k.find("_float_tensor") != std::string::npos) return MHIP_OK;
  if (k.rfind("decoder.", 0) != 0) return mhip_fail(m->ctx, MHIP_EINVAL, "unknown state_dict key %s", key);
  m->ready = false;
  return m->store.set(m->ctx, k, data, shape, ndim);
}

extern "C" int mhip_trocr_alloc_arena(mhip_trocr* m) {
  if (!m) return MHIP_EINVAL;
  int rc = m->arena.alloc(m->ctx);
  if (rc) return rc;
  if ((rc = mhip_vit_alloc_arena(m->vit))) return rc;
  m->ready = true;
  return MHIP_OK;
}

extern "C" int mhip_trocr_arena(mhip_trocr* m, int which, void** dev, size_t* bytes) {
  if (!m || which < 0 || which > 1) return MHIP_EINVAL;
  if (which == 0) return mhip_vit_arena(m->vit, dev, bytes);
  if (dev) *dev = m->arena.dev;
  if (bytes) *bytes = m->arena.bytes;
  return MHIP_OK;
}

extern "C" int mhip_trocr_finalize(mhip_trocr* m) {
  if (!m) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = mhip_vit_finalize(m->vit);
  if (rc) return rc;
  const mhip_trocr_config& c = m->cfg;
  const int prec = m->precision, D = c.dec_dim, E = c.enc_dim, F = c.dec_ffn;
  Arena& a = m->arena;
  const TensorStore& st = m->store;
  a.begin_fill();
  const HostTensor* emb = st.find(ctx, "decoder.embed_tokens.weight", {c.vocab, D});
  const HostTensor* pos = st.find(ctx, "decoder.embed_positions.weight", {c.max_positions + c.pad + 1, D});
  const HostTensor* lg = st.find(ctx, "decoder.layernorm_embedding.weight", {D});
  const HostTensor* lb = st.find(ctx, "decoder.layernorm_embedding.bias", {D});
  if (!emb || !pos || !lg || !lb) return MHIP_ESTATE;
  Arena::put(prec, a.h("emb"), emb->data.data(), emb->numel());
  if (st.has("decoder.output_projection.weight")) {
    const HostTensor* ow = st.find(ctx, "decoder.output_projection.weight", {c.vocab, D});
    if (!ow) return MHIP_ESTATE;
    Arena::put(prec, a.h("out_w"), ow->data.data(), ow->numel());
  } else {
    Arena::put(prec, a.h("out_w"), emb->data.data(), emb->numel());   // share_decoder_input_output_embed
  }
  memcpy(a.h("pos"), pos->data.data(), pos->numel() * 4);
  memcpy(a.h("lne_g"), lg->data.data(), D * 4);
  memcpy(a.h("lne_b"), lb->data.data(), D * 4);
  const float qscale = 0.125f;   // head_dim 64: MultiheadAttention scales q (bias included) by head_dim^-0.5
  for (int l = 0; l < c.dec_layers; ++l) {
    const std::string p = "decoder.layers." + std::to_string(l) + ".";
    struct Lin { const char* name; std::string key; int out, in; float scale; };
    const Lin lins[] = {{"sa_q", p + "self_attn.q_proj", D, D, qscale}, {"sa_k", p + "self_attn.k_proj", D, D, 1.f},
                        {"sa_v", p + "self_attn.v_proj", D, D, 1.f},    {"sa_o", p + "self_attn.out_proj", D, D, 1.f},
                        {"ca_q", p + "encoder_attn.q_proj", D, D, qscale}, {"ca_k", p + "encoder_attn.k_proj", D, E, 1.f},
                        {"ca_v", p + "encoder_attn.v_proj", D, E, 1.f}, {"ca_o", p + "encoder_attn.out_proj", D, D, 1.f},
                        {"fc1", p + "fc1", F, D, 1.f}, {"fc2", p + "fc2", D, F, 1.f}};
    for (const Lin& L : lins) {
      if (m->absorb && !strcmp(L.name, "ca_k")) continue;
      const HostTensor* w = st.find(ctx, L.key + ".weight", {L.out, L.in});
      const HostTensor* b = st.find(ctx, L.key + ".bias", {L.out});
      if (!w || !b) return MHIP_ESTATE;
      if (L.scale != 1.f) {
        std::vector<float> t(w->data);
        for (float& v : t) v *= L.scale;
        Arena::put(prec, a.h(lay(l, L.name) + "_w"), t.data(), t.size());
        float* bb = (float*)a.h(lay(l, L.name) + "_b");
        for (int i = 0; i < L.out; ++i) bb[i] = b->data[i] * L.scale;
      } else {
        Arena::put(prec, a.h(lay(l, L.name) + "_w"), w->data.data(), w->numel());
        memcpy(a.h(lay(l, L.name) + "_b"), b->data.data(), (size_t)L.out * 4);
      }
    }
    if (m->absorb) {
      const HostTensor* wk = st.find(ctx, p + "encoder_attn.k_proj.weight", {D, E});
      if (!wk) return MHIP_ESTATE;
      pack_ca_kt(wk->data.data(), c.dec_heads, E, (_Float16*)a.h(lay(l, "ca_kt")));
    }
    const std::pair<const char*, std::string> lns[] = {{"sa_ln", p + "self_attn_layer_norm"}, {"ca_ln", p + "encoder_attn_layer_norm"},
                                                       {"fin_ln", p + "final_layer_norm"}};
    for (const auto& ln : lns) {
      const HostTensor* g = st.find(ctx, ln.second + ".weight", {D});
      const HostTensor* b = st.find(ctx, ln.second + ".bias", {D});
      if (!g || !b) return MHIP_ESTATE;
      memcpy(a.h(lay(l, ln.first) + "_g"), g->data.data(), D * 4);
      memcpy(a.h(lay(l, ln.first) + "_b"), b->data.data(), D * 4);
    }
  }
  if ((rc = a.upload(ctx))) return rc;
  m->ready = true;
  m->store.t.clear();
  return MHIP_OK;
}

extern "C" int mhip_trocr_set_decode_gate(mhip_trocr* m, mhip_gate* gate) {
  if (!m) return MHIP_EINVAL;
  m->decode_gate = gate;
  return MHIP_OK;
}

extern "C" int mhip_trocr_max_len(const mhip_trocr_config* c) { return c ? trocr_max_len(*c) : MHIP_EINVAL; }

// the decoder's buffers, in layout order
struct TrocrDecodeBufs {
  char *ck = nullptr, *cv = nullptr;   // projected path: encoder keys / values of every decoder layer
  char *qt = nullptr, *ct = nullptr;   // absorbed path: absorbed queries / contexts
  char* hqkv;                          // self-attention history [layer][step][slot][q | k | v]
  float* x;
  char *xt, *qb, *ao, *hid;
  char* logits;                        // element type T: f16 logits in the f16 mode, fp32 in the parity mode
  int* anc[2];
  float* cand_scores;
  int *cand_tokens, *cand_beams;
  BeamState bs;                        // generator state
  int *out_tok, *out_len;              // device copies of the outputs
  float* out_score;
  float* step0_stage = nullptr;        // parity entries: step-0 logits in fp32
};

static void trocr_decode_carve(const mhip_trocr* m, Carver& ws, int n, const VitGeom& vg, bool step0_stage, TrocrDecodeBufs* b) {
  const mhip_trocr_config& c = m->cfg;
  const size_t es = m->esz(), D = c.dec_dim, M = (size_t)n * c.beam;
  const int ML = trocr_max_len(c), ldv = (c.vocab + 7) / 8 * 8, K2 = 2 * c.beam;
  if (m->absorb) {
    b->qt = ws.take(M * 16 * c.enc_dim * 2);
    b->ct = ws.take(M * 16 * c.enc_dim * 2);
  } else {
    const size_t cross = (size_t)c.dec_layers * n * vg.npad * D * es;
    b->ck = ws.take(cross);
    b->cv = ws.take(cross);
  }
  b->hqkv = ws.take((size_t)c.dec_layers * (ML + 1) * M * 3 * D * es);
  b->x = ws.take<float>(M * D * 4);
  b->xt = ws.take(M * D * es);
  b->qb = ws.take(M * D * es);
  b->ao = ws.take(M * D * es);
  b->hid = ws.take(M * c.dec_ffn * es);
  b->logits = ws.take(M * ldv * 4);
  for (int i = 0; i < 2; ++i) b->anc[i] = ws.take<int>(M * (ML + 2) * 4);
  b->cand_scores = ws.take<float>((size_t)n * K2 * 4);
  b->cand_tokens = ws.take<int>((size_t)n * K2 * 4);
  b->cand_beams = ws.take<int>((size_t)n * K2 * 4);
  mhip_beam_state_carve(ws, n, c.beam, ML, c.pad, c.eos, &b->bs);
  b->bs.cand_scores = b->cand_scores; b->bs.cand_tokens = b->cand_tokens; b->bs.cand_beams = b->cand_beams;
  b->out_tok = ws.take<int>((size_t)n * (ML + 1) * 4);
  b->out_len = ws.take<int>((size_t)n * 4);
  b->out_score = ws.take<float>((size_t)n * 4);
  if (step0_stage) b->step0_stage = ws.take<float>((size_t)c.vocab * 4);
}

// the layout of one generate call over n crops: encoder, the parity entries' staging on request, decoder
struct TrocrBufs {
  VitRun run;
  float* enc_stage = nullptr;
  TrocrDecodeBufs dec;
};

static void trocr_carve(const mhip_trocr* m, Carver& ws, int n, bool enc_stage, bool step0_stage, TrocrBufs* b) {
  VitGeom vg;
  vit_geometry(m->vit, m->cfg.img_size, m->cfg.img_size, &vg);
  vit_carve(m->vit, ws, n, vg, &b->run);
  if (enc_stage) b->enc_stage = ws.take<float>((size_t)vg.n_tok * m->cfg.enc_dim * 4);
  trocr_decode_carve(m, ws, n, vg, step0_stage, &b->dec);
}

extern "C" size_t mhip_trocr_workspace_bytes(mhip_trocr* m, int n) {
  if (!m || n < 1) return 0;
  TrocrBufs b;
  return mhip_layout_bytes([&](Carver& ws) { trocr_carve(m, ws, n, false, false, &b); });
}

// crops_dev: n images u8 [img][img][3].  tokens_out [n][max_len + 1] (the hypothesis without the leading eos, eos included,
// padded with `pad`), lengths_out [n], scores_out [n] (length-normalised log-probability of the best hypothesis).
struct TrocrTrace {          // host arrays [max_len + 1][n][2 * beam], filled for the steps that ran
  float* scores;
  int32_t* tokens;
  int32_t* beams;
  int steps;
};

static int trocr_decode(mhip_trocr* m, const TrocrDecodeBufs& b, const char* enc_tokens, const VitGeom& vg, int n,
                        int32_t* tokens_out, int32_t* lengths_out, float* scores_out, float* step0_logits_host, TrocrTrace* trace);

static int trocr_generate(mhip_trocr* m, const uint8_t* crops_dev, int n, int swap_rb, int32_t* tokens_out,
                          int32_t* lengths_out, float* scores_out, float* enc_tokens_host, float* step0_logits_host,
                          TrocrTrace* trace = nullptr) {
  mhip_ctx* ctx = m->ctx;
  if (!m->ready) return mhip_fail(ctx, MHIP_ESTATE, "trocr: weights not finalized");
  if (n < 1) return mhip_fail(ctx, MHIP_EINVAL, "trocr: empty batch");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const mhip_trocr_config& c = m->cfg;
  const int prec = m->precision, E = c.enc_dim;
  const size_t es = m->esz();
  TrocrBufs b;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) { trocr_carve(m, ws, n, enc_tokens_host, step0_logits_host, &b); });
  if (rc) return rc;
  // ---- encoder --------------------------------------------------------------------------------------------------
  if ((rc = vit_encode(m->vit, crops_dev, n, c.img_size, c.img_size, c.img_size, c.img_size, swap_rb, &b.run))) return rc;
  const VitGeom& vg = b.run.g;
  if (enc_tokens_host) {
    for (int i = 0; i < n; ++i) {
      if ((rc = mhip_launch_convert_rows(ctx, prec, b.run.tokens + (size_t)i * vg.npad * E * es, b.enc_stage, vg.n_tok, E))) return rc;
      MHIP_HIP(ctx, hipMemcpyAsync(enc_tokens_host + (size_t)i * vg.n_tok * E, b.enc_stage, (size_t)vg.n_tok * E * 4, hipMemcpyDeviceToHost, ctx->stream));
      MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  return trocr_decode(m, b.dec, b.run.tokens, vg, n, tokens_out, lengths_out, scores_out, step0_logits_host, trace);
}

// The autoregressive part (TextRecognitionGenerator._generate, generator.py:127-362) over the encoder tokens of n crops:
// enc_tokens T [n * vg.npad + CROSS_ATTN_SLACK_ROWS][enc_dim].
static int trocr_decode(mhip_trocr* m, const TrocrDecodeBufs& b, const char* enc_tokens, const VitGeom& vg, int n,
                        int32_t* tokens_out, int32_t* lengths_out, float* scores_out, float* step0_logits_host, TrocrTrace* trace) {
  mhip_ctx* ctx = m->ctx;
  const mhip_trocr_config& c = m->cfg;
  const int prec = m->precision, D = c.dec_dim, E = c.enc_dim, F = c.dec_ffn, beam = c.beam, L = c.dec_layers;
  const int K2 = 2 * beam, ML = trocr_max_len(c), M = n * beam;
  const size_t es = m->esz();
  const int ldv = (c.vocab + 7) / 8 * 8;
  const Arena& a = m->arena;
  int rc;
  // ---- encoder keys / values of every decoder layer (static over the steps) -----------------------------------------
  const size_t cross_l = (size_t)n * vg.npad * D * es;
  for (int l = 0; l < L && !m->absorb; ++l) {
    if ((rc = mhip_gemm(ctx, prec, enc_tokens, a.d(lay(l, "ca_k") + "_w"), (long long)n * vg.npad, D, E, nullptr, a.d<float>(lay(l, "ca_k") + "_b"), b.ck + l * cross_l, ACT_NONE, 0))) return rc;
    if ((rc = mhip_gemm(ctx, prec, enc_tokens, a.d(lay(l, "ca_v") + "_w"), (long long)n * vg.npad, D, E, nullptr, a.d<float>(lay(l, "ca_v") + "_b"), b.cv + l * cross_l, ACT_NONE, 0))) return rc;
  }
  // the MFMA-bound part of the call is enqueued; what follows is HBM- and latency-bound: whoever waits on the gate (the
  // detector of the next page batch) runs underneath it
  if (m->decode_gate && (rc = mhip_gate_signal(m->decode_gate, ctx))) return rc;
  // ---- decoder state ------------------------------------------------------------------------------------------------
  const size_t hist_s = (size_t)M * 3 * D * es;              // one step of one layer: rows of q | k | v
  const int anc_ld = ML + 2;
  // generator state (b.bs: TextRecognitionGenerator._generate without batch compaction, finished crops keep their rows), all in HBM
  if ((rc = mhip_launch_beam_init(ctx, b.bs, b.anc[0], anc_ld))) return rc;
  int cur = 0, tcur = 0;
  for (int step = 0; step <= ML; ++step) {
    if (step >= 2) {
      // the counter of two steps ago: the stream still holds step - 1 while this one is enqueued, so the device never waits for
      // the host; when every crop has finished, one step too many has been enqueued — finished crops ignore it
      MHIP_HIP(ctx, hipEventSynchronize(m->rem_ev[step & 1]));
      if (m->h_remaining[step - 2] == 0) break;
    }
    if (step > 0) {
      if ((rc = mhip_launch_ancestry(ctx, b.anc[cur], b.anc[cur ^ 1], b.bs.parent, M, anc_ld, step - 1))) return rc;
      cur ^= 1;
    }
    // LearnedPositionalEmbedding, incremental: position = padding_idx + (step + 1)
    const float* pos_row = a.d<float>("pos") + (size_t)(c.pad + step + 1) * D;
    if ((rc = mhip_launch_embed_step(ctx, prec, b.bs.last_tok, a.d("emb"), pos_row, c.embed_scale, a.d<float>("lne_g"), a.d<float>("lne_b"), b.x, b.xt, M, D, DEC_LN_EPS))) return rc;
    for (int l = 0; l < L; ++l) {
      char* hl = b.hqkv + ((size_t)l * (ML + 1)) * hist_s;
      // self-attention over the hypothesis' own history (post-LN residual block): q | k | v of this step in ONE GEMM (the three
      // weights are adjacent in the arena), written as one row of the history
      if ((rc = mhip_gemm(ctx, prec, b.xt, a.d(lay(l, "sa_q") + "_w"), M, 3 * D, D, nullptr, a.d<float>(lay(l, "sa_q") + "_b"), hl + (size_t)step * hist_s, ACT_NONE, 0))) return rc;
      DecAttnDesc sa;
      sa.q = hl + (size_t)step * hist_s; sa.k = hl + (size_t)D * es; sa.v = hl + (size_t)2 * D * es; sa.out = b.ao;
      sa.anc = b.anc[cur]; sa.anc_ld = anc_ld; sa.slots = M;
      sa.ldq = sa.ldk = 3 * D; sa.ldo = D; sa.heads = c.dec_heads; sa.groups = M; sa.nq = 1; sa.n_keys = step + 1;
      if ((rc = mhip_launch_decode_attention(ctx, prec, sa))) return rc;
      if ((rc = mhip_gemm(ctx, prec, b.ao, a.d(lay(l, "sa_o") + "_w"), M, D, D, nullptr, a.d<float>(lay(l, "sa_o") + "_b"), b.x, ACT_NONE, 1, b.x))) return rc;
      if ((rc = mhip_launch_layernorm2(ctx, prec, b.x, a.d<float>(lay(l, "sa_ln") + "_g"), a.d<float>(lay(l, "sa_ln") + "_b"), b.x, b.xt, M, D, DEC_LN_EPS))) return rc;
      // attention over the crop's encoder tokens (keys / values shared by its beams)
      if ((rc = mhip_gemm(ctx, prec, b.xt, a.d(lay(l, "ca_q") + "_w"), M, D, D, nullptr, a.d<float>(lay(l, "ca_q") + "_b"), b.qb, ACT_NONE, 0))) return rc;
      if (m->absorb) {
        CrossAbsorbDesc cd;
        cd.q = b.qb; cd.ldq = D; cd.E = enc_tokens; cd.kv_rows = vg.npad; cd.n_keys = vg.n_tok; cd.enc_dim = E;
        cd.wkt = a.d(lay(l, "ca_kt")); cd.wv = a.d(lay(l, "ca_v") + "_w"); cd.bv = a.d<float>(lay(l, "ca_v") + "_b");
        cd.qt = b.qt; cd.ct = b.ct; cd.ao = b.ao; cd.ldo = D; cd.crops = n; cd.beam = beam; cd.heads = c.dec_heads;
        if ((rc = mhip_launch_cross_absorbed(ctx, cd))) return rc;
      } else {
        DecAttnDesc ca;
        ca.q = b.qb; ca.k = b.ck + l * cross_l; ca.v = b.cv + l * cross_l; ca.out = b.ao; ca.kv_rows = vg.npad;
        ca.ldq = ca.ldk = ca.ldo = D; ca.heads = c.dec_heads; ca.groups = n; ca.nq = beam; ca.n_keys = vg.n_tok;
        if ((rc = mhip_launch_decode_attention(ctx, prec, ca))) return rc;
      }
      if ((rc = mhip_gemm(ctx, prec, b.ao, a.d(lay(l, "ca_o") + "_w"), M, D, D, nullptr, a.d<float>(lay(l, "ca_o") + "_b"), b.x, ACT_NONE, 1, b.x))) return rc;
      if ((rc = mhip_launch_layernorm2(ctx, prec, b.x, a.d<float>(lay(l, "ca_ln") + "_g"), a.d<float>(lay(l, "ca_ln") + "_b"), b.x, b.xt, M, D, DEC_LN_EPS))) return rc;
      // feed-forward
      if ((rc = mhip_gemm(ctx, prec, b.xt, a.d(lay(l, "fc1_w")), M, F, D, nullptr, a.d<float>(lay(l, "fc1_b")), b.hid, ACT_GELU, 0))) return rc;
      if ((rc = mhip_gemm(ctx, prec, b.hid, a.d(lay(l, "fc2_w")), M, D, F, nullptr, a.d<float>(lay(l, "fc2_b")), b.x, ACT_NONE, 1, b.x))) return rc;
      if ((rc = mhip_launch_layernorm2(ctx, prec, b.x, a.d<float>(lay(l, "fin_ln") + "_g"), a.d<float>(lay(l, "fin_ln") + "_b"), b.x, b.xt, M, D, DEC_LN_EPS))) return rc;
    }
    if ((rc = mhip_gemm(ctx, prec, b.xt, a.d("out_w"), M, c.vocab, D, nullptr, nullptr, b.logits, ACT_NONE, 0, nullptr, ldv, 1))) return rc;
    if (step == 0 && step0_logits_host) {
      for (int i = 0; i < n; ++i) {
        if ((rc = mhip_launch_convert_rows(ctx, prec, b.logits + (size_t)i * beam * ldv * es, b.step0_stage, 1, c.vocab))) return rc;
        MHIP_HIP(ctx, hipMemcpyAsync(step0_logits_host + (size_t)i * c.vocab, b.step0_stage, (size_t)c.vocab * 4, hipMemcpyDeviceToHost, ctx->stream));
        MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
      }
    }
    BeamCandDesc bc;
    bc.logits = b.logits; bc.logits_f16 = prec == MHIP_PREC_F16; bc.ld = ldv; bc.vocab = c.vocab; bc.beam = beam; bc.bsz = n; bc.cum = b.bs.cum; bc.step = step;
    bc.max_len = ML; bc.min_len = c.min_len; bc.pad = c.pad; bc.eos = c.eos;
    bc.cand_scores = b.cand_scores; bc.cand_tokens = b.cand_tokens; bc.cand_beams = b.cand_beams;
    if ((rc = mhip_launch_beam_candidates(ctx, bc))) return rc;
    if (trace) {       // parity tests: the step's candidate list as the generator sees it (this path drains the stream)
      const size_t off = (size_t)step * n * K2;
      MHIP_HIP(ctx, hipMemcpyAsync(trace->scores + off, b.cand_scores, (size_t)n * K2 * 4, hipMemcpyDeviceToHost, ctx->stream));
      MHIP_HIP(ctx, hipMemcpyAsync(trace->tokens + off, b.cand_tokens, (size_t)n * K2 * 4, hipMemcpyDeviceToHost, ctx->stream));
      MHIP_HIP(ctx, hipMemcpyAsync(trace->beams + off, b.cand_beams, (size_t)n * K2 * 4, hipMemcpyDeviceToHost, ctx->stream));
      MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
      trace->steps = step + 1;
    }
    if ((rc = mhip_launch_beam_select(ctx, b.bs, tcur, step))) return rc;
    tcur ^= 1;
    MHIP_HIP(ctx, hipMemcpyAsync(&m->h_remaining[step], b.bs.remaining, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MHIP_HIP(ctx, hipEventRecord(m->rem_ev[step & 1], ctx->stream));
  }
  // best hypothesis per crop: highest score, first finalized wins ties (torch.sort(descending) on the score list)
  if ((rc = mhip_launch_beam_best(ctx, b.bs, b.out_tok, b.out_len, b.out_score))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(tokens_out, b.out_tok, (size_t)n * (ML + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(lengths_out, b.out_len, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(scores_out, b.out_score, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_trocr_generate(mhip_trocr* m, const uint8_t* crops_dev, int n, int swap_rb, int32_t* tokens_out,
                                   int32_t* lengths_out, float* scores_out) {
  if (!m || !crops_dev || !tokens_out || !lengths_out || !scores_out) return MHIP_EINVAL;
  return trocr_generate(m, crops_dev, n, swap_rb, tokens_out, lengths_out, scores_out, nullptr, nullptr);
}

// trocr_generate on host crops [n][img][img][3]
static int trocr_generate_host(mhip_trocr* m, const uint8_t* crops_host, int n, int swap_rb, int32_t* tokens_out, int32_t* lengths_out,
                               float* scores_out, float* enc_tokens_out, float* step0_logits_out, TrocrTrace* trace) {
  mhip_ctx* ctx = m->ctx;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  return mhip_with_upload(ctx, crops_host, (size_t)n * m->cfg.img_size * m->cfg.img_size * 3, "crop", [&](const uint8_t* dev) {
    return trocr_generate(m, dev, n, swap_rb, tokens_out, lengths_out, scores_out, enc_tokens_out, step0_logits_out, trace);
  });
}

extern "C" int mhip_trocr_generate_host(mhip_trocr* m, const uint8_t* crops_host, int n, int swap_rb, int32_t* tokens_out,
                                        int32_t* lengths_out, float* scores_out, float* enc_tokens_out,
                                        float* step0_logits_out) {
  if (!m || !crops_host || !tokens_out || !lengths_out || !scores_out || n < 1) return MHIP_EINVAL;
  return trocr_generate_host(m, crops_host, n, swap_rb, tokens_out, lengths_out, scores_out, enc_tokens_out, step0_logits_out, nullptr);
}

// generate_host + the candidate list of every step as the generator saw it (parity tests: the CPU restatement walks the two
// searches side by side).  trace_* : host arrays [max_len + 1][n][2 * beam]; *steps_out = steps that ran.
extern "C" int mhip_trocr_generate_trace_host(mhip_trocr* m, const uint8_t* crops_host, int n, int swap_rb, int32_t* tokens_out,
                                              int32_t* lengths_out, float* scores_out, float* trace_scores,
                                              int32_t* trace_tokens, int32_t* trace_beams, int* steps_out) {
  if (!m || !crops_host || !tokens_out || !lengths_out || !scores_out || !trace_scores || !trace_tokens || !trace_beams ||
      !steps_out || n < 1)
    return MHIP_EINVAL;
  TrocrTrace tr{trace_scores, trace_tokens, trace_beams, 0};
  const int rc = trocr_generate_host(m, crops_host, n, swap_rb, tokens_out, lengths_out, scores_out, nullptr, nullptr, &tr);
  *steps_out = tr.steps;
  return rc;
}

// The Pillow bicubic resize of n fragments to img x img into the handle's grow-only staging (m->frag_crops)
static int trocr_resize_fragments(mhip_trocr* m, const uint8_t* base_dev, const mhip_crop_desc* descs_host, int n) {
  mhip_ctx* ctx = m->ctx;
  const int S = m->cfg.img_size;
  int rc = m->frag_crops.ensure(ctx, (size_t)n * S * S * 3);
  if (!rc) rc = m->frag_scratch.ensure(ctx, mhip_pil_resize_fragments_scratch(descs_host, n, S, S, MHIP_PIL_BICUBIC));
  if (rc) return rc;
  return mhip_pil_resize_fragments(ctx, base_dev, descs_host, n, m->frag_crops.as<uint8_t>(), S, S, MHIP_PIL_BICUBIC, m->frag_scratch.p,
                                   m->frag_scratch.bytes);
}

// bytes of enc_store for `crops` crops
static size_t enc_store_bytes(const mhip_trocr* m, const VitGeom& vg, int crops) {
  return ((size_t)crops * vg.npad + CROSS_ATTN_SLACK_ROWS) * m->cfg.enc_dim * m->esz();
}

// Fragments of any size (u8, 3 channels, rows of row_stride bytes at base_dev + src_offset) -> Pillow bicubic resize to
// img x img (aspect ratio not preserved, as preprocess_image does) -> generate.
extern "C" int mhip_trocr_generate_fragments(mhip_trocr* m, const uint8_t* base_dev, const mhip_crop_desc* descs_host, int n,
                                             int swap_rb, int32_t* tokens_out, int32_t* lengths_out, float* scores_out) {
  if (!m || !base_dev || !descs_host || !tokens_out || !lengths_out || !scores_out || n < 1) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  int rc = trocr_resize_fragments(m, base_dev, descs_host, n);
  if (!rc) rc = trocr_generate(m, m->frag_crops.as<uint8_t>(), n, swap_rb, tokens_out, lengths_out, scores_out, nullptr, nullptr);
  return rc;
}

// ---- the same recognizer in two halves: the image encoder per batch of fragments, the decoder once over all of them ----------
// (OcrEngine's batched path: page batches leave the detector one after the other; their crops are encoded as they come — the
// encoder's GEMMs are as efficient on 300 crops as on 3000 — while the decoder, whose 16 steps are latency-bound on small
// batches (~5 ms per step whatever the batch), runs once.)
extern "C" int mhip_trocr_encode_begin(mhip_trocr* m, int max_crops) {
  if (!m || max_crops < 0) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  m->enc_count = 0;
  if (max_crops > m->enc_cap) {
    VitGeom vg;
    vit_geometry(m->vit, m->cfg.img_size, m->cfg.img_size, &vg);
    m->enc_cap = 0;
    const int rc = m->enc_store.ensure(ctx, enc_store_bytes(m, vg, max_crops));
    if (rc) return rc;
    m->enc_cap = max_crops;
  }
  return MHIP_OK;
}

extern "C" int mhip_trocr_encoded(mhip_trocr* m) { return m ? m->enc_count : MHIP_EINVAL; }

extern "C" int mhip_trocr_encode_fragments(mhip_trocr* m, const uint8_t* base_dev, const mhip_crop_desc* descs_host, int n,
                                           int swap_rb) {
  if (!m || !base_dev || !descs_host || n < 1) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  if (!m->ready) return mhip_fail(ctx, MHIP_ESTATE, "trocr: weights not finalized");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const mhip_trocr_config& c = m->cfg;
  const int S = c.img_size;
  const size_t es = m->esz();
  VitGeom vg;
  vit_geometry(m->vit, S, S, &vg);
  if (m->enc_count + n > m->enc_cap) {      // grow, keeping what has been encoded
    const int cap = std::max(m->enc_count + n, 2 * m->enc_cap);
    DevBuf bigger;
    bigger.bytes = enc_store_bytes(m, vg, cap);
    MHIP_HIP(ctx, hipMalloc(&bigger.p, bigger.bytes));
    if (m->enc_count) MHIP_HIP(ctx, hipMemcpyAsync(bigger.p, m->enc_store.p, (size_t)m->enc_count * vg.npad * c.enc_dim * es, hipMemcpyDeviceToDevice, ctx->stream));
    MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    m->enc_store.release();
    m->enc_store = bigger;
    m->enc_cap = cap;
  }
  VitRun run;
  run.tokens_dst = m->enc_store.as() + (size_t)m->enc_count * vg.npad * c.enc_dim * es;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) { vit_carve(m->vit, ws, n, vg, &run); });
  if (rc) return rc;
  if ((rc = trocr_resize_fragments(m, base_dev, descs_host, n))) return rc;
  if ((rc = vit_encode(m->vit, m->frag_crops.as<uint8_t>(), n, S, S, S, S, swap_rb, &run))) return rc;
  m->enc_count += n;
  return MHIP_OK;
}

extern "C" int mhip_trocr_decode(mhip_trocr* m, int32_t* tokens_out, int32_t* lengths_out, float* scores_out) {
  if (!m || !tokens_out || !lengths_out || !scores_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  if (m->enc_count < 1) return mhip_fail(ctx, MHIP_EINVAL, "trocr: nothing encoded since mhip_trocr_encode_begin");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const int n = m->enc_count;
  VitGeom vg;
  vit_geometry(m->vit, m->cfg.img_size, m->cfg.img_size, &vg);
  TrocrDecodeBufs b;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) { trocr_decode_carve(m, ws, n, vg, false, &b); });
  if (rc) return rc;
  // the slack rows behind the last crop are read (masked) by its final key tiles: keep them finite
  const size_t row = (size_t)m->cfg.enc_dim * m->esz();
  MHIP_HIP(ctx, hipMemsetAsync(m->enc_store.as() + (size_t)n * vg.npad * row, 0, CROSS_ATTN_SLACK_ROWS * row, ctx->stream));
  rc = trocr_decode(m, b, m->enc_store.as(), vg, n, tokens_out, lengths_out, scores_out, nullptr, nullptr);
  m->enc_count = 0;
  return rc;
}

// The decoder's encoder-attention stage on caller-supplied host inputs, through the absorbed kernels (f16 operands): what the
// parity tests compare with fairseq's MultiheadAttention (q already projected and scaled).  q [crops*beam][heads*64],
// enc [crops][n_tok][enc_dim], wk / wv [heads*64][enc_dim], bv [heads*64] -> out [crops*beam][heads*64], all fp32.
//
// mhip_cross_attention_stages_host is the same call with the crop pitch in the caller's hands (enc [crops][kv_rows][enc_dim],
// kv_rows >= n_tok, a multiple of 8: rows n_tok .. kv_rows - 1 of a crop are the caller's padding and must be finite) and with
// what each of the three kernels left on the device copied out: qt_out / ct_out [crops*beam][16][enc_dim] (either may be
// NULL).  The qt / ct scratch and the output are filled with 0xffff (an f16 NaN) before the launch, so whatever a kernel did not
// write comes back as NaN.  The CROSS_ATTN_SLACK_ROWS zero rows behind the last crop are appended here.
extern "C" int mhip_cross_attention_stages_host(mhip_ctx* ctx, const float* q, const float* enc, const float* wk, const float* wv,
                                                const float* bv, int crops, int beam, int heads, int n_tok, int kv_rows,
                                                int enc_dim, float* qt_out, float* ct_out, float* out) {
  if (!ctx) return MHIP_EINVAL;
  if (!q || !enc || !wk || !wv || !bv || !out) return mhip_fail(ctx, MHIP_EINVAL, "cross_attention: null operand");
  if (crops < 1 || n_tok < 1 || kv_rows < n_tok || kv_rows % 8)
    return mhip_fail(ctx, MHIP_EINVAL, "cross_attention: crops %d, n_tok %d, kv_rows %d (kv_rows >= n_tok >= 1, kv_rows %% 8 == 0)",
                     crops, n_tok, kv_rows);
  if (!mhip_cross_absorb_supported(enc_dim, beam, heads))
    return mhip_fail(ctx, MHIP_EINVAL, "cross_attention: unsupported shape (enc_dim %d, beam %d, heads %d)", enc_dim, beam, heads);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const int D = heads * 64, M = crops * beam;
  const size_t rowsIn = (size_t)crops * kv_rows, rowsE = rowsIn + CROSS_ATTN_SLACK_ROWS;
  std::vector<_Float16> hq((size_t)M * D), hE(rowsE * enc_dim, (_Float16)0.f), hkt((size_t)D * enc_dim), hwv((size_t)D * enc_dim);
  for (size_t i = 0; i < hq.size(); ++i) hq[i] = (_Float16)q[i];
  for (size_t i = 0; i < rowsIn * enc_dim; ++i) hE[i] = (_Float16)enc[i];
  pack_ca_kt(wk, heads, enc_dim, hkt.data());
  for (size_t i = 0; i < hwv.size(); ++i) hwv[i] = (_Float16)wv[i];
  const size_t scr = (size_t)M * 16 * enc_dim * 2;
  char *dq = nullptr, *dE = nullptr, *dkt = nullptr, *dwv = nullptr, *qt = nullptr, *ct = nullptr, *ao = nullptr;
  float* dbv = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dq = ws.take(hq.size() * 2); dE = ws.take(hE.size() * 2); dkt = ws.take(hkt.size() * 2);
    dwv = ws.take(hwv.size() * 2); dbv = ws.take<float>((size_t)D * 4);
    qt = ws.take(scr); ct = ws.take(scr); ao = ws.take((size_t)M * D * 2);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dq, hq.data(), hq.size() * 2, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dE, hE.data(), hE.size() * 2, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dkt, hkt.data(), hkt.size() * 2, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dwv, hwv.data(), hwv.size() * 2, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dbv, bv, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemsetAsync(qt, 0xff, scr, ctx->stream));
  MHIP_HIP(ctx, hipMemsetAsync(ct, 0xff, scr, ctx->stream));
  MHIP_HIP(ctx, hipMemsetAsync(ao, 0xff, (size_t)M * D * 2, ctx->stream));
  CrossAbsorbDesc cd;
  cd.q = dq; cd.ldq = D; cd.E = dE; cd.kv_rows = kv_rows; cd.n_keys = n_tok; cd.enc_dim = enc_dim;
  cd.wkt = dkt; cd.wv = dwv; cd.bv = dbv; cd.qt = qt; cd.ct = ct; cd.ao = ao; cd.ldo = D;
  cd.crops = crops; cd.beam = beam; cd.heads = heads;
  if ((rc = mhip_launch_cross_absorbed(ctx, cd))) return rc;
  std::vector<_Float16> ho((size_t)M * D), hqt(qt_out ? scr / 2 : 0), hct(ct_out ? scr / 2 : 0);
  MHIP_HIP(ctx, hipMemcpyAsync(ho.data(), ao, ho.size() * 2, hipMemcpyDeviceToHost, ctx->stream));
  if (qt_out) MHIP_HIP(ctx, hipMemcpyAsync(hqt.data(), qt, scr, hipMemcpyDeviceToHost, ctx->stream));
  if (ct_out) MHIP_HIP(ctx, hipMemcpyAsync(hct.data(), ct, scr, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < ho.size(); ++i) out[i] = (float)ho[i];
  for (size_t i = 0; i < hqt.size(); ++i) qt_out[i] = (float)hqt[i];
  for (size_t i = 0; i < hct.size(); ++i) ct_out[i] = (float)hct[i];
  return MHIP_OK;
}

extern "C" int mhip_cross_attention_host(mhip_ctx* ctx, const float* q, const float* enc, const float* wk, const float* wv,
                                         const float* bv, int crops, int beam, int heads, int n_tok, int enc_dim, float* out) {
  if (!ctx || !q || !enc || !wk || !wv || !bv || !out || crops < 1 || n_tok < 1) return MHIP_EINVAL;
  if (!mhip_cross_absorb_supported(enc_dim, beam, heads)) return mhip_fail(ctx, MHIP_EINVAL, "cross_attention: unsupported shape");
  // the crops at the production pitch (npad rows, zeros behind the tokens)
  const int npad = (n_tok + 7) / 8 * 8;
  std::vector<float> padded((size_t)crops * npad * enc_dim, 0.f);
  for (int c = 0; c < crops; ++c)
    std::copy(enc + (size_t)c * n_tok * enc_dim, enc + (size_t)(c + 1) * n_tok * enc_dim, padded.begin() + (size_t)c * npad * enc_dim);
  return mhip_cross_attention_stages_host(ctx, q, padded.data(), wk, wv, bv, crops, beam, heads, n_tok, npad, enc_dim, nullptr,
                                          nullptr, out);
}

// The decoder's decode attention on caller-supplied host inputs, through mhip_launch_decode_attention as trocr_decode drives it
// (operands rounded to the precision's element type, the production pitches): what the kernel-level tests compare with softmax
// attention in fp64.  See include/marie_hip.h for the two layouts.
template <typename T>
static void to_elems(const float* src, size_t n, std::vector<char>& dst, size_t off, size_t count, size_t src_ld, size_t dst_ld) {
  // count rows of n elements: src row i at src + i * src_ld -> dst element offset off + i * dst_ld
  T* d = (T*)dst.data();
  for (size_t i = 0; i < count; ++i)
    for (size_t j = 0; j < n; ++j) d[off + i * dst_ld + j] = (T)src[i * src_ld + j];
}

extern "C" int mhip_decode_attention_host(mhip_ctx* ctx, int precision, int heads, int n_keys, int nq, int rows, int slots,
                                          int kv_rows, const float* q, const float* k, const float* v, const int32_t* anc,
                                          int anc_ld, int force_generic, float* out) {
  if (!ctx || !q || !k || !v || !out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (heads < 1 || heads > 16 || n_keys < 1 || nq < 1 || rows < 1 || rows % nq)
    return mhip_fail(ctx, MHIP_EINVAL, "decode_attention_host: heads %d n_keys %d nq %d rows %d", heads, n_keys, nq, rows);
  // the launcher judges n_keys and nq; here only what the host layout needs to stay inside its buffers
  const bool self = anc != nullptr;
  if (self && (nq != 1 || slots < 1 || anc_ld < std::min(n_keys, DEC_ATTN_MAX_KEYS + 1)))
    return mhip_fail(ctx, MHIP_EINVAL, "decode_attention_host: self-attention needs nq 1, slots >= 1, anc_ld >= n_keys");
  if (!self && kv_rows < n_keys) return mhip_fail(ctx, MHIP_EINVAL, "decode_attention_host: kv_rows %d < n_keys %d", kv_rows, n_keys);
  const int hist = std::min(n_keys, DEC_ATTN_MAX_KEYS + 1);     // rows of history laid out (a rejected n_keys reads none)
  if (self)
    for (int r = 0; r < rows; ++r)
      for (int s = 0; s < hist; ++s)
        if (anc[(size_t)r * anc_ld + s] < 0 || anc[(size_t)r * anc_ld + s] >= slots)
          return mhip_fail(ctx, MHIP_EINVAL, "decode_attention_host: ancestry slot out of range at row %d step %d", r, s);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const int D = heads * 64, groups = rows / nq;
  const size_t es = precision == MHIP_PREC_F16 ? 2 : 4;
  // self-attention: one [hist][slots][3 D] buffer, q | k | v of a step side by side (the q columns of the history are never read by
  // the attention: NaN), the queries in a [rows][3 D] buffer of the same pitch.  cross: q [rows][D], k / v [groups][kv_rows][D].
  const int ldq = self ? 3 * D : D, ldk = self ? 3 * D : D;
  const size_t nq_el = (size_t)rows * ldq;
  const size_t nk_el = self ? (size_t)hist * slots * ldk : (size_t)groups * kv_rows * D;
  std::vector<char> hq(nq_el * es), hk(nk_el * es), hv(self ? 0 : nk_el * es);
  auto fill_nan = [&](std::vector<char>& b) {
    if (es == 2) std::fill((_Float16*)b.data(), (_Float16*)(b.data() + b.size()), (_Float16)NAN);
    else std::fill((float*)b.data(), (float*)(b.data() + b.size()), NAN);
  };
  fill_nan(hq);
  if (self) fill_nan(hk);
  auto conv = [&](const float* src, std::vector<char>& dst, size_t off, size_t count, size_t dst_ld) {
    if (es == 2) to_elems<_Float16>(src, D, dst, off, count, D, dst_ld);
    else to_elems<float>(src, D, dst, off, count, D, dst_ld);
  };
  conv(q, hq, 0, rows, ldq);
  if (self) {
    conv(k, hk, D, (size_t)hist * slots, ldk);
    conv(v, hk, 2 * D, (size_t)hist * slots, ldk);
  } else {
    conv(k, hk, 0, (size_t)groups * kv_rows, D);
    conv(v, hv, 0, (size_t)groups * kv_rows, D);
  }
  const size_t anc_bytes = self ? (size_t)rows * anc_ld * 4 : 0, out_bytes = (size_t)rows * D * es;
  char *dq = nullptr, *dk = nullptr, *dv = nullptr, *dout = nullptr;
  int* danc = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dq = ws.take(hq.size());
    dk = ws.take(hk.size());
    dv = self ? dk : ws.take(hv.size());
    danc = self ? ws.take<int>(anc_bytes) : nullptr;
    dout = ws.take(out_bytes);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dq, hq.data(), hq.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dk, hk.data(), hk.size(), hipMemcpyHostToDevice, ctx->stream));
  if (!self) MHIP_HIP(ctx, hipMemcpyAsync(dv, hv.data(), hv.size(), hipMemcpyHostToDevice, ctx->stream));
  if (self) MHIP_HIP(ctx, hipMemcpyAsync(danc, anc, anc_bytes, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemsetAsync(dout, 0xff, out_bytes, ctx->stream));      // all-ones: NaN in f16 and fp32, a cell left unwritten shows
  DecAttnDesc d;
  d.q = dq; d.k = self ? dk + (size_t)D * es : dk; d.v = self ? dk + (size_t)2 * D * es : dv; d.out = dout;
  d.anc = danc; d.anc_ld = anc_ld; d.slots = slots; d.kv_rows = kv_rows;
  d.ldq = ldq; d.ldk = ldk; d.ldo = D; d.heads = heads; d.groups = groups; d.nq = nq; d.n_keys = n_keys;
  d.force_generic = force_generic;
  if ((rc = mhip_launch_decode_attention(ctx, precision, d))) return rc;
  std::vector<char> ho(out_bytes);
  MHIP_HIP(ctx, hipMemcpyAsync(ho.data(), dout, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < (size_t)rows * D; ++i) out[i] = es == 2 ? (float)((const _Float16*)ho.data())[i] : ((const float*)ho.data())[i];
  return MHIP_OK;
}
