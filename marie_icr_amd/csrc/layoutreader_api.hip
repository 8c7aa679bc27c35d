// layoutreader_api.hip — LayoutReader reading order (the model behind TextLayout) behind the C ABI.
//
// Host-side counterpart of LayoutlmForSeq2SeqDecoder.forward with search_beam_size == 1 and pos_shift == False
// (marie/models/unilm/layoutreader/s2s_ft/modeling_decoding.py) as marie/document/layoutreader/text_layout.py drives it through
// Preprocess4Seq2seqDecoder: a layout-only LayoutLM encoder (post-LN BERT layers, erf GELU, a key projection without bias) over
// the source rows [CLS] words [SEP] pads, then T = S - 2 greedy steps of a pointer decoder, each feeding the row pointed at by
// the step before and a mask row, and scoring the mask row's output against the S embedded source rows.  One object = one
// weight arena + the launch sequence.
//
// What is computed differently, at identical results:
//   * K and V of a layer are cached ([layer][page][S + T][D]); the model projects the whole history again at every step;
//   * the encoder runs over the n + 2 real source rows of a page (rounded up to 8): a pad row is nobody's key and the pointer
//     head reads the embedding of the source rows, never their encoder output;
//   * the value bias is added behind the soft-max (encoder_block.h); key.bias is not used, as in the model.
// The source pass runs page by page (attn_flash over n + 2 keys), the T steps run on all pages at once: rows [page][pointed,
// mask], 2 * pages rows through the same weights.  A step is plain launches on the context's stream: the embedding kernel reads
// the rows the select kernel of the step before wrote, so no decision crosses to the host until all T are made.
#include <math.h>

#include "encoder_block.h"

struct mhip_layoutreader {
  mhip_ctx* ctx = nullptr;
  int precision = MHIP_PREC_F16;
  mhip_layoutreader_config cfg{};
  TensorStore store;
  Arena arena;
  bool ready = false;
  size_t esz() const { return precision == MHIP_PREC_F16 ? 2 : 4; }
  int S() const { return cfg.max_source; }
  int T() const { return cfg.max_source - 2; }
  int spad() const { return (cfg.max_source + 7) / 8 * 8; }
};

namespace {

constexpr int MAX_PAGES = 64;      // 2 * pages rows stay inside one row tile of the GEMMs: a page's rows do not depend on the batch
constexpr int BOX_MAX = 1000;

// the buffers of one call of `pages` pages
struct LrRun {
  int *src_tok = nullptr, *tok0 = nullptr, *tok = nullptr, *src_len = nullptr, *tgt_tab = nullptr, *forced = nullptr, *dec = nullptr;
  float *E = nullptr, *hs = nullptr, *ys = nullptr;      // source pass: embeddings [pages][spad][D], one page's stream and sum
  char* Et = nullptr;                                    // E in the element type
  EncoderWs w;                                           // one page's layer buffers
  float *h = nullptr, *y = nullptr, *hd = nullptr, *sc = nullptr;      // steps: [2 pages][D] each; scores
  char *ht = nullptr, *qkv = nullptr, *ao = nullptr, *hid = nullptr;
  char *kc = nullptr, *vc = nullptr;                     // [depth][pages][S + T][D]
};

void lr_carve(const mhip_layoutreader* m, Carver& ws, int pages, bool forced, bool all_scores, LrRun* r) {
  const mhip_layoutreader_config& c = m->cfg;
  const size_t D = c.dim, F = c.ffn, P = pages, SP = m->spad(), S = m->S(), T = m->T(), es = m->esz(), R = 2 * P;
  r->src_tok = ws.take<int>(P * SP * LR_TOK_INTS * 4);
  r->tok0 = ws.take<int>(P * LR_TOK_INTS * 4);
  r->tok = ws.take<int>(R * LR_TOK_INTS * 4);
  r->src_len = ws.take<int>(P * 4);
  r->tgt_tab = ws.take<int>(T * R * 4);
  r->forced = forced ? ws.take<int>(P * T * 4) : nullptr;
  r->dec = ws.take<int>(P * T * 4);
  r->E = ws.take<float>(P * SP * D * 4);
  r->Et = ws.take(P * SP * D * es);
  r->hs = ws.take<float>(SP * D * 4);
  r->ys = ws.take<float>(SP * D * 4);
  encoder_ws_carve(ws, SP, D, F, 0, es, &r->w);
  r->h = ws.take<float>(R * D * 4);
  r->y = ws.take<float>(R * D * 4);
  r->hd = ws.take<float>(R * D * 4);
  r->sc = ws.take<float>((all_scores ? P * T * S : P * S) * 4);
  r->ht = ws.take(R * D * es);
  r->qkv = ws.take(R * 3 * D * es);
  r->ao = ws.take(R * D * es);
  r->hid = ws.take(R * F * es);
  r->kc = ws.take((size_t)c.depth * P * (S + T) * D * es);
  r->vc = ws.take((size_t)c.depth * P * (S + T) * D * es);
}

// the entries of block i: encoder_block_take's, with v_w right behind qk_w and a bias of 3 D, so that a step's q | k | v is one
// GEMM over [3 D][D] while the source pass still finds its q|k and V^T operands under their names
void lr_block_take(Arena& a, int i, size_t D, size_t F, size_t es) {
  a.take(enc_blk(i, "ln1_g"), D * 4); a.take(enc_blk(i, "ln1_b"), D * 4);
  a.take(enc_blk(i, "qk_w"), 2 * D * D * es);      // D % 64 == 0: a multiple of 256 bytes, v_w follows without a gap
  a.take(enc_blk(i, "v_w"), D * D * es);
  a.take(enc_blk(i, "qk_b"), 3 * D * 4);           // q (scaled) | zeros (no key bias) | zeros (the value bias is in ao_b)
  a.take(enc_blk(i, "ao_w"), D * D * es); a.take(enc_blk(i, "ao_b"), D * 4);
  a.take(enc_blk(i, "ln2_g"), D * 4); a.take(enc_blk(i, "ln2_b"), D * 4);
  a.take(enc_blk(i, "fc1_w"), F * D * es); a.take(enc_blk(i, "fc1_b"), F * 4);
  a.take(enc_blk(i, "fc2_w"), D * F * es); a.take(enc_blk(i, "fc2_b"), D * 4);
}

// block i as the checkpoint holds it, "encoder.layer.N.": BERT's keys; attention.self.key.bias is not looked up
bool lr_layer_weights(mhip_ctx* ctx, const TensorStore& st, int i, int D, int F, EncoderBlockWeights* w) {
  const std::string p = "encoder.layer." + std::to_string(i) + ".";
  auto mat = [&](const std::string& k, int r, int c) -> const float* {
    const HostTensor* t = st.find(ctx, p + k, {r, c});
    return t ? t->data.data() : nullptr;
  };
  auto vec = [&](const std::string& k, int n) -> const float* {
    const HostTensor* t = st.find(ctx, p + k, {n});
    return t ? t->data.data() : nullptr;
  };
  w->bk = nullptr;
  return (w->wq = mat("attention.self.query.weight", D, D)) && (w->bq = vec("attention.self.query.bias", D)) &&
         (w->wk = mat("attention.self.key.weight", D, D)) &&
         (w->wv = mat("attention.self.value.weight", D, D)) && (w->bv = vec("attention.self.value.bias", D)) &&
         (w->wo = mat("attention.output.dense.weight", D, D)) && (w->bo = vec("attention.output.dense.bias", D)) &&
         (w->ln1_g = vec("attention.output.LayerNorm.weight", D)) && (w->ln1_b = vec("attention.output.LayerNorm.bias", D)) &&
         (w->w1 = mat("intermediate.dense.weight", F, D)) && (w->b1 = vec("intermediate.dense.bias", F)) &&
         (w->w2 = mat("output.dense.weight", D, F)) && (w->b2 = vec("output.dense.bias", D)) &&
         (w->ln2_g = vec("output.LayerNorm.weight", D)) && (w->ln2_b = vec("output.LayerNorm.bias", D));
}

int lr_check_call(mhip_layoutreader* m, const int32_t* boxes, const int32_t* counts, int pages, const int32_t* forced) {
  mhip_ctx* ctx = m->ctx;
  const int S = m->S(), T = m->T();
  if (!m->ready) return mhip_fail(ctx, MHIP_ESTATE, "layoutreader: weights not finalized");
  if (!boxes || !counts || pages < 1 || pages > MAX_PAGES) return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: bad arguments (%d pages; 1 .. %d)", pages, MAX_PAGES);
  for (int p = 0; p < pages; ++p) {
    if (counts[p] < 0 || counts[p] > S - 2) return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: page %d has %d words (0 .. %d)", p, counts[p], S - 2);
    for (int i = 0; i < counts[p]; ++i) {
      const int32_t* b = boxes + ((size_t)p * (S - 2) + i) * 4;
      if (b[0] < 0 || b[1] < 0 || b[2] > BOX_MAX || b[3] > BOX_MAX || b[2] < b[0] || b[3] < b[1])
        return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: page %d, word %d: box (%d, %d, %d, %d) outside 0 .. %d or inverted", p, i, b[0], b[1], b[2], b[3], BOX_MAX);
    }
    if (forced)
      for (int t = 0; t < T; ++t)
        if (forced[(size_t)p * T + t] < 0 || forced[(size_t)p * T + t] >= S)
          return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: page %d, step %d: forced index %d outside 0 .. %d", p, t, forced[(size_t)p * T + t], S - 1);
  }
  return MHIP_OK;
}

LrEmbedDesc lr_embed_desc(const mhip_layoutreader* m, const int* tok, int rows, float* h, void* ht) {
  const Arena& a = m->arena;
  LrEmbedDesc e;
  e.tok = tok; e.pos = a.d<float>("pos"); e.xe = a.d<float>("xe"); e.ye = a.d<float>("ye"); e.he = a.d<float>("he"); e.we = a.d<float>("we");
  e.type = a.d<float>("type"); e.g = a.d<float>("ln_emb_g"); e.b = a.d<float>("ln_emb_b");
  e.h = h; e.ht = ht; e.rows = rows; e.D = m->cfg.dim; e.max_position = m->cfg.max_position; e.max_2d = m->cfg.max_2d;
  e.type_vocab = m->cfg.type_vocab; e.eps = m->cfg.ln_eps;
  return e;
}

// the MLP half of block i on `rows` rows: y = ao Wo^T + b + h -> h, ht = LN1 -> hid = gelu(fc1) -> y = fc2 + h -> h, ht = LN2
int lr_block_tail(mhip_layoutreader* m, int i, long long rows, const char* ao, float* h, char* ht, float* y, char* hid) {
  mhip_ctx* ctx = m->ctx;
  const Arena& a = m->arena;
  const int D = m->cfg.dim, F = m->cfg.ffn, prec = m->precision;
  const float eps = m->cfg.ln_eps;
  int rc;
  if ((rc = mhip_gemm(ctx, prec, ao, a.d(enc_blk(i, "ao_w")), rows, D, D, nullptr, a.d<float>(enc_blk(i, "ao_b")), y, ACT_NONE, 1, h))) return rc;
  if ((rc = mhip_launch_row_layernorm(ctx, MHIP_K_BERTTEXT_EMBED, prec, y, 0, nullptr, a.d<float>(enc_blk(i, "ln1_g")), a.d<float>(enc_blk(i, "ln1_b")), h, ht, (int)rows, D, eps))) return rc;
  if ((rc = mhip_gemm(ctx, prec, ht, a.d(enc_blk(i, "fc1_w")), rows, F, D, nullptr, a.d<float>(enc_blk(i, "fc1_b")), hid, ACT_GELU, 0))) return rc;
  if ((rc = mhip_gemm(ctx, prec, hid, a.d(enc_blk(i, "fc2_w")), rows, D, F, nullptr, a.d<float>(enc_blk(i, "fc2_b")), y, ACT_NONE, 1, h))) return rc;
  return mhip_launch_row_layernorm(ctx, MHIP_K_BERTTEXT_EMBED, prec, y, 0, nullptr, a.d<float>(enc_blk(i, "ln2_g")), a.d<float>(enc_blk(i, "ln2_b")), h, ht, (int)rows, D, eps);
}

// the source rows of every page: embeddings (run.E / run.Et), then page by page the encoder over the n + 2 real rows, filling
// rows [0, n + 2) of every layer's caches.  emb_out / last_out (host, or null): [pages][S][D]
int lr_source_pass(mhip_layoutreader* m, const int32_t* counts, int pages, const LrRun& run, float* emb_out, float* last_out) {
  mhip_ctx* ctx = m->ctx;
  const mhip_layoutreader_config& c = m->cfg;
  const int D = c.dim, prec = m->precision, S = m->S(), SP = m->spad(), CR = S + m->T();
  const size_t es = m->esz();
  const Arena& a = m->arena;
  const EncoderWs& w = run.w;
  int rc;
  if ((rc = mhip_launch_lr_embed(ctx, prec, lr_embed_desc(m, run.src_tok, pages * SP, run.E, run.Et)))) return rc;
  for (int p = 0; p < pages; ++p) {
    const int n2 = counts[p] + 2, npad = (n2 + 7) / 8 * 8;
    const float* Ep = run.E + (size_t)p * SP * D;
    if (emb_out) MHIP_HIP(ctx, hipMemcpyAsync(emb_out + (size_t)p * S * D, Ep, (size_t)S * D * 4, hipMemcpyDeviceToHost, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(run.hs, Ep, (size_t)npad * D * 4, hipMemcpyDeviceToDevice, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(w.ht, run.Et + (size_t)p * SP * D * es, (size_t)npad * D * es, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = encoder_ws_clear_slack(ctx, w, (size_t)npad, (size_t)D, es))) return rc;
    AttnDesc ad = encoder_attn_desc(w.qk, w.vt, w.ao, D, es, 1, c.heads, npad, n2);
    ad.n_queries = npad;      // the rows up to npad are queries like any other (finite, nobody reads them), never keys
    for (int i = 0; i < c.depth; ++i) {
      char* kc = run.kc + ((size_t)i * pages + p) * CR * D * es;
      char* vc = run.vc + ((size_t)i * pages + p) * CR * D * es;
      if ((rc = encoder_block_attention(ctx, prec, a, i, w, ad))) return rc;
      // the real rows' K (the k half of the q|k rows) and V (rows, where the attention took V^T) into the caches
      MHIP_HIP(ctx, hipMemcpy2DAsync(kc, (size_t)D * es, w.qk + (size_t)D * es, (size_t)2 * D * es, (size_t)D * es, (size_t)n2, hipMemcpyDeviceToDevice, ctx->stream));
      if ((rc = mhip_gemm(ctx, prec, w.ht, a.d(enc_blk(i, "v_w")), n2, D, D, nullptr, nullptr, vc, ACT_NONE, 0))) return rc;
      if ((rc = lr_block_tail(m, i, npad, w.ao, run.hs, w.ht, run.ys, w.hid))) return rc;
    }
    if (last_out) MHIP_HIP(ctx, hipMemcpyAsync(last_out + (size_t)p * S * D, run.hs, (size_t)n2 * D * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  return MHIP_OK;
}

// step t on all pages: the rows run.tok0 (t == 0: the mask row alone) or run.tok hold -> decision t, and the rows of step t + 1
int lr_decode_step(mhip_layoutreader* m, int t, int pages, const LrRun& run, bool all_scores) {
  mhip_ctx* ctx = m->ctx;
  const mhip_layoutreader_config& c = m->cfg;
  const int D = c.dim, prec = m->precision, S = m->S(), T = m->T(), SP = m->spad(), CR = S + T;
  const size_t es = m->esz();
  const Arena& a = m->arena;
  const int nq = t ? 2 : 1, rows = pages * nq;
  int rc;
  if ((rc = mhip_launch_lr_embed(ctx, prec, lr_embed_desc(m, t ? run.tok : run.tok0, rows, run.h, run.ht)))) return rc;
  LrDecAttnDesc d;
  d.q = run.qkv; d.k = run.qkv + (size_t)D * es; d.v = run.qkv + (size_t)2 * D * es; d.ld = 3 * D;
  d.out = run.ao; d.ldo = D;
  d.src_len = run.src_len; d.tgt_len = run.tgt_tab + (size_t)t * 2 * pages;
  d.pages = pages; d.heads = c.heads; d.nq = nq; d.cache_rows = CR; d.tgt_base = S; d.keep = 1;
  for (int i = 0; i < c.depth; ++i) {
    d.kc = run.kc + (size_t)i * pages * CR * D * es;
    d.vc = run.vc + (size_t)i * pages * CR * D * es;
    if ((rc = mhip_gemm(ctx, prec, run.ht, a.d(enc_blk(i, "qk_w")), rows, 3 * D, D, nullptr, a.d<float>(enc_blk(i, "qk_b")), run.qkv, ACT_NONE, 0))) return rc;
    if ((rc = mhip_launch_lr_decode_attention(ctx, prec, d))) return rc;
    if ((rc = lr_block_tail(m, i, rows, run.ao, run.h, run.ht, run.y, run.hid))) return rc;
  }
  if ((rc = mhip_gemm(ctx, prec, run.ht, a.d("head_w"), rows, D, D, nullptr, a.d<float>("head_b"), run.hd, ACT_GELU, 1))) return rc;
  float* sc = run.sc + (all_scores ? (size_t)t * S : 0);
  const long long stride = all_scores ? (long long)T * S : S;
  if ((rc = mhip_launch_lr_pointer_scores(ctx, run.hd, nq, a.d<float>("head_ln_g"), a.d<float>("head_ln_b"), c.ln_eps, run.E, SP,
                                          a.d<float>("ptr_bias"), S, D, pages, sc, stride)))
    return rc;
  return mhip_launch_lr_pointer_select(ctx, sc, stride, S, run.forced, t, T, run.src_tok, SP, run.src_len, c.target_type, pages, run.dec, run.tok);
}

// the one body of order_host and debug_host
int lr_run(mhip_layoutreader* m, const int32_t* boxes, const int32_t* counts, int pages, const int32_t* forced, int32_t* decisions,
           float* scores_out, float* emb_out, float* last_out) {
  mhip_ctx* ctx = m->ctx;
  int rc = lr_check_call(m, boxes, counts, pages, forced);
  if (rc) return rc;
  const mhip_layoutreader_config& c = m->cfg;
  const int S = m->S(), T = m->T(), SP = m->spad(), D = c.dim;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  LrRun run;
  const bool all_scores = scores_out != nullptr;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { lr_carve(m, ws, pages, forced != nullptr, all_scores, &run); }))) return rc;
  // the rows of the source: [CLS] (box 0) words [SEP] (box 1000) pads (box 0, position 0)
  std::vector<int> tok((size_t)pages * SP * LR_TOK_INTS, 0), tok0((size_t)pages * LR_TOK_INTS, 0), len(pages), tab((size_t)T * 2 * pages);
  for (int p = 0; p < pages; ++p) {
    const int n = counts[p];
    len[p] = n + 2;
    for (int r = 0; r < SP; ++r) {
      int* t = &tok[((size_t)p * SP + r) * LR_TOK_INTS];
      if (r >= 1 && r <= n) memcpy(t, boxes + ((size_t)p * (S - 2) + r - 1) * 4, 16);
      else if (r == n + 1) t[0] = t[1] = t[2] = t[3] = BOX_MAX;
      t[4] = r <= n + 1 ? r : 0;
      t[5] = c.source_type;
    }
    tok0[(size_t)p * LR_TOK_INTS + 4] = n + 2;
    tok0[(size_t)p * LR_TOK_INTS + 5] = c.target_type;
  }
  // cached target rows a step's rows see: the pointed tokens of steps 1 .. t - 1 (that of step t is the step's own first row)
  for (int t = 0; t < T; ++t) std::fill(tab.begin() + (size_t)t * 2 * pages, tab.begin() + (size_t)(t + 1) * 2 * pages, std::max(t - 1, 0));
  if ((rc = mhip_stage_h2d(ctx, run.src_tok, tok.data(), tok.size() * 4))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.tok0, tok0.data(), tok0.size() * 4))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.src_len, len.data(), len.size() * 4))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.tgt_tab, tab.data(), tab.size() * 4))) return rc;
  if (forced && (rc = mhip_stage_h2d(ctx, run.forced, forced, (size_t)pages * T * 4))) return rc;
  if (last_out) memset(last_out, 0, (size_t)pages * S * D * 4);      // rows past a page's [SEP] are not computed
  if ((rc = lr_source_pass(m, counts, pages, run, emb_out, last_out))) return rc;
  for (int t = 0; t < T; ++t)
    if ((rc = lr_decode_step(m, t, pages, run, all_scores))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(decisions, run.dec, (size_t)pages * T * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (scores_out) MHIP_HIP(ctx, hipMemcpyAsync(scores_out, run.sc, (size_t)pages * T * S * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- lifecycle
extern "C" int mhip_layoutreader_create(mhip_ctx* ctx, int precision, const mhip_layoutreader_config* cfg, mhip_layoutreader** out) {
  if (!ctx || !out || !cfg) return MHIP_EINVAL;
  *out = nullptr;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  const mhip_layoutreader_config& c = *cfg;
  if (c.dim < 64 || c.dim % 64 || c.dim > 1024) return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: dim %d (a multiple of 64 up to 1024)", c.dim);
  if (c.heads < 1 || c.dim % c.heads || c.dim / c.heads != 64)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: heads %d at dim %d: a head dimension of %d, the attention kernels have heads of 64", c.heads, c.dim,
                     c.heads > 0 ? c.dim / c.heads : 0);
  if (c.depth < 1) return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: depth %d", c.depth);
  if (c.ffn < 64 || c.ffn % 64) return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: ffn %d (a multiple of 64)", c.ffn);
  if (c.max_source < 3 || 2 * c.max_source - 1 > LR_ATTN_MAX_KEYS)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: max_source %d (3 .. %d: the decode attention has %d keys)", c.max_source, (LR_ATTN_MAX_KEYS + 1) / 2, LR_ATTN_MAX_KEYS);
  if (c.max_position < 2 * c.max_source - 2)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: max_position %d (the last step sits at position %d)", c.max_position, 2 * c.max_source - 3);
  if (c.max_2d <= BOX_MAX || c.max_2d > (1 << 20)) return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: max_2d %d (boxes reach %d)", c.max_2d, BOX_MAX);
  if (c.type_vocab < 1 || c.source_type < 0 || c.source_type >= c.type_vocab || c.target_type < 0 || c.target_type >= c.type_vocab)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: type ids %d / %d of %d", c.source_type, c.target_type, c.type_vocab);
  if (!(c.ln_eps > 0.f)) return mhip_fail(ctx, MHIP_EINVAL, "layoutreader: ln_eps");
  mhip_layoutreader* m = new mhip_layoutreader();
  m->ctx = ctx;
  m->precision = precision;
  m->cfg = c;
  const size_t es = m->esz(), D = c.dim;
  Arena& a = m->arena;
  a.take("pos", (size_t)c.max_position * D * 4);
  for (const char* k : {"xe", "ye", "he", "we"}) a.take(k, (size_t)c.max_2d * D * 4);
  a.take("type", (size_t)c.type_vocab * D * 4);
  a.take("ln_emb_g", D * 4); a.take("ln_emb_b", D * 4);
  for (int i = 0; i < c.depth; ++i) lr_block_take(a, i, D, c.ffn, es);
  a.take("head_w", D * D * es); a.take("head_b", D * 4);
  a.take("head_ln_g", D * 4); a.take("head_ln_b", D * 4);
  a.take("ptr_bias", (size_t)c.max_source * 4);
  *out = m;
  return MHIP_OK;
}

extern "C" int mhip_layoutreader_destroy(mhip_layoutreader* m) {
  if (!m) return MHIP_OK;
  mhip_quiesce(m->ctx);
  m->arena.release();
  delete m;
  return MHIP_OK;
}

extern "C" int mhip_layoutreader_set_tensor(mhip_layoutreader* m, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!m || !key) return MHIP_EINVAL;
  std::string k(key);
  if (k.rfind("bert.", 0) == 0) k = k.substr(5);
  auto ends = [&](const char* s) { const size_t n = strlen(s); return k.size() >= n && k.compare(k.size() - n, n, s) == 0; };
  if (k.rfind("pooler.", 0) == 0 || k.rfind("cls.seq_relationship.", 0) == 0 || k == "embeddings.position_ids" ||
      k == "embeddings.word_embeddings.weight" || ends("attention.self.key.bias"))
    return MHIP_OK;
  if (k.rfind("embeddings.", 0) != 0 && k.rfind("encoder.layer.", 0) != 0 && k.rfind("cls.predictions.", 0) != 0)
    return mhip_fail(m->ctx, MHIP_EINVAL, "unknown state_dict key %s", key);
  m->ready = false;
  return m->store.set(m->ctx, k, data, shape, ndim);
}

extern "C" int mhip_layoutreader_alloc_arena(mhip_layoutreader* m) {
  if (!m) return MHIP_EINVAL;
  int rc = m->arena.alloc(m->ctx);
  if (rc) return rc;
  m->ready = true;
  return MHIP_OK;
}

extern "C" int mhip_layoutreader_arena(mhip_layoutreader* m, void** dev, size_t* bytes) {
  if (!m) return MHIP_EINVAL;
  if (dev) *dev = m->arena.dev;
  if (bytes) *bytes = m->arena.bytes;
  return MHIP_OK;
}

extern "C" int mhip_layoutreader_finalize(mhip_layoutreader* m) {
  if (!m) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  const mhip_layoutreader_config& c = m->cfg;
  const int D = c.dim, F = c.ffn, prec = m->precision;
  Arena& a = m->arena;
  const TensorStore& st = m->store;
  if (a.off.at(enc_blk(0, "v_w")) != a.off.at(enc_blk(0, "qk_w")) + (size_t)2 * D * D * m->esz())
    return mhip_fail(ctx, MHIP_ESTATE, "layoutreader: the q|k and v matrices are not adjacent in the arena");
  a.begin_fill();
  struct { const char* key; const char* entry; int rows; } tables[] = {
      {"embeddings.position_embeddings.weight", "pos", c.max_position},
      {"embeddings.x_position_embeddings.weight", "xe", c.max_2d},
      {"embeddings.y_position_embeddings.weight", "ye", c.max_2d},
      {"embeddings.h_position_embeddings.weight", "he", c.max_2d},
      {"embeddings.w_position_embeddings.weight", "we", c.max_2d},
      {"embeddings.token_type_embeddings.weight", "type", c.type_vocab}};
  for (const auto& t : tables) {
    const HostTensor* h = st.find(ctx, t.key, {t.rows, D});
    if (!h) return MHIP_ESTATE;
    memcpy(a.h(t.entry), h->data.data(), h->numel() * 4);
  }
  struct { const char* key; const char* entry; int n; } vecs[] = {
      {"embeddings.LayerNorm.weight", "ln_emb_g", D}, {"embeddings.LayerNorm.bias", "ln_emb_b", D},
      {"cls.predictions.transform.dense.bias", "head_b", D},
      {"cls.predictions.transform.LayerNorm.weight", "head_ln_g", D}, {"cls.predictions.transform.LayerNorm.bias", "head_ln_b", D},
      {"cls.predictions.bias", "ptr_bias", c.max_source}};
  for (const auto& v : vecs) {
    const HostTensor* h = st.find(ctx, v.key, {v.n});
    if (!h) return MHIP_ESTATE;
    memcpy(a.h(v.entry), h->data.data(), (size_t)v.n * 4);
  }
  const HostTensor* hw = st.find(ctx, "cls.predictions.transform.dense.weight", {D, D});
  if (!hw) return MHIP_ESTATE;
  Arena::put(prec, a.h("head_w"), hw->data.data(), hw->numel());
  for (int i = 0; i < c.depth; ++i) {
    EncoderBlockWeights w;
    if (!lr_layer_weights(ctx, st, i, D, F, &w)) return MHIP_ESTATE;
    encoder_block_fill(a, prec, i, D, F, w);      // heads of 64: ATTN_SCORE_SCALE
  }
  int rc = a.upload(ctx);
  if (rc) return rc;
  m->ready = true;
  m->store.t.clear();
  return MHIP_OK;
}

extern "C" size_t mhip_layoutreader_workspace_bytes(mhip_layoutreader* m, int pages) {
  if (!m || pages < 1 || pages > MAX_PAGES) return 0;
  LrRun run;
  return mhip_layout_bytes([&](Carver& ws) { lr_carve(m, ws, pages, false, false, &run); });
}

// ---------------------------------------------------------------------------------------------------- forward
extern "C" int mhip_layoutreader_order_host(mhip_layoutreader* m, const int32_t* boxes, const int32_t* counts, int pages, int32_t* decisions) {
  if (!m || !decisions) return MHIP_EINVAL;
  return lr_run(m, boxes, counts, pages, nullptr, decisions, nullptr, nullptr, nullptr);
}

extern "C" int mhip_layoutreader_debug_host(mhip_layoutreader* m, const int32_t* boxes, const int32_t* counts, int pages, const int32_t* forced,
                                            int32_t* decisions, float* scores_out, float* emb_out, float* last_out) {
  if (!m || !decisions) return MHIP_EINVAL;
  return lr_run(m, boxes, counts, pages, forced, decisions, scores_out, emb_out, last_out);
}

// ---------------------------------------------------------------------------------------------------- the kernel alone
extern "C" int mhip_layoutreader_attention_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v, const float* kc,
                                                const float* vc, const int32_t* src_len, const int32_t* tgt_len, int pages, int nq, int heads,
                                                int cache_rows, int tgt_base, float* out) {
  if (!ctx || !q || !k || !v || !kc || !vc || !src_len || !tgt_len || !out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (pages < 1 || pages > 4096 || (nq != 1 && nq != 2) || heads < 1 || heads > 16 || tgt_base < 1 || tgt_base > LR_ATTN_MAX_KEYS - 2 ||
      cache_rows < tgt_base || cache_rows > 4096)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutreader_attention: pages=%d nq=%d heads=%d cache_rows=%d tgt_base=%d", pages, nq, heads, cache_rows, tgt_base);
  for (int p = 0; p < pages; ++p) {
    int tmax = 0;
    for (int i = 0; i < nq; ++i) {
      const int tl = tgt_len[p * nq + i];
      if (tl < 0 || tl > cache_rows - tgt_base) return mhip_fail(ctx, MHIP_EINVAL, "layoutreader_attention: row %d sees %d target rows (0 .. %d)", p * nq + i, tl, cache_rows - tgt_base);
      tmax = std::max(tmax, tl);
    }
    if (src_len[p] < 0 || src_len[p] > tgt_base || src_len[p] + tmax + nq > LR_ATTN_MAX_KEYS)
      return mhip_fail(ctx, MHIP_EINVAL, "layoutreader_attention: page %d has %d source and %d target keys (source <= %d, %d keys in all)", p, src_len[p], tmax, tgt_base, LR_ATTN_MAX_KEYS);
  }
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t es = precision == MHIP_PREC_F16 ? 2 : 4, D = (size_t)heads * 64, R = (size_t)pages * nq, CN = (size_t)pages * cache_rows * D;
  char *dq = nullptr, *dk = nullptr, *dv = nullptr, *dkc = nullptr, *dvc = nullptr, *dao = nullptr;
  float* dout = nullptr;
  int *dsl = nullptr, *dtl = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dq = ws.take(R * D * es); dk = ws.take(R * D * es); dv = ws.take(R * D * es); dkc = ws.take(CN * es); dvc = ws.take(CN * es);
    dao = ws.take(R * D * es); dout = ws.take<float>(R * D * 4); dsl = ws.take<int>((size_t)pages * 4); dtl = ws.take<int>(R * 4);
  });
  if (rc) return rc;
  std::vector<char> tq(R * D * es), tk(R * D * es), tv(R * D * es), tkc(CN * es), tvc(CN * es);
  Arena::put(precision, tq.data(), q, R * D); Arena::put(precision, tk.data(), k, R * D); Arena::put(precision, tv.data(), v, R * D);
  Arena::put(precision, tkc.data(), kc, CN); Arena::put(precision, tvc.data(), vc, CN);
  MHIP_HIP(ctx, hipMemcpyAsync(dq, tq.data(), tq.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dk, tk.data(), tk.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dv, tv.data(), tv.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dkc, tkc.data(), tkc.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dvc, tvc.data(), tvc.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dsl, src_len, (size_t)pages * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dtl, tgt_len, R * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the sources are host temporaries in pageable memory
  LrDecAttnDesc d;
  d.q = dq; d.k = dk; d.v = dv; d.kc = dkc; d.vc = dvc; d.out = dao; d.src_len = dsl; d.tgt_len = dtl;
  d.ld = (int)D; d.ldo = (int)D; d.pages = pages; d.heads = heads; d.nq = nq; d.cache_rows = cache_rows; d.tgt_base = tgt_base; d.keep = 0;
  if ((rc = mhip_launch_lr_decode_attention(ctx, precision, d))) return rc;
  if ((rc = mhip_launch_convert_rows(ctx, precision, dao, dout, (int)R, (int)D))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(out, dout, R * D * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}
