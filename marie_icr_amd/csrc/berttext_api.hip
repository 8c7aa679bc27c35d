// berttext_api.hip — BERT sentence encoders (the text embeddings of SentenceTransformerEmbeddings and JinaEmbeddings) behind the
// C ABI, and the three families that differ from BERT in the embedding front and one score term: RoBERTa (position rows from
// pad_id + 1), DistilBERT (no token types) and MPNet (both, and a relative attention bias shared by the layers).
//
// Host-side counterpart of SentenceTransformer.encode as marie/embeddings/sentence_transformers/sentence_transformers_embeddings.py
// and marie/embeddings/jina/jina_embeddings.py drive it: BertModel.forward without the pooler (transformers/models/bert/
// modeling_bert.py: BertEmbeddings, BertLayer under the padding mask), or JinaBERT (no position table, a symmetric ALiBi bias on
// the scores, a gated GELU MLP), or MPNetModel (transformers/models/mpnet/modeling_mpnet.py: MPNetEncoder.compute_position_bias
// folded into a table over the clamped distance query - key, `rel`), then the Pooling (mean over the attention mask, or the
// [CLS] row) and Normalize modules.  One object = one weight arena + the launch sequence.
//
// Row layout: every text owns `npad` rows (a multiple of 8, the same for the whole call) of which its first len[b] are its
// tokens; the rest carry the [PAD] id, are computed like any other row and are never a key.  The residual stream h is fp32.  The
// layers are LayoutLMv3's (post-LN: attention, ao GEMM + residual, LayerNorm, fc1, fc2 + residual, LayerNorm) with attn_short as
// the attention of calls of npad <= 128 and attn_long, which streams the keys, past that (at most 8192 rows a text and 4096 * 128
// rows a call).  The word table stays fp32 in both precision modes: it is a gather of B * npad rows, not a GEMM operand.
//
// The same handle runs LongformerForSequenceClassification behind pipeline("text-classification") (transformers/models/longformer/
// modeling_longformer.py: LongformerSelfAttention with global attention on <s> alone, LongformerClassificationHead), created
// through mhip_berttext_create_cls: RoBERTa's embedding front, and in every layer attn_window for the local queries (the band of
// that layer's window plus key 0), attn_global_row for query 0 (query_global / key_global / value_global over all the rows: k_g | v_g
// from one GEMM into the MLP's hidden buffer, which is free during the attention), then the block as above; cls_head on row 0.
#include <math.h>

#include "encoder_block.h"

enum { BT_POS_ABSOLUTE = 0, BT_POS_ALIBI = 1, BT_MLP_GELU = 0, BT_MLP_GEGLU = 1, BT_POOL_MEAN = 0, BT_POOL_CLS = 1 };

struct mhip_berttext {
  mhip_ctx* ctx = nullptr;
  int precision = MHIP_PREC_F16;
  mhip_berttext_config cfg{};
  int pos_offset = 0, rel_buckets = 0, rel_max_distance = 0;      // mhip_berttext_config_ex's; zero through mhip_berttext_create
  std::vector<int> window;                                        // mhip_berttext_config_cls's: the one-sided window of every layer
  int num_labels = 0, head_function = 0;                          // (empty: full attention); 0 labels: no classification head
  TensorStore store;
  Arena arena;
  bool ready = false;
  size_t esz() const { return precision == MHIP_PREC_F16 ? 2 : 4; }
  int head_dim() const { return cfg.dim / cfg.heads; }
  bool alibi() const { return cfg.position == BT_POS_ALIBI; }
  bool rel() const { return rel_buckets > 0; }
  bool geglu() const { return cfg.mlp == BT_MLP_GEGLU; }
  bool windowed() const { return !window.empty(); }
  bool has_head() const { return num_labels > 0; }
  // tokens of a text: the streamed attention's 8192, or the position table's rows when it has fewer
  int max_tokens() const { return alibi() ? 8192 : std::min(cfg.max_position - pos_offset, 8192); }
  int max_npad() const { return (max_tokens() + 7) / 8 * 8; }
};

namespace {

constexpr int MAX_TEXTS = 4096, MAX_ROWS = 128;      // MAX_ROWS: the LDS-resident attention's, the routing boundary
constexpr int MAX_LONG_ROWS = 8192;                   // the streamed attention's
constexpr long long MAX_CALL_ROWS = (long long)MAX_TEXTS * MAX_ROWS;      // B * npad of one call: the most this path has laid out
constexpr double LOG2E = 1.4426950408889634;

// the buffers of one call of B texts (and n_pairs cosines)
struct BertRun {
  int *ids = nullptr, *len = nullptr, *pair_a = nullptr, *pair_b = nullptr;
  float *h = nullptr, *y = nullptr, *emb = nullptr, *cos = nullptr;
  float *qg = nullptr, *logits = nullptr, *scores = nullptr;      // [B][D] the global queries (windowed); [B][L] each (head)
  char* gg = nullptr;      // [R][F] the gated product (geglu only)
  EncoderWs w;
};

void berttext_carve(const mhip_berttext* m, Carver& ws, int B, int npad, int n_pairs, BertRun* r) {
  const mhip_berttext_config& c = m->cfg;
  const size_t D = c.dim, F = c.ffn, R = (size_t)B * npad;
  r->ids = ws.take<int>(R * 4);
  r->len = ws.take<int>((size_t)B * 4);
  r->pair_a = n_pairs ? ws.take<int>((size_t)n_pairs * 4) : nullptr;
  r->pair_b = n_pairs ? ws.take<int>((size_t)n_pairs * 4) : nullptr;
  r->cos = n_pairs ? ws.take<float>((size_t)n_pairs * 4) : nullptr;
  r->h = ws.take<float>(R * D * 4);
  r->y = ws.take<float>(R * D * 4);
  r->emb = ws.take<float>((size_t)B * D * 4);
  r->gg = m->geglu() ? ws.take(R * F * m->esz()) : nullptr;
  r->qg = m->windowed() ? ws.take<float>((size_t)B * D * 4) : nullptr;
  r->logits = m->has_head() ? ws.take<float>((size_t)B * m->num_labels * 4) : nullptr;
  r->scores = m->has_head() ? ws.take<float>((size_t)B * m->num_labels * 4) : nullptr;
  // windowed: the hidden buffer also holds k_g | v_g [R][2 D] during the attention
  encoder_ws_carve(ws, R, D, std::max(m->geglu() ? 2 * F : F, m->windowed() ? 2 * D : (size_t)0), 0, m->esz(), &r->w);
}

bool npad_ok(int npad, int max_npad) { return npad >= 8 && npad % 8 == 0 && npad <= max_npad; }

// MPNet's relative attention bias as a function of d = query - key clamped to +-R (R = max_distance): out[h][d + R] =
// weight[bucket(-d)][h] * scale, the bucket MPNetEncoder.relative_position_bucket's (the T5 rule, in float32 as the library takes
// it: mhip_relative_position_bucket).  false where the rule is not defined (max_distance <= buckets / 4) or the bucket still
// changes past +-R, up to the MAX_LONG_ROWS rows a text can have: the clamp would then differ from the model
bool rel_table_fold(int buckets, int R, const float* weight, int heads, double scale, float* out) {
  if (R <= buckets / 4) return false;
  for (int sign = -1; sign <= 1; sign += 2) {
    const int at_r = mhip_relative_position_bucket(sign * R, buckets, R);
    for (int n = R + 1; n <= MAX_LONG_ROWS; ++n)
      if (mhip_relative_position_bucket(sign * n, buckets, R) != at_r) return false;
  }
  for (int d = -R; d <= R; ++d) {
    const int bucket = mhip_relative_position_bucket(-d, buckets, R);
    for (int h = 0; h < heads; ++h) out[(size_t)h * (2 * R + 1) + d + R] = (float)((double)weight[(size_t)bucket * heads + h] * scale);
  }
  return true;
}

// ALiBi slopes of n heads: for n a power of two 2^(-8 (i + 1) / n); otherwise those of the largest power of two p <= n, then the
// even-indexed slopes of 2 p, the first n - p of them
std::vector<double> alibi_slopes(int n) {
  auto pow2 = [](int p) {
    std::vector<double> s(p);
    for (int i = 0; i < p; ++i) s[i] = exp2(-8.0 * (i + 1) / p);
    return s;
  };
  int p = 1;
  while (p * 2 <= n) p *= 2;
  std::vector<double> s = pow2(p);
  if (p < n) {
    const std::vector<double> more = pow2(2 * p);
    for (int i = 0; i < n - p; ++i) s.push_back(more[2 * i]);
  }
  return s;
}

int berttext_check_call(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad) {
  mhip_ctx* ctx = m->ctx;
  if (!m->ready) return mhip_fail(ctx, MHIP_ESTATE, "berttext: weights not finalized");
  if (!ids || !len || B < 1 || B > MAX_TEXTS) return mhip_fail(ctx, MHIP_EINVAL, "berttext: bad arguments (%d texts; 1 .. %d)", B, MAX_TEXTS);
  if (!npad_ok(npad, m->max_npad()))
    return mhip_fail(ctx, MHIP_EINVAL, "berttext: %d rows a text (a multiple of 8 up to %d)", npad, m->max_npad());
  if ((long long)B * npad > MAX_CALL_ROWS)
    return mhip_fail(ctx, MHIP_EINVAL, "berttext: %d texts of %d rows are %lld rows, a call lays out at most %lld", B, npad, (long long)B * npad, MAX_CALL_ROWS);
  for (int b = 0; b < B; ++b)
    if (len[b] < 1 || len[b] > npad || len[b] > m->max_tokens())
      return mhip_fail(ctx, MHIP_EINVAL, "berttext: text %d has %d tokens (1 .. %d)", b, len[b], std::min(npad, m->max_tokens()));
  for (size_t e = 0; e < (size_t)B * npad; ++e)
    if (ids[e] < 0 || ids[e] >= m->cfg.vocab)
      return mhip_fail(ctx, MHIP_EINVAL, "berttext: id %d at text %zu, position %zu is outside the vocabulary of %d", ids[e], e / npad, e % npad, m->cfg.vocab);
  return MHIP_OK;
}

int berttext_upload(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad, const BertRun& run) {
  int rc = mhip_stage_h2d(m->ctx, run.ids, ids, (size_t)B * npad * 4);
  return rc ? rc : mhip_stage_h2d(m->ctx, run.len, len, (size_t)B * 4);
}

// ids / len staged in run -> embeddings in run.emb (want_emb), logits and scores in run.logits / run.scores (want_head).  taps (host, or null): h after the embedding kernel and after every layer,
// [depth + 1][B][npad][D]
int berttext_forward(mhip_berttext* m, int B, int npad, const BertRun& run, float* taps, bool want_emb, bool want_head) {
  mhip_ctx* ctx = m->ctx;
  const mhip_berttext_config& c = m->cfg;
  const int D = c.dim, F = c.ffn, prec = m->precision;
  const size_t es = m->esz(), R = (size_t)B * npad;
  const Arena& a = m->arena;
  const EncoderWs& w = run.w;
  int rc;
  if ((rc = mhip_launch_berttext_embed(ctx, prec, a.d<float>("word"), c.type_vocab ? a.d<float>("type0") : nullptr,
                                       m->alibi() ? nullptr : a.d<float>("pos"), a.d<float>("ln_emb_g"), a.d<float>("ln_emb_b"), c.ln_eps,
                                       run.ids, run.h, w.ht, B, npad, D, m->pos_offset)))
    return rc;
  auto tap = [&](int i) -> int {
    if (!taps) return MHIP_OK;
    MHIP_HIP(ctx, hipMemcpyAsync(taps + (size_t)i * R * D, run.h, R * D * 4, hipMemcpyDeviceToHost, ctx->stream));
    return MHIP_OK;
  };
  if ((rc = tap(0))) return rc;
  AttnShortDesc sd;
  sd.a = encoder_attn_desc(w.qk, w.vt, w.ao, D, es, B, c.heads, npad, npad);
  sd.len = run.len;
  sd.slopes = m->alibi() ? a.d<float>("alibi") : nullptr;
  sd.head_dim = m->head_dim();
  if (m->rel()) {
    sd.rel_table = a.d<float>("rel");
    sd.rel_radius = m->rel_max_distance;
  }
  AttnGlobalRowDesc gd;
  if (m->windowed()) {      // k_g | v_g rows in w.hid
    gd.qg = run.qg; gd.k = w.hid; gd.v = w.hid + (size_t)D * es; gd.out = w.ao; gd.len = run.len;
    gd.ldq = D; gd.ldk = gd.ldv = 2 * D; gd.ldo = D; gd.npad = npad; gd.heads = c.heads; gd.seqs = B; gd.out_rows = npad;
  }
  for (int i = 0; i < c.depth; ++i) {
    if (m->windowed()) {
      if ((rc = encoder_block_qkv(ctx, prec, a, i, w, sd.a))) return rc;
      if ((rc = mhip_gemm(ctx, prec, w.ht, a.d(enc_blk(i, "kvg_w")), (long long)R, 2 * D, D, nullptr, a.d<float>(enc_blk(i, "kvg_b")), w.hid, ACT_NONE, 0))) return rc;
      if ((rc = mhip_launch_first_row_linear(ctx, prec, w.ht, npad, a.d(enc_blk(i, "qg_w")), a.d<float>(enc_blk(i, "qg_b")), run.qg, B, D, D))) return rc;
      if ((rc = mhip_launch_attention_window(ctx, prec, sd, m->window[i]))) return rc;
      gd.bias = a.d<float>(enc_blk(i, "vg_b"));
      if ((rc = mhip_launch_attention_global_row(ctx, prec, gd))) return rc;      // row 0 of every text, over the window kernel's
    } else if ((rc = encoder_block_attention(ctx, prec, a, i, w, sd))) return rc;
    if ((rc = mhip_gemm(ctx, prec, w.ao, a.d(enc_blk(i, "ao_w")), (long long)R, D, D, nullptr, a.d<float>(enc_blk(i, "ao_b")), run.y, ACT_NONE, 1, run.h))) return rc;
    if ((rc = mhip_launch_row_layernorm(ctx, MHIP_K_BERTTEXT_EMBED, prec, run.y, 0, nullptr, a.d<float>(enc_blk(i, "ln1_g")), a.d<float>(enc_blk(i, "ln1_b")), run.h, w.ht, (int)R, D, c.ln_eps))) return rc;
    const char* hid = w.hid;
    if (m->geglu()) {
      if ((rc = mhip_gemm(ctx, prec, w.ht, a.d(enc_blk(i, "fc1_w")), (long long)R, 2 * F, D, nullptr, nullptr, w.hid, ACT_NONE, 0))) return rc;
      if ((rc = mhip_launch_geglu(ctx, prec, w.hid, run.gg, (long long)R, F))) return rc;
      hid = run.gg;
    } else {
      if ((rc = mhip_gemm(ctx, prec, w.ht, a.d(enc_blk(i, "fc1_w")), (long long)R, F, D, nullptr, a.d<float>(enc_blk(i, "fc1_b")), w.hid, ACT_GELU, 0))) return rc;
    }
    if ((rc = mhip_gemm(ctx, prec, hid, a.d(enc_blk(i, "fc2_w")), (long long)R, D, F, nullptr, a.d<float>(enc_blk(i, "fc2_b")), run.y, ACT_NONE, 1, run.h))) return rc;
    if ((rc = mhip_launch_row_layernorm(ctx, MHIP_K_BERTTEXT_EMBED, prec, run.y, 0, nullptr, a.d<float>(enc_blk(i, "ln2_g")), a.d<float>(enc_blk(i, "ln2_b")), run.h, w.ht, (int)R, D, c.ln_eps))) return rc;
    if ((rc = tap(i + 1))) return rc;
  }
  // the pooled rows and the head's outputs only where the call hands them on
  if (want_emb && (rc = mhip_launch_berttext_pool(ctx, run.h, run.len, B, npad, D, c.pool == BT_POOL_CLS, c.normalize, run.emb))) return rc;
  if (!want_head) return MHIP_OK;
  return mhip_launch_cls_head(ctx, run.h, npad, a.d<float>("cls_dense_w"), a.d<float>("cls_dense_b"), a.d<float>("cls_out_w"),
                              a.d<float>("cls_out_b"), B, D, m->num_labels, m->head_function, run.logits, run.scores);
}

// block i as Hugging Face BERT holds it, "encoder.layer.N.": attention.self.{query,key,value}, attention.output.{dense,LayerNorm},
// then intermediate.dense / output.{dense,LayerNorm}, or (gated) JinaBERT's mlp.{gated_layers,wo,layernorm}.  false (the error
// names the tensor) when one is missing or misshapen
bool bert_layer_weights(mhip_ctx* ctx, const TensorStore& st, int i, int D, int F, bool gated, EncoderBlockWeights* w) {
  const std::string p = "encoder.layer." + std::to_string(i) + ".";
  auto mat = [&](const std::string& k, int r, int c) -> const float* {
    const HostTensor* t = st.find(ctx, p + k, {r, c});
    return t ? t->data.data() : nullptr;
  };
  auto vec = [&](const std::string& k, int n) -> const float* {
    const HostTensor* t = st.find(ctx, p + k, {n});
    return t ? t->data.data() : nullptr;
  };
  if (!(w->wq = mat("attention.self.query.weight", D, D)) || !(w->bq = vec("attention.self.query.bias", D)) ||
      !(w->wk = mat("attention.self.key.weight", D, D)) || !(w->bk = vec("attention.self.key.bias", D)) ||
      !(w->wv = mat("attention.self.value.weight", D, D)) || !(w->bv = vec("attention.self.value.bias", D)) ||
      !(w->wo = mat("attention.output.dense.weight", D, D)) || !(w->bo = vec("attention.output.dense.bias", D)) ||
      !(w->ln1_g = vec("attention.output.LayerNorm.weight", D)) || !(w->ln1_b = vec("attention.output.LayerNorm.bias", D)))
    return false;
  w->gated = gated;
  if (gated)
    return (w->w1 = mat("mlp.gated_layers.weight", 2 * F, D)) && (w->w2 = mat("mlp.wo.weight", D, F)) && (w->b2 = vec("mlp.wo.bias", D)) &&
           (w->ln2_g = vec("mlp.layernorm.weight", D)) && (w->ln2_b = vec("mlp.layernorm.bias", D));
  return (w->w1 = mat("intermediate.dense.weight", F, D)) && (w->b1 = vec("intermediate.dense.bias", F)) &&
         (w->w2 = mat("output.dense.weight", D, F)) && (w->b2 = vec("output.dense.bias", D)) &&
         (w->ln2_g = vec("output.LayerNorm.weight", D)) && (w->ln2_b = vec("output.LayerNorm.bias", D));
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- lifecycle
// the one body of the create entries.  cls (or null): the windows and the head of mhip_berttext_config_cls
static int berttext_create_impl(mhip_ctx* ctx, int precision, const mhip_berttext_config_ex* cfg, const mhip_berttext_config_cls* cls,
                                mhip_berttext** out) {
  if (!ctx || !out || !cfg) return MHIP_EINVAL;
  *out = nullptr;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  const mhip_berttext_config& c = cfg->base;
  const mhip_berttext_config_ex& x = *cfg;
  if (c.dim < 64 || c.dim % 64 || c.dim > 1024) return mhip_fail(ctx, MHIP_EINVAL, "berttext: dim %d (a multiple of 64 up to 1024)", c.dim);
  if (c.heads < 1 || c.dim % c.heads || (c.dim / c.heads != 64 && c.dim / c.heads != 32))
    return mhip_fail(ctx, MHIP_EINVAL, "berttext: heads %d at dim %d: a head dimension of %d, the attention kernel has heads of 64 or 32", c.heads, c.dim,
                     c.heads > 0 ? c.dim / c.heads : 0);
  if (c.ffn < 64 || c.ffn % 64) return mhip_fail(ctx, MHIP_EINVAL, "berttext: ffn %d (a multiple of 64)", c.ffn);
  if (c.depth < 1) return mhip_fail(ctx, MHIP_EINVAL, "berttext: depth %d", c.depth);
  if (c.vocab < 2 || c.vocab > (1 << 24)) return mhip_fail(ctx, MHIP_EINVAL, "berttext: vocab %d", c.vocab);
  if (c.type_vocab < 0) return mhip_fail(ctx, MHIP_EINVAL, "berttext: type_vocab %d", c.type_vocab);
  if (c.position != BT_POS_ABSOLUTE && c.position != BT_POS_ALIBI) return mhip_fail(ctx, MHIP_EINVAL, "berttext: position %d (0 absolute, 1 alibi)", c.position);
  if (c.position == BT_POS_ABSOLUTE && c.max_position < 2) return mhip_fail(ctx, MHIP_EINVAL, "berttext: max_position %d", c.max_position);
  if (c.mlp != BT_MLP_GELU && c.mlp != BT_MLP_GEGLU) return mhip_fail(ctx, MHIP_EINVAL, "berttext: mlp %d (0 gelu, 1 geglu)", c.mlp);
  if (c.pool != BT_POOL_MEAN && c.pool != BT_POOL_CLS) return mhip_fail(ctx, MHIP_EINVAL, "berttext: pool %d (0 mean, 1 cls)", c.pool);
  if (c.normalize != 0 && c.normalize != 1) return mhip_fail(ctx, MHIP_EINVAL, "berttext: normalize %d (0 or 1)", c.normalize);
  if (!(c.ln_eps > 0.f)) return mhip_fail(ctx, MHIP_EINVAL, "berttext: ln_eps");
  if (x.pos_offset < 0 || (x.pos_offset && c.position != BT_POS_ABSOLUTE) || (c.position == BT_POS_ABSOLUTE && c.max_position - x.pos_offset < 2))
    return mhip_fail(ctx, MHIP_EINVAL, "berttext: pos_offset %d (0 .. max_position - 2 = %d with a position table, 0 without)", x.pos_offset, c.max_position - 2);
  if (x.rel_buckets < 0 || (x.rel_buckets && (x.rel_buckets < 4 || x.rel_buckets % 2 || x.rel_buckets > 4096)))
    return mhip_fail(ctx, MHIP_EINVAL, "berttext: rel_buckets %d (0: no relative attention bias; otherwise even, 4 .. 4096)", x.rel_buckets);
  if (x.rel_buckets && c.position == BT_POS_ALIBI)
    return mhip_fail(ctx, MHIP_EINVAL, "berttext: rel_buckets %d with position alibi: slopes and a relative table together", x.rel_buckets);
  if (x.rel_buckets ? (x.rel_max_distance < 1 || x.rel_max_distance > MAX_LONG_ROWS) : x.rel_max_distance != 0)
    return mhip_fail(ctx, MHIP_EINVAL, "berttext: rel_max_distance %d (1 .. %d with rel_buckets, 0 without)", x.rel_max_distance, MAX_LONG_ROWS);
  if (cls) {
    if (!cls->attention_window) return mhip_fail(ctx, MHIP_EINVAL, "berttext: attention_window is null");
    for (int i = 0; i < c.depth; ++i) {
      const int aw = cls->attention_window[i];
      if (aw < 2 || aw % 2) return mhip_fail(ctx, MHIP_EINVAL, "berttext: attention_window %d of layer %d (even and positive)", aw, i);
      if (aw / 2 > ATTN_WINDOW_MAX)
        return mhip_fail(ctx, MHIP_EINVAL, "berttext: attention_window %d of layer %d: a one-sided window of %d (at most %d)", aw, i, aw / 2, ATTN_WINDOW_MAX);
    }
    if (cls->num_labels < 1 || cls->num_labels > CLS_HEAD_MAX_LABELS)
      return mhip_fail(ctx, MHIP_EINVAL, "berttext: num_labels %d (1 .. %d)", cls->num_labels, CLS_HEAD_MAX_LABELS);
    if (cls->head_function < 0 || cls->head_function > 2)
      return mhip_fail(ctx, MHIP_EINVAL, "berttext: head_function %d (0 none, 1 softmax, 2 sigmoid)", cls->head_function);
    if (c.dim / c.heads != 64)
      return mhip_fail(ctx, MHIP_EINVAL, "berttext: heads %d at dim %d: a head dimension of %d, the windowed attention has heads of 64", c.heads, c.dim, c.dim / c.heads);
    if (c.position != BT_POS_ABSOLUTE || x.rel_buckets)
      return mhip_fail(ctx, MHIP_EINVAL, "berttext: attention_window with position alibi or rel_buckets: the windowed attention has no bias term");
  }
  mhip_berttext* m = new mhip_berttext();
  m->ctx = ctx;
  m->precision = precision;
  m->cfg = c;
  m->pos_offset = x.pos_offset; m->rel_buckets = x.rel_buckets; m->rel_max_distance = x.rel_max_distance;
  if (cls) {
    for (int i = 0; i < c.depth; ++i) m->window.push_back(cls->attention_window[i] / 2);
    m->num_labels = cls->num_labels; m->head_function = cls->head_function;
  }
  const size_t es = m->esz(), D = c.dim;
  Arena& a = m->arena;
  a.take("word", (size_t)c.vocab * D * 4);
  if (c.type_vocab) a.take("type0", D * 4);
  if (m->alibi()) a.take("alibi", (size_t)c.heads * 4);
  else a.take("pos", (size_t)(m->pos_offset + m->max_npad()) * D * 4);      // rows past the table (padding rows only) are zeros
  if (m->rel()) a.take("rel", (size_t)c.heads * (2 * m->rel_max_distance + 1) * 4);
  a.take("ln_emb_g", D * 4); a.take("ln_emb_b", D * 4);
  for (int i = 0; i < c.depth; ++i) {
    encoder_block_take(a, i, D, c.ffn, es, m->geglu());
    if (m->windowed()) {      // key_global | value_global, query_global (scaled), b_vg - b_v
      a.take(enc_blk(i, "kvg_w"), 2 * D * D * es); a.take(enc_blk(i, "kvg_b"), 2 * D * 4);
      a.take(enc_blk(i, "qg_w"), D * D * es); a.take(enc_blk(i, "qg_b"), D * 4);
      a.take(enc_blk(i, "vg_b"), D * 4);
    }
  }
  if (m->has_head()) {      // fp32 in both modes: B rows, not a GEMM
    a.take("cls_dense_w", D * D * 4); a.take("cls_dense_b", D * 4);
    a.take("cls_out_w", (size_t)m->num_labels * D * 4); a.take("cls_out_b", (size_t)m->num_labels * 4);
  }
  *out = m;
  return MHIP_OK;
}

extern "C" int mhip_berttext_create_ex(mhip_ctx* ctx, int precision, const mhip_berttext_config_ex* cfg, mhip_berttext** out) {
  return berttext_create_impl(ctx, precision, cfg, nullptr, out);
}

extern "C" int mhip_berttext_create_cls(mhip_ctx* ctx, int precision, const mhip_berttext_config_cls* cfg, mhip_berttext** out) {
  if (!ctx || !out || !cfg) return MHIP_EINVAL;
  return berttext_create_impl(ctx, precision, &cfg->ex, cfg, out);
}

// the twelve fields of mhip_berttext_config alone: a token type table is required, as it always was
extern "C" int mhip_berttext_create(mhip_ctx* ctx, int precision, const mhip_berttext_config* cfg, mhip_berttext** out) {
  if (!ctx || !out || !cfg) return MHIP_EINVAL;
  *out = nullptr;
  if (cfg->type_vocab < 1) return mhip_fail(ctx, MHIP_EINVAL, "berttext: type_vocab %d", cfg->type_vocab);
  mhip_berttext_config_ex x{};
  x.base = *cfg;
  return mhip_berttext_create_ex(ctx, precision, &x, out);
}

extern "C" int mhip_berttext_destroy(mhip_berttext* m) {
  if (!m) return MHIP_OK;
  mhip_quiesce(m->ctx);
  m->arena.release();
  delete m;
  return MHIP_OK;
}

extern "C" int mhip_berttext_set_tensor(mhip_berttext* m, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!m || !key) return MHIP_EINVAL;
  std::string k(key);
  if (k.rfind("bert.", 0) == 0) k = k.substr(5);
  else if (k.rfind("longformer.", 0) == 0) k = k.substr(11);
  if (k.rfind("pooler.", 0) == 0 || k == "embeddings.position_ids") return MHIP_OK;
  if (k.rfind("embeddings.", 0) != 0 && k.rfind("encoder.layer.", 0) != 0 && k != "encoder.relative_attention_bias.weight" &&
      !(m->has_head() && k.rfind("classifier.", 0) == 0))
    return mhip_fail(m->ctx, MHIP_EINVAL, "unknown state_dict key %s", key);
  m->ready = false;
  return m->store.set(m->ctx, k, data, shape, ndim);
}

extern "C" int mhip_berttext_alloc_arena(mhip_berttext* m) {
  if (!m) return MHIP_EINVAL;
  int rc = m->arena.alloc(m->ctx);
  if (rc) return rc;
  m->ready = true;
  return MHIP_OK;
}

extern "C" int mhip_berttext_arena(mhip_berttext* m, void** dev, size_t* bytes) {
  if (!m) return MHIP_EINVAL;
  if (dev) *dev = m->arena.dev;
  if (bytes) *bytes = m->arena.bytes;
  return MHIP_OK;
}

extern "C" int mhip_berttext_finalize(mhip_berttext* m) {
  if (!m) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  const mhip_berttext_config& c = m->cfg;
  const int D = c.dim, F = c.ffn, prec = m->precision;
  Arena& a = m->arena;
  const TensorStore& st = m->store;
  a.begin_fill();
  const HostTensor* word = st.find(ctx, "embeddings.word_embeddings.weight", {c.vocab, D});
  if (!word) return MHIP_ESTATE;
  const HostTensor* type = c.type_vocab ? st.find(ctx, "embeddings.token_type_embeddings.weight", {c.type_vocab, D}) : nullptr;
  if (c.type_vocab && !type) return MHIP_ESTATE;
  const HostTensor* g0 = st.find(ctx, "embeddings.LayerNorm.weight", {D});
  if (!g0) return MHIP_ESTATE;
  const HostTensor* b0 = st.find(ctx, "embeddings.LayerNorm.bias", {D});
  if (!b0) return MHIP_ESTATE;
  memcpy(a.h("word"), word->data.data(), word->numel() * 4);
  if (type) memcpy(a.h("type0"), type->data.data(), (size_t)D * 4);
  memcpy(a.h("ln_emb_g"), g0->data.data(), (size_t)D * 4); memcpy(a.h("ln_emb_b"), b0->data.data(), (size_t)D * 4);
  if (m->alibi()) {
    const std::vector<double> s = alibi_slopes(c.heads);
    float* dst = (float*)a.h("alibi");
    for (int h = 0; h < c.heads; ++h) dst[h] = (float)(s[h] * LOG2E);      // the scores are in log2 units
  } else {
    const HostTensor* pos = st.find(ctx, "embeddings.position_embeddings.weight", {c.max_position, D});
    if (!pos) return MHIP_ESTATE;
    memcpy(a.h("pos"), pos->data.data(), (size_t)std::min(c.max_position, m->pos_offset + m->max_npad()) * D * 4);
  }
  if (m->rel()) {
    const HostTensor* bias = st.find(ctx, "encoder.relative_attention_bias.weight", {m->rel_buckets, c.heads});
    if (!bias) return MHIP_ESTATE;
    for (float v : bias->data)
      if (!std::isfinite(v)) return mhip_fail(ctx, MHIP_EINVAL, "berttext: encoder.relative_attention_bias.weight holds a non-finite value");
    // the scores are in log2 units
    if (!rel_table_fold(m->rel_buckets, m->rel_max_distance, bias->data.data(), c.heads, LOG2E, (float*)a.h("rel")))
      return mhip_fail(ctx, MHIP_EINVAL, "berttext: rel_max_distance %d: the bucket of %d buckets still changes past that distance, the table cannot clamp there",
                       m->rel_max_distance, m->rel_buckets);
  }
  const float scale = (float)(LOG2E / sqrt((double)m->head_dim()));
  for (int i = 0; i < c.depth; ++i) {
    EncoderBlockWeights w;
    if (!bert_layer_weights(ctx, st, i, D, F, m->geglu(), &w)) return MHIP_ESTATE;
    encoder_block_fill(a, prec, i, D, F, w, scale);
    if (m->windowed()) {
      const std::string p = "encoder.layer." + std::to_string(i) + ".attention.self.";
      const HostTensor *wq = st.find(ctx, p + "query_global.weight", {D, D}), *bq = wq ? st.find(ctx, p + "query_global.bias", {D}) : nullptr;
      const HostTensor *wk = bq ? st.find(ctx, p + "key_global.weight", {D, D}) : nullptr, *bk = wk ? st.find(ctx, p + "key_global.bias", {D}) : nullptr;
      const HostTensor *wv = bk ? st.find(ctx, p + "value_global.weight", {D, D}) : nullptr, *bv = wv ? st.find(ctx, p + "value_global.bias", {D}) : nullptr;
      if (!bv) return MHIP_ESTATE;
      const size_t es = m->esz(), DD = (size_t)D * D;
      std::vector<float> sq(DD);
      for (size_t e = 0; e < DD; ++e) sq[e] = wq->data[e] * scale;
      Arena::put(prec, a.h(enc_blk(i, "qg_w")), sq.data(), DD);
      Arena::put(prec, a.h(enc_blk(i, "kvg_w")), wk->data.data(), DD);
      Arena::put(prec, a.h(enc_blk(i, "kvg_w")) + DD * es, wv->data.data(), DD);
      float *qb = (float*)a.h(enc_blk(i, "qg_b")), *kvb = (float*)a.h(enc_blk(i, "kvg_b")), *vb = (float*)a.h(enc_blk(i, "vg_b"));
      for (int d = 0; d < D; ++d) {
        qb[d] = bq->data[d] * scale;
        kvb[d] = bk->data[d];
        kvb[D + d] = 0.f;
        vb[d] = bv->data[d] - (w.bv ? w.bv[d] : 0.f);      // the output projection's folded bias adds W_o b_v to every row
      }
    }
  }
  if (m->has_head()) {
    const HostTensor *dw = st.find(ctx, "classifier.dense.weight", {D, D}), *db = dw ? st.find(ctx, "classifier.dense.bias", {D}) : nullptr;
    const HostTensor *ow = db ? st.find(ctx, "classifier.out_proj.weight", {m->num_labels, D}) : nullptr;
    const HostTensor* ob = ow ? st.find(ctx, "classifier.out_proj.bias", {m->num_labels}) : nullptr;
    if (!ob) return MHIP_ESTATE;
    memcpy(a.h("cls_dense_w"), dw->data.data(), dw->numel() * 4); memcpy(a.h("cls_dense_b"), db->data.data(), (size_t)D * 4);
    memcpy(a.h("cls_out_w"), ow->data.data(), ow->numel() * 4); memcpy(a.h("cls_out_b"), ob->data.data(), (size_t)m->num_labels * 4);
  }
  int rc = a.upload(ctx);
  if (rc) return rc;
  m->ready = true;
  m->store.t.clear();
  return MHIP_OK;
}

extern "C" size_t mhip_berttext_workspace_bytes(mhip_berttext* m, int B, int npad) {
  if (!m || B < 1 || B > MAX_TEXTS || !npad_ok(npad, m->max_npad()) || (long long)B * npad > MAX_CALL_ROWS) return 0;
  BertRun run;
  return mhip_layout_bytes([&](Carver& ws) { berttext_carve(m, ws, B, npad, 0, &run); });
}

extern "C" int mhip_berttext_alibi_slopes(int heads, float* slopes_out) {
  if (heads < 1 || heads > 4096 || !slopes_out) return MHIP_EINVAL;
  const std::vector<double> s = alibi_slopes(heads);
  for (int h = 0; h < heads; ++h) slopes_out[h] = (float)s[h];
  return MHIP_OK;
}

extern "C" int mhip_berttext_rel_table(int buckets, int max_distance, const float* weight, int heads, float* table_out) {
  if (buckets < 4 || buckets % 2 || buckets > 4096 || max_distance < 1 || max_distance > MAX_LONG_ROWS || heads < 1 || heads > 4096 || !weight ||
      !table_out)
    return MHIP_EINVAL;
  return rel_table_fold(buckets, max_distance, weight, heads, 1.0, table_out) ? MHIP_OK : MHIP_EINVAL;
}

// ---------------------------------------------------------------------------------------------------- forward
// the one body of the three entries: cosines with n_pairs > 0, taps with taps_out
static int berttext_run(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad, const int32_t* pair_a,
                        const int32_t* pair_b, int n_pairs, float* cos_out, float* taps_out, float* emb_out, float* logits_out = nullptr,
                        float* scores_out = nullptr) {
  mhip_ctx* ctx = m->ctx;
  if ((logits_out || scores_out) && !m->has_head()) return mhip_fail(ctx, MHIP_ESTATE, "berttext: the handle has no classification head");
  int rc = berttext_check_call(m, ids, len, B, npad);
  if (rc) return rc;
  if (cos_out) {
    if (n_pairs < 1 || n_pairs > (1 << 24)) return mhip_fail(ctx, MHIP_EINVAL, "berttext: %d pairs", n_pairs);
    for (int p = 0; p < n_pairs; ++p)
      if (pair_a[p] < 0 || pair_a[p] >= B || pair_b[p] < 0 || pair_b[p] >= B)
        return mhip_fail(ctx, MHIP_EINVAL, "berttext: pair %d names texts %d and %d of %d", p, pair_a[p], pair_b[p], B);
  }
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  BertRun run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { berttext_carve(m, ws, B, npad, n_pairs, &run); }))) return rc;
  if ((rc = berttext_upload(m, ids, len, B, npad, run))) return rc;
  if (cos_out) {
    if ((rc = mhip_stage_h2d(ctx, run.pair_a, pair_a, (size_t)n_pairs * 4))) return rc;
    if ((rc = mhip_stage_h2d(ctx, run.pair_b, pair_b, (size_t)n_pairs * 4))) return rc;
  }
  if ((rc = berttext_forward(m, B, npad, run, taps_out, emb_out || cos_out, logits_out || scores_out))) return rc;
  if (cos_out) {
    if ((rc = mhip_launch_pair_cosine(ctx, run.emb, m->cfg.dim, run.pair_a, run.pair_b, n_pairs, run.cos))) return rc;
    MHIP_HIP(ctx, hipMemcpyAsync(cos_out, run.cos, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (emb_out) MHIP_HIP(ctx, hipMemcpyAsync(emb_out, run.emb, (size_t)B * m->cfg.dim * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (logits_out) MHIP_HIP(ctx, hipMemcpyAsync(logits_out, run.logits, (size_t)B * m->num_labels * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (scores_out) MHIP_HIP(ctx, hipMemcpyAsync(scores_out, run.scores, (size_t)B * m->num_labels * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_berttext_embed_host(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad, float* emb_out) {
  if (!m || !emb_out) return MHIP_EINVAL;
  return berttext_run(m, ids, len, B, npad, nullptr, nullptr, 0, nullptr, nullptr, emb_out);
}

extern "C" int mhip_berttext_embed_pairs_host(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad,
                                              const int32_t* pair_a, const int32_t* pair_b, int n_pairs, float* cos_out, float* emb_out) {
  if (!m || !pair_a || !pair_b || !cos_out) return MHIP_EINVAL;
  return berttext_run(m, ids, len, B, npad, pair_a, pair_b, n_pairs, cos_out, nullptr, emb_out);
}

extern "C" int mhip_berttext_debug_taps_host(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad, float* taps_out,
                                             float* emb_out) {
  if (!m || !taps_out) return MHIP_EINVAL;
  return berttext_run(m, ids, len, B, npad, nullptr, nullptr, 0, nullptr, taps_out, emb_out);
}

extern "C" int mhip_berttext_classify_host(mhip_berttext* m, const int32_t* ids, const int32_t* len, int B, int npad, float* logits_out,
                                           float* scores_out) {
  if (!m || !logits_out || !scores_out) return MHIP_EINVAL;
  return berttext_run(m, ids, len, B, npad, nullptr, nullptr, 0, nullptr, nullptr, nullptr, logits_out, scores_out);
}

// ---------------------------------------------------------------------------------------------------- the kernels alone
// the one body of the two embedding entries: type0 may be null, pos holds pos_offset + npad rows
static int berttext_embed_rows_run(mhip_ctx* ctx, const float* word, const float* type0, const float* pos, const float* g, const float* b,
                                   float eps, const int32_t* ids, int B, int npad, int vocab, int D, int pos_offset, float* h_out) {
  if (!ctx || !word || !g || !b || !ids || !h_out) return MHIP_EINVAL;
  if (B < 1 || B > MAX_TEXTS || !npad_ok(npad, MAX_ROWS) || vocab < 1 || vocab > (1 << 24) || D < 64 || D % 64 || D > 1024 || !(eps > 0.f) ||
      pos_offset < 0 || pos_offset > MAX_LONG_ROWS)
    return mhip_fail(ctx, MHIP_EINVAL, "berttext_embed: B=%d npad=%d vocab=%d D=%d pos_offset=%d", B, npad, vocab, D, pos_offset);
  const size_t R = (size_t)B * npad, PR = (size_t)pos_offset + npad;
  for (size_t e = 0; e < R; ++e)
    if (ids[e] < 0 || ids[e] >= vocab) return mhip_fail(ctx, MHIP_EINVAL, "berttext_embed: id %d outside the vocabulary of %d", ids[e], vocab);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  float *dw = nullptr, *dt = nullptr, *dp = nullptr, *dg = nullptr, *db = nullptr, *dh = nullptr;
  int* di = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dw = ws.take<float>((size_t)vocab * D * 4); dt = ws.take<float>((size_t)D * 4); dp = ws.take<float>(PR * D * 4);
    dg = ws.take<float>((size_t)D * 4); db = ws.take<float>((size_t)D * 4); di = ws.take<int>(R * 4); dh = ws.take<float>(R * D * 4);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dw, word, (size_t)vocab * D * 4, hipMemcpyHostToDevice, ctx->stream));
  if (type0) MHIP_HIP(ctx, hipMemcpyAsync(dt, type0, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  if (pos) MHIP_HIP(ctx, hipMemcpyAsync(dp, pos, PR * D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dg, g, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(db, b, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(di, ids, R * 4, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_launch_berttext_embed(ctx, MHIP_PREC_F32, dw, type0 ? dt : nullptr, pos ? dp : nullptr, dg, db, eps, di, dh, nullptr, B, npad, D,
                                       pos_offset)))
    return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(h_out, dh, R * D * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_berttext_embed_rows_host(mhip_ctx* ctx, const float* word, const float* type0, const float* pos, const float* g,
                                             const float* b, float eps, const int32_t* ids, int B, int npad, int vocab, int D, float* h_out) {
  if (!type0) return MHIP_EINVAL;
  return berttext_embed_rows_run(ctx, word, type0, pos, g, b, eps, ids, B, npad, vocab, D, 0, h_out);
}

extern "C" int mhip_berttext_embed_rows_ex_host(mhip_ctx* ctx, const float* word, const float* type0, const float* pos, const float* g,
                                                const float* b, float eps, const int32_t* ids, int B, int npad, int vocab, int D,
                                                int pos_offset, float* h_out) {
  return berttext_embed_rows_run(ctx, word, type0, pos, g, b, eps, ids, B, npad, vocab, D, pos_offset, h_out);
}

// the one body of the attention entries: attn_short (npad <= 128), streamed, attn_long (npad <= 8192), or with a one-sided
// window w > 0, attn_window (head_dim 64, no bias term)
static int berttext_attention_run(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v, const int32_t* len,
                                  const float* slopes, const float* table, int radius, int B, int heads, int head_dim, int npad, float* out,
                                  bool streamed, int w = 0) {
  if (!ctx || !q || !k || !v || !len || !out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (head_dim != 64 && head_dim != 32) return mhip_fail(ctx, MHIP_EINVAL, "berttext_attention: head_dim %d (64 or 32)", head_dim);
  if (B < 1 || B > MAX_TEXTS || heads < 1 || heads > 32 || (heads * head_dim) % 64 || !npad_ok(npad, streamed ? MAX_LONG_ROWS : MAX_ROWS) ||
      (long long)B * npad > MAX_CALL_ROWS)
    return mhip_fail(ctx, MHIP_EINVAL, "berttext_attention: B=%d heads=%d npad=%d", B, heads, npad);
  for (int b = 0; b < B; ++b)
    if (len[b] < 1 || len[b] > npad) return mhip_fail(ctx, MHIP_EINVAL, "berttext_attention: sequence %d has %d keys (1 .. %d)", b, len[b], npad);
  const size_t tn = table ? (size_t)heads * (2 * (size_t)radius + 1) : 0;
  if (table) {
    if (radius < 0 || radius > MAX_LONG_ROWS) return mhip_fail(ctx, MHIP_EINVAL, "berttext_attention: radius %d (0 .. %d)", radius, MAX_LONG_ROWS);
    for (size_t e = 0; e < tn; ++e)      // the whole-row kernel masks by a -inf initial value: the term must not undo it
      if (!std::isfinite(table[e])) return mhip_fail(ctx, MHIP_EINVAL, "berttext_attention: the table holds a non-finite value (head %zu)", e / (2 * (size_t)radius + 1));
  }
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  float *dsl = nullptr, *dtab = nullptr;
  int* dlen = nullptr;
  return encoder_attention_host(
      ctx, precision, q, k, v, B, heads, head_dim, npad, out,
      [&](Carver& ws) {
        dlen = ws.take<int>((size_t)B * 4); dsl = ws.take<float>((size_t)heads * 4);
        if (tn) dtab = ws.take<float>(tn * 4);
      },
      [&](const AttnDesc& ad) {      // len, slopes and table are the caller's: they outlive the call's last synchronisation
        MHIP_HIP(ctx, hipMemcpyAsync(dlen, len, (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
        if (slopes) MHIP_HIP(ctx, hipMemcpyAsync(dsl, slopes, (size_t)heads * 4, hipMemcpyHostToDevice, ctx->stream));
        if (tn) MHIP_HIP(ctx, hipMemcpyAsync(dtab, table, tn * 4, hipMemcpyHostToDevice, ctx->stream));
        AttnShortDesc sd;
        sd.a = ad; sd.len = dlen; sd.slopes = slopes ? dsl : nullptr; sd.head_dim = head_dim;
        sd.rel_table = tn ? dtab : nullptr; sd.rel_radius = tn ? radius : 0;
        if (w) return mhip_launch_attention_window(ctx, precision, sd, w);
        return streamed ? mhip_launch_attention_long(ctx, precision, sd) : mhip_launch_attention_short(ctx, precision, sd);
      });
}

extern "C" int mhip_berttext_attention_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v, const int32_t* len,
                                            const float* slopes, int B, int heads, int head_dim, int npad, float* out) {
  return berttext_attention_run(ctx, precision, q, k, v, len, slopes, nullptr, 0, B, heads, head_dim, npad, out, false);
}

extern "C" int mhip_berttext_attention_long_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v,
                                                 const int32_t* len, const float* slopes, int B, int heads, int head_dim, int npad,
                                                 float* out) {
  return berttext_attention_run(ctx, precision, q, k, v, len, slopes, nullptr, 0, B, heads, head_dim, npad, out, true);
}

extern "C" int mhip_berttext_attention_rel_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v,
                                                const int32_t* len, const float* table, int radius, int B, int heads, int head_dim, int npad,
                                                float* out) {
  return berttext_attention_run(ctx, precision, q, k, v, len, nullptr, table, radius, B, heads, head_dim, npad, out, false);
}

extern "C" int mhip_berttext_attention_rel_long_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v,
                                                     const int32_t* len, const float* table, int radius, int B, int heads, int head_dim,
                                                     int npad, float* out) {
  return berttext_attention_run(ctx, precision, q, k, v, len, nullptr, table, radius, B, heads, head_dim, npad, out, true);
}

extern "C" int mhip_berttext_attention_window_host(mhip_ctx* ctx, int precision, const float* q, const float* k, const float* v,
                                                   const int32_t* len, int w, int B, int heads, int head_dim, int npad, float* out) {
  if (!ctx) return MHIP_EINVAL;
  if (head_dim != 64) return mhip_fail(ctx, MHIP_EINVAL, "berttext_attention_window: head_dim %d (64)", head_dim);
  if (w < 1 || w > ATTN_WINDOW_MAX) return mhip_fail(ctx, MHIP_EINVAL, "berttext_attention_window: w %d (one-sided, 1 .. %d)", w, ATTN_WINDOW_MAX);
  return berttext_attention_run(ctx, precision, q, k, v, len, nullptr, nullptr, 0, B, heads, head_dim, npad, out, true, w);
}

extern "C" int mhip_berttext_attention_global_host(mhip_ctx* ctx, int precision, const float* qg, const float* kg, const float* vg,
                                                   const int32_t* len, int B, int heads, int npad, float* out) {
  if (!ctx || !qg || !kg || !vg || !len || !out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (B < 1 || B > MAX_TEXTS || heads < 1 || heads > 32 || !npad_ok(npad, MAX_LONG_ROWS) || (long long)B * npad > MAX_CALL_ROWS)
    return mhip_fail(ctx, MHIP_EINVAL, "berttext_attention_global: B=%d heads=%d npad=%d", B, heads, npad);
  for (int b = 0; b < B; ++b)
    if (len[b] < 1 || len[b] > npad) return mhip_fail(ctx, MHIP_EINVAL, "berttext_attention_global: sequence %d has %d keys (1 .. %d)", b, len[b], npad);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t es = precision == MHIP_PREC_F16 ? 2 : 4, D = (size_t)heads * 64, R = (size_t)B * npad;
  char *dk = nullptr, *dv = nullptr, *dr = nullptr;
  float *dq = nullptr, *dout = nullptr;
  int* dlen = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dk = ws.take(R * D * es); dv = ws.take(R * D * es); dr = ws.take((size_t)B * D * es); dq = ws.take<float>((size_t)B * D * 4);
    dout = ws.take<float>((size_t)B * D * 4); dlen = ws.take<int>((size_t)B * 4);
  });
  if (rc) return rc;
  std::vector<char> kt(R * D * es), vt(R * D * es);
  Arena::put(precision, kt.data(), kg, R * D);
  Arena::put(precision, vt.data(), vg, R * D);
  MHIP_HIP(ctx, hipMemcpyAsync(dk, kt.data(), kt.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dv, vt.data(), vt.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dq, qg, (size_t)B * D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dlen, len, (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // kt, vt are host temporaries in pageable memory
  AttnGlobalRowDesc gd;
  gd.qg = dq; gd.k = dk; gd.v = dv; gd.out = dr; gd.len = dlen;
  gd.ldq = gd.ldk = gd.ldv = gd.ldo = (int)D; gd.npad = npad; gd.heads = heads; gd.seqs = B; gd.out_rows = 1;
  if ((rc = mhip_launch_attention_global_row(ctx, precision, gd))) return rc;
  if ((rc = mhip_launch_convert_rows(ctx, precision, dr, dout, B, (int)D))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(out, dout, (size_t)B * D * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_berttext_cls_head_host(mhip_ctx* ctx, const float* h0, const float* dense_w, const float* dense_b, const float* out_w,
                                           const float* out_b, int B, int D, int L, int function, float* logits_out, float* scores_out) {
  if (!ctx || !h0 || !dense_w || !dense_b || !out_w || !out_b || !logits_out || !scores_out) return MHIP_EINVAL;
  if (B < 1 || B > MAX_TEXTS || D < 64 || D % 64 || D > 1024 || L < 1 || L > CLS_HEAD_MAX_LABELS || function < 0 || function > 2)
    return mhip_fail(ctx, MHIP_EINVAL, "berttext_cls_head: B=%d D=%d L=%d function=%d", B, D, L, function);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t uD = D, uL = L;
  float *dh = nullptr, *dw = nullptr, *db = nullptr, *ow = nullptr, *ob = nullptr, *dl = nullptr, *ds = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dh = ws.take<float>(B * uD * 4); dw = ws.take<float>(uD * uD * 4); db = ws.take<float>(uD * 4); ow = ws.take<float>(uL * uD * 4);
    ob = ws.take<float>(uL * 4); dl = ws.take<float>(B * uL * 4); ds = ws.take<float>(B * uL * 4);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dh, h0, B * uD * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dw, dense_w, uD * uD * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(db, dense_b, uD * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(ow, out_w, uL * uD * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(ob, out_b, uL * 4, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_launch_cls_head(ctx, dh, 1, dw, db, ow, ob, B, D, L, function, dl, ds))) {
    (void)hipStreamSynchronize(ctx->stream);      // the copies from the caller's memory do not outlive the call
    return rc;
  }
  MHIP_HIP(ctx, hipMemcpyAsync(logits_out, dl, B * uL * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(scores_out, ds, B * uL * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_berttext_geglu_host(mhip_ctx* ctx, int precision, const float* x, int R, int F, float* out) {
  if (!ctx || !x || !out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (R < 1 || R > (1 << 20) || F < 8 || F % 8 || F > (1 << 16)) return mhip_fail(ctx, MHIP_EINVAL, "geglu: R=%d F=%d (a multiple of 8)", R, F);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t es = precision == MHIP_PREC_F16 ? 2 : 4, n = (size_t)R * F;
  char *dx = nullptr, *dy = nullptr;
  float* dout = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) { dx = ws.take(2 * n * es); dy = ws.take(n * es); dout = ws.take<float>(n * 4); });
  if (rc) return rc;
  std::vector<char> xt(2 * n * es);
  Arena::put(precision, xt.data(), x, 2 * n);
  MHIP_HIP(ctx, hipMemcpyAsync(dx, xt.data(), xt.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // xt is a host temporary in pageable memory
  if ((rc = mhip_launch_geglu(ctx, precision, dx, dy, R, F))) return rc;
  if ((rc = mhip_launch_convert_rows(ctx, precision, dy, dout, R, F))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(out, dout, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_berttext_pool_host(mhip_ctx* ctx, const float* h, const int32_t* len, int B, int npad, int D, int mode, int normalize,
                                       float* emb_out) {
  if (!ctx || !h || !len || !emb_out) return MHIP_EINVAL;
  if (B < 1 || B > MAX_TEXTS || !npad_ok(npad, MAX_ROWS) || D < 64 || D % 64 || D > 1024 || (mode != BT_POOL_MEAN && mode != BT_POOL_CLS) ||
      (normalize != 0 && normalize != 1))
    return mhip_fail(ctx, MHIP_EINVAL, "berttext_pool: B=%d npad=%d D=%d mode=%d normalize=%d", B, npad, D, mode, normalize);
  for (int b = 0; b < B; ++b)
    if (len[b] < 1 || len[b] > npad) return mhip_fail(ctx, MHIP_EINVAL, "berttext_pool: text %d has %d tokens (1 .. %d)", b, len[b], npad);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t HN = (size_t)B * npad * D;
  float *dh = nullptr, *de = nullptr;
  int* dl = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) { dh = ws.take<float>(HN * 4); de = ws.take<float>((size_t)B * D * 4); dl = ws.take<int>((size_t)B * 4); });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dh, h, HN * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dl, len, (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_launch_berttext_pool(ctx, dh, dl, B, npad, D, mode == BT_POOL_CLS, normalize, de))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(emb_out, de, (size_t)B * D * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}
