// layoutlmv3_api.hip — the LayoutLMv3 page classifier and token tagger behind the C ABI.
//
// Host-side counterpart of LayoutLMv3ForSequenceClassification.forward (transformers/models/layoutlmv3/modeling_layoutlmv3.py:
// LayoutLMv3Model.forward, LayoutLMv3Encoder.forward, LayoutLMv3Layer, LayoutLMv3ClassificationHead) as
// TransformersDocumentClassifier drives it (marie/components/document_classifier/transformers.py, task
// "text-classification-multimodal"), and of LayoutLMv3ForTokenClassification.forward as TransformersDocumentIndexer drives it
// (marie/components/document_indexer/transformers.py:519-568).  One object = one weight arena + the launch sequence.
//
// A call runs `n` windows of text over `n_pages` page images: window w attends to the patch rows of page win_page[w].  The
// classifier has one window a page (the identity map); the tagger cuts a long page into several windows that share the page's
// resize, patch matrix and patch projection.
//
// Row layout: every window owns `npad` rows (seq_len rounded up to 8): max_text text rows, then cls + patches, then zeros.
// Padded text rows stay in the sequence and are masked as keys, as the library does.
// The hidden states h are fp32 (every LayerNorm writes them, and their copy in the GEMM element type); a post-LN layer is
//   q|k = ht Wqk^T + b        V^T = Wv ht^T            (the value bias moves into the output projection: soft-max rows sum to 1)
//   ao = attention_bias(q, k, V^T)     y = ao Wo^T + (bo + Wo bv) + h     h, ht = LN(y)
//   hid = gelu(ht Wi^T + bi)           y = hid Wd^T + bd + h              h, ht = LN(y)
#include <math.h>

#include "encoder_block.h"

struct mhip_layoutlmv3 {
  mhip_ctx* ctx = nullptr;
  int precision = MHIP_PREC_F16;
  int resample = MHIP_PIL_BILINEAR;      // the Pillow filter of the page resize (mhip_layoutlmv3_set_resample)
  mhip_layoutlmv3_config cfg{};
  TensorStore store;
  Arena arena;
  bool ready = false;
  int head = -1;      // HEAD_DENSE / HEAD_LINEAR; -1 until finalize (or, after alloc_arena, until the first call reads it back)
  size_t esz() const { return precision == MHIP_PREC_F16 ? 2 : 4; }
  int grid() const { return cfg.input_size / cfg.patch; }
  int n_vis() const { return grid() * grid() + 1; }
  int seq() const { return cfg.max_text + n_vis(); }
  int npad() const { return (seq() + 7) / 8 * 8; }
  int dp() const { return std::max(cfg.max_text, n_vis()) - 1; }
  int dx() const { return cfg.max_2d_position_embeddings - 1; }
};

namespace {

// classifier.dense + classifier.out_proj (sequence classification; token classification with num_labels >= 10), or one
// classifier.weight (token classification with num_labels < 10)
enum { HEAD_DENSE = 0, HEAD_LINEAR = 1 };
enum { TASK_CLASSIFY = 0, TASK_TAG = 1 };
const char* PFX = "layoutlmv3.";

std::string lyr(int i, const char* s) { return "layoutlmv3.encoder.layer." + std::to_string(i) + "." + s; }

// the buffers of one call of n windows over n_pages pages
struct Lmv3Run {
  uint8_t* resized = nullptr;
  void* frag_scratch = nullptr;
  size_t frag_bytes = 0;
  int *tok = nullptr, *win_page = nullptr, *labels = nullptr;
  uint32_t *qcode = nullptr, *kcode = nullptr;
  float *pe = nullptr, *h = nullptr, *y = nullptr, *logits = nullptr, *scores = nullptr, *dense = nullptr;
  EncoderWs w;      // w.hid is also the patch matrix (n_pages <= n, fewer rows than R)
};

// task: TASK_CLASSIFY (logits [n][labels]) or TASK_TAG (labels / scores [n][max_text]; token logits when want_logits; the
// dense product of the text rows when the head is the dense one)
void lmv3_carve(const mhip_layoutlmv3* m, Carver& ws, const mhip_crop_desc* pages, int n_pages, int n, int task, bool want_logits,
                Lmv3Run* r) {
  const mhip_layoutlmv3_config& c = m->cfg;
  const size_t es = m->esz(), D = c.hidden, R = (size_t)n * m->npad(), S = c.input_size, NPAT = m->n_vis() - 1, K0 = 3 * c.patch * c.patch;
  r->resized = ws.take<uint8_t>((size_t)n_pages * S * S * 3);
  r->frag_bytes = mhip_pil_resize_fragments_scratch(pages, n_pages, c.input_size, c.input_size, m->resample);
  r->frag_scratch = ws.take(r->frag_bytes);
  r->tok = ws.take<int>((size_t)n * c.max_text * 8 * 4);
  r->win_page = ws.take<int>((size_t)n * 4);
  r->qcode = ws.take<uint32_t>((R + ATTN_SLACK_ROWS) * 4);
  r->kcode = ws.take<uint32_t>((R + ATTN_SLACK_ROWS) * 4);
  r->pe = ws.take<float>((size_t)n_pages * NPAT * D * 4);
  r->h = ws.take<float>(R * D * 4);
  r->y = ws.take<float>(R * D * 4);
  const size_t TR = (size_t)n * c.max_text;      // text rows
  if (task == TASK_CLASSIFY) {
    r->logits = ws.take<float>((size_t)n * c.num_labels * 4);
  } else {
    r->labels = ws.take<int>(TR * 4);
    r->scores = ws.take<float>(TR * 4);
    r->logits = want_logits ? ws.take<float>(TR * c.num_labels * 4) : nullptr;
    r->dense = m->head == HEAD_DENSE ? ws.take<float>(TR * D * 4) : nullptr;
  }
  encoder_ws_carve(ws, R, D, c.ffn, K0, es, &r->w);
}

// token ids / boxes / mask of n pages -> the embedding kernel's gather rows and the attention codes (host)
int lmv3_prepare(mhip_layoutlmv3* m, int n, const int32_t* ids, const int32_t* bbox, const int32_t* mask, std::vector<int>& tok,
                 std::vector<uint32_t>& qcode, std::vector<uint32_t>& kcode) {
  const mhip_layoutlmv3_config& c = m->cfg;
  const int T = c.max_text, NP = m->npad(), G = m->grid(), NV = m->n_vis(), M2 = c.max_2d_position_embeddings;
  const uint32_t masked = (uint32_t)(2 * m->dp() + 1);
  tok.assign((size_t)n * T * 8, 0);
  qcode.assign((size_t)n * NP + ATTN_SLACK_ROWS, 0);
  kcode.assign((size_t)n * NP + ATTN_SLACK_ROWS, masked);
  for (int p = 0; p < n; ++p) {
    int seen = 0;
    for (int t = 0; t < T; ++t) {
      const size_t e = (size_t)p * T + t;
      const int id = ids[e];
      const int32_t* b = bbox + e * 4;
      if (id < 0 || id >= c.vocab) return mhip_fail(m->ctx, MHIP_EINVAL, "layoutlmv3: token id %d outside the vocabulary (page %d, token %d)", id, p, t);
      for (int j = 0; j < 4; ++j)
        if (b[j] < 0 || b[j] >= M2)
          return mhip_fail(m->ctx, MHIP_EINVAL, "layoutlmv3: box coordinate %d outside [0, %d) (page %d, token %d)", b[j], M2, p, t);
      int pid = c.pad_id;
      if (id != c.pad_id) pid += ++seen;
      if (pid >= c.max_position_embeddings) return mhip_fail(m->ctx, MHIP_EINVAL, "layoutlmv3: position id %d beyond the table", pid);
      int* tk = &tok[e * 8];
      tk[0] = id; tk[1] = pid; tk[2] = b[0]; tk[3] = b[1]; tk[4] = b[2]; tk[5] = b[3];
      tk[6] = std::min(std::max(b[3] - b[1], 0), M2 - 1);
      tk[7] = std::min(std::max(b[2] - b[0], 0), M2 - 1);
      const uint32_t xy = ((uint32_t)b[0] << 12) | ((uint32_t)b[3] << 22);
      qcode[(size_t)p * NP + t] = (uint32_t)t | xy;
      kcode[(size_t)p * NP + t] = (mask[e] ? (uint32_t)t : masked) | xy;
    }
    // LayoutLMv3Model.create_visual_bbox: cls box [1, 1, 999, 999], then the G x G grid on 0..1000 (x0, y1 matter here)
    for (int v = 0; v < NV; ++v) {
      int x0 = 1, y1 = 999;
      if (v > 0) { x0 = 1000 * ((v - 1) % G) / G; y1 = 1000 * ((v - 1) / G + 1) / G; }
      const uint32_t code = (uint32_t)v | ((uint32_t)x0 << 12) | ((uint32_t)y1 << 22);
      qcode[(size_t)p * NP + T + v] = code;
      kcode[(size_t)p * NP + T + v] = code;
    }
  }
  return MHIP_OK;
}

// pages already resized in run.resized; codes and the window -> page map staged -> hidden states of n windows in run.h / run.w.ht
int lmv3_forward(mhip_layoutlmv3* m, int n_pages, int n, const Lmv3Run& run) {
  mhip_ctx* ctx = m->ctx;
  const mhip_layoutlmv3_config& c = m->cfg;
  const int D = c.hidden, F = c.ffn, prec = m->precision, NP = m->npad(), G = m->grid(), P = c.patch, S = c.input_size;
  const size_t es = m->esz(), R = (size_t)n * NP;
  const Arena& a = m->arena;
  const EncoderWs& w = run.w;
  int rc;
  if ((rc = encoder_ws_clear_slack(ctx, w, R, D, es))) return rc;
  // (x / 255 - 0.5) / 0.5 -> 16 x 16 patches -> projection + bias + position rows 1.. (row q takes position row q % G^2)
  const int K0 = 3 * P * P, np = G * G;
  if ((rc = mhip_launch_patchify(ctx, prec, run.resized, n_pages, S, S, G, G, P, 0, 127.5f, 127.5f, w.hid, K0))) return rc;
  {
    ConvDesc cd;
    cd.in = w.hid; cd.w = a.d("pe_w"); cd.bias = a.d<float>("pe_b"); cd.out = run.pe; cd.res = a.d<float>("pos_vis");
    cd.B = 1; cd.H = 1; cd.W = n_pages * np; cd.Cin = K0; cd.N = D; cd.out_f32 = 1;
    cd.row_period = np; cd.row_stride = np; cd.row_offset = 0;
    if ((rc = mhip_launch_conv_igemm(ctx, prec, cd))) return rc;
  }
  Lmv3EmbedDesc e;
  e.tok = run.tok; e.win_page = run.win_page; e.word = a.d("word"); e.type0 = a.d<float>("type0"); e.pos = a.d<float>("pos");
  e.xe = a.d<float>("xe"); e.ye = a.d<float>("ye"); e.he = a.d<float>("he"); e.we = a.d<float>("we");
  e.g_text = a.d<float>("ln_text_g"); e.b_text = a.d<float>("ln_text_b");
  e.patches = run.pe; e.cls = a.d<float>("cls");
  e.g_vis = a.d<float>("ln_vis_g"); e.b_vis = a.d<float>("ln_vis_b");
  e.g_all = a.d<float>("ln_all_g"); e.b_all = a.d<float>("ln_all_b");
  e.h = run.h; e.ht = w.ht;
  e.pages = n; e.max_text = c.max_text; e.n_vis = m->n_vis(); e.npad = NP; e.D = D; e.coord = c.coordinate_size; e.shape = c.shape_size;
  e.eps = c.layer_norm_eps; e.eps_vis = 1e-6f;      // LayoutLMv3Model.norm = nn.LayerNorm(hidden, eps=1e-6)
  if ((rc = mhip_launch_lmv3_embed(ctx, prec, e))) return rc;

  AttnBiasDesc ad;
  ad.a = encoder_attn_desc(w.qk, w.vt, w.ao, D, es, n, c.heads, NP, m->seq());
  ad.qcode = run.qcode; ad.kcode = run.kcode; ad.tab = a.d<float>("bias_tab"); ad.dp = m->dp(); ad.dx = m->dx();
  for (int i = 0; i < c.layers; ++i) {
    if ((rc = encoder_block_attention(ctx, prec, a, i, w, ad))) return rc;
    if ((rc = mhip_gemm(ctx, prec, w.ao, a.d(enc_blk(i, "ao_w")), (long long)R, D, D, nullptr, a.d<float>(enc_blk(i, "ao_b")), run.y, ACT_NONE, 1, run.h))) return rc;
    if ((rc = mhip_launch_layernorm2(ctx, prec, run.y, a.d<float>(enc_blk(i, "ln1_g")), a.d<float>(enc_blk(i, "ln1_b")), run.h, w.ht, (int)R, D, c.layer_norm_eps))) return rc;
    if ((rc = mhip_gemm(ctx, prec, w.ht, a.d(enc_blk(i, "fc1_w")), (long long)R, F, D, nullptr, a.d<float>(enc_blk(i, "fc1_b")), w.hid, ACT_GELU, 0))) return rc;
    if ((rc = mhip_gemm(ctx, prec, w.hid, a.d(enc_blk(i, "fc2_w")), (long long)R, D, F, nullptr, a.d<float>(enc_blk(i, "fc2_b")), run.y, ACT_NONE, 1, run.h))) return rc;
    if ((rc = mhip_launch_layernorm2(ctx, prec, run.y, a.d<float>(enc_blk(i, "ln2_g")), a.d<float>(enc_blk(i, "ln2_b")), run.h, w.ht, (int)R, D, c.layer_norm_eps))) return rc;
  }
  return MHIP_OK;
}

// the head of LayoutLMv3ForSequenceClassification on row 0 of every window -> run.logits
int lmv3_head_rows0(mhip_layoutlmv3* m, int n, const Lmv3Run& run) {
  const Arena& a = m->arena;
  return mhip_launch_lmv3_head(m->ctx, run.h, n, m->npad(), m->cfg.hidden, a.d<float>("cd_w"), a.d<float>("cd_b"), a.d<float>("co_w"),
                               a.d<float>("co_b"), m->cfg.num_labels, run.logits);
}

// the head of LayoutLMv3ForTokenClassification on the text rows of every window (sequence_output[:, :seq_length]) and the
// decision on its logits -> run.labels / run.scores (/ run.logits)
int lmv3_head_tokens(mhip_layoutlmv3* m, int n, const Lmv3Run& run) {
  const mhip_layoutlmv3_config& c = m->cfg;
  const Arena& a = m->arena;
  const int D = c.hidden, T = c.max_text, NP = m->npad();
  int rc;
  TokenHeadDesc t;
  t.w = a.d<float>("co_w"); t.b = a.d<float>("co_b"); t.label = run.labels; t.score = run.scores; t.logits = run.logits;
  t.rows = n * T; t.seg = T; t.D = D; t.L = c.num_labels;
  if (m->head == HEAD_DENSE) {
    // dense on the text rows only, in the model's precision, fp32 out; tanh belongs to the head kernel
    for (int w = 0; w < n; ++w)
      if ((rc = mhip_gemm(m->ctx, m->precision, run.w.ht + (size_t)w * NP * D * m->esz(), a.d("cdt_w"), T, D, D, nullptr, a.d<float>("cd_b"),
                          run.dense + (size_t)w * T * D, ACT_NONE, 1)))
        return rc;
    t.x = run.dense; t.seg_stride = T; t.use_tanh = 1;
  } else {
    t.x = run.h; t.seg_stride = NP; t.use_tanh = 0;
  }
  return mhip_launch_token_head(m->ctx, t);
}

// the head kind of a model whose arena was filled by another rank
int lmv3_head_kind(mhip_layoutlmv3* m) {
  if (m->head >= 0) return MHIP_OK;
  mhip_ctx* ctx = m->ctx;
  int kind = -1;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  MHIP_HIP(ctx, hipMemcpyAsync(&kind, m->arena.d("head_kind"), 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (kind != HEAD_DENSE && kind != HEAD_LINEAR) return mhip_fail(m->ctx, MHIP_ESTATE, "layoutlmv3: the arena holds no weights yet");
  m->head = kind;
  return MHIP_OK;
}

int lmv3_check_call(mhip_layoutlmv3* m, const mhip_crop_desc* pages, int n, const int32_t* ids, const int32_t* bbox,
                    const int32_t* mask, int task) {
  if (!m->ready) return mhip_fail(m->ctx, MHIP_ESTATE, "layoutlmv3: weights not finalized");
  if (!pages || !ids || !bbox || !mask || n < 1 || n > 4096) return mhip_fail(m->ctx, MHIP_EINVAL, "layoutlmv3: bad arguments (n = %d)", n);
  int rc = lmv3_head_kind(m);
  if (rc) return rc;
  if (task == TASK_CLASSIFY && m->head != HEAD_DENSE)
    return mhip_fail(m->ctx, MHIP_ESTATE, "layoutlmv3: the weights hold the linear token head (classifier.weight): no sequence classification");
  // the row-0 head serves any label count; only the token head has a limit, so it is checked where the task is known
  if (task == TASK_TAG && m->cfg.num_labels > mhip_token_head_max_labels(m->cfg.hidden))
    return mhip_fail(m->ctx, MHIP_EINVAL, "layoutlmv3: num_labels %d beyond the %d the token head covers at hidden %d", m->cfg.num_labels,
                     mhip_token_head_max_labels(m->cfg.hidden), m->cfg.hidden);
  return MHIP_OK;
}

int lmv3_check_pages(mhip_layoutlmv3* m, const mhip_crop_desc* pages, int n_pages, size_t pages_bytes) {
  for (int i = 0; i < n_pages; ++i)
    if (pages[i].h < 1 || pages[i].w < 1 || pages[i].row_stride < pages[i].w * 3 ||
        pages[i].src_offset + (size_t)(pages[i].h - 1) * pages[i].row_stride + (size_t)pages[i].w * 3 > pages_bytes)
      return mhip_fail(m->ctx, MHIP_EINVAL, "layoutlmv3: page %d lies outside the buffer", i);
  return MHIP_OK;
}

// the window -> page map of a tag call: every window names one of the n_pages pages
int lmv3_check_windows(mhip_layoutlmv3* m, const int32_t* window_page, int n_win, int n_pages, std::vector<int>& map) {
  if (!window_page || n_pages < 1 || n_pages > n_win) return mhip_fail(m->ctx, MHIP_EINVAL, "layoutlmv3: %d pages for %d windows", n_pages, n_win);
  map.assign(window_page, window_page + n_win);
  for (int w = 0; w < n_win; ++w)
    if (map[w] < 0 || map[w] >= n_pages) return mhip_fail(m->ctx, MHIP_EINVAL, "layoutlmv3: window %d names page %d of %d", w, map[w], n_pages);
  return MHIP_OK;
}

// resize + stage the host tables + forward + the task's head; the caller has carved `run`
int lmv3_run(mhip_layoutlmv3* m, const uint8_t* base_dev, const mhip_crop_desc* pages, int n_pages, const std::vector<int>& win_page,
             const std::vector<int>& tok, const std::vector<uint32_t>& qcode, const std::vector<uint32_t>& kcode, int task,
             const Lmv3Run& run) {
  mhip_ctx* ctx = m->ctx;
  const int S = m->cfg.input_size, n = (int)win_page.size();
  int rc = mhip_pil_resize_fragments(ctx, base_dev, pages, n_pages, run.resized, S, S, m->resample, run.frag_scratch, run.frag_bytes);
  if (rc) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.tok, tok.data(), tok.size() * 4))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.win_page, win_page.data(), win_page.size() * 4))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.qcode, qcode.data(), qcode.size() * 4))) return rc;
  if ((rc = mhip_stage_h2d(ctx, run.kcode, kcode.data(), kcode.size() * 4))) return rc;
  if ((rc = lmv3_forward(m, n_pages, n, run))) return rc;
  return task == TASK_CLASSIFY ? lmv3_head_rows0(m, n, run) : lmv3_head_tokens(m, n, run);
}

std::vector<int> lmv3_identity(int n) {
  std::vector<int> v(n);
  for (int i = 0; i < n; ++i) v[i] = i;
  return v;
}

// labels / scores (/ logits) of a tag call to the host
int lmv3_tag_out(mhip_layoutlmv3* m, int n_win, const Lmv3Run& run, int32_t* label_out, float* score_out, float* logits_out) {
  mhip_ctx* ctx = m->ctx;
  const size_t TR = (size_t)n_win * m->cfg.max_text;
  MHIP_HIP(ctx, hipMemcpyAsync(label_out, run.labels, TR * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(score_out, run.scores, TR * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (logits_out) MHIP_HIP(ctx, hipMemcpyAsync(logits_out, run.logits, TR * m->cfg.num_labels * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- lifecycle
extern "C" int mhip_layoutlmv3_default_config(mhip_layoutlmv3_config* cfg) {
  if (!cfg) return MHIP_EINVAL;
  mhip_layoutlmv3_config c{};
  c.hidden = 768; c.layers = 12; c.heads = 12; c.ffn = 3072;
  c.vocab = 50265; c.type_vocab = 1;
  c.max_position_embeddings = 514; c.max_2d_position_embeddings = 1024;
  c.coordinate_size = 128; c.shape_size = 128;
  c.input_size = 224; c.patch = 16;
  c.rel_pos_bins = 32; c.max_rel_pos = 128; c.rel_2d_pos_bins = 64; c.max_rel_2d_pos = 256;
  c.layer_norm_eps = 1e-5f; c.pad_id = 1; c.num_labels = 2; c.max_text = 512;
  *cfg = c;
  return MHIP_OK;
}

extern "C" int mhip_layoutlmv3_seq_len(const mhip_layoutlmv3_config* cfg) {
  if (!cfg || cfg->patch < 1) return MHIP_EINVAL;
  const int g = cfg->input_size / cfg->patch;
  return cfg->max_text + g * g + 1;
}

extern "C" int mhip_layoutlmv3_max_token_labels(int hidden) { return mhip_token_head_max_labels(hidden); }

extern "C" int mhip_layoutlmv3_bucket(int relative_position, int num_buckets, int max_distance) {
  return mhip_relative_position_bucket(relative_position, num_buckets, max_distance);
}

extern "C" int mhip_layoutlmv3_create(mhip_ctx* ctx, int precision, const mhip_layoutlmv3_config* cfg, mhip_layoutlmv3** out) {
  if (!ctx || !out || !cfg) return MHIP_EINVAL;
  *out = nullptr;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  const mhip_layoutlmv3_config& c = *cfg;
  if (c.hidden != c.heads * 64 || c.hidden % 256 || c.hidden > 1024 || c.layers < 1 || c.ffn < 64 || c.ffn % 64)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutlmv3: unsupported width (hidden %d, heads %d, ffn %d: heads of 64, hidden a multiple of 256 up to 1024)", c.hidden, c.heads, c.ffn);
  if (c.patch != 16 || c.input_size < 16 || c.input_size % 16)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutlmv3: unsupported image geometry (input %d, patch %d)", c.input_size, c.patch);
  if (c.coordinate_size < 4 || c.shape_size < 4 || c.coordinate_size % 4 || c.shape_size % 4 || 4 * c.coordinate_size + 2 * c.shape_size != c.hidden)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutlmv3: 4 * coordinate_size + 2 * shape_size must equal hidden");
  if (c.max_2d_position_embeddings < 1001 || c.max_2d_position_embeddings > 1024)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutlmv3: max_2d_position_embeddings %d (1001 .. 1024)", c.max_2d_position_embeddings);
  if (c.max_text < 8 || c.max_text > 1024 || c.max_text % 8 || c.pad_id < 0 || c.vocab <= c.pad_id || c.type_vocab < 1 || c.num_labels < 1)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutlmv3: unsupported text geometry (max_text %d, vocab %d, pad %d, labels %d)", c.max_text, c.vocab, c.pad_id, c.num_labels);
  if (c.max_position_embeddings < c.max_text + c.pad_id + 1)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutlmv3: max_position_embeddings %d cannot hold %d unpadded tokens (needs %d)",
                     c.max_position_embeddings, c.max_text, c.max_text + c.pad_id + 1);
  if (c.rel_pos_bins < 4 || c.rel_pos_bins % 4 || c.rel_2d_pos_bins < 4 || c.rel_2d_pos_bins % 4 || c.max_rel_pos <= c.rel_pos_bins / 4 ||
      c.max_rel_2d_pos <= c.rel_2d_pos_bins / 4)
    return mhip_fail(ctx, MHIP_EINVAL, "layoutlmv3: unsupported relative-position buckets");
  if (!(c.layer_norm_eps > 0.f)) return mhip_fail(ctx, MHIP_EINVAL, "layoutlmv3: layer_norm_eps");
  mhip_layoutlmv3* m = new mhip_layoutlmv3();
  m->ctx = ctx;
  m->precision = precision;
  m->cfg = c;
  if (m->dp() > 1023) { delete m; return mhip_fail(ctx, MHIP_EINVAL, "layoutlmv3: more than 1024 positions"); }
  const size_t es = m->esz(), D = c.hidden, F = c.ffn, M2 = c.max_2d_position_embeddings;
  Arena& a = m->arena;
  a.take("word", (size_t)c.vocab * D * es);
  a.take("type0", D * 4);
  a.take("pos", (size_t)c.max_position_embeddings * D * 4);
  a.take("xe", M2 * c.coordinate_size * 4); a.take("ye", M2 * c.coordinate_size * 4);
  a.take("he", M2 * c.shape_size * 4); a.take("we", M2 * c.shape_size * 4);
  a.take("ln_text_g", D * 4); a.take("ln_text_b", D * 4);
  a.take("ln_vis_g", D * 4); a.take("ln_vis_b", D * 4);
  a.take("ln_all_g", D * 4); a.take("ln_all_b", D * 4);
  a.take("pe_w", D * 3 * 16 * 16 * es); a.take("pe_b", D * 4);
  a.take("pos_vis", (size_t)(m->n_vis() - 1) * D * 4);
  a.take("cls", D * 4);
  a.take("bias_tab", (size_t)c.heads * mhip_attn_bias_table_len(m->dp(), m->dx()) * 4);
  for (int i = 0; i < c.layers; ++i) encoder_block_take(a, i, D, F, es);
  // the head: dense (fp32 for the row-0 head, the element type for the token head's GEMM) + out_proj, or — in the out_proj
  // entries — the linear token head; which of the two, for the ranks that receive the arena filled
  a.take("cd_w", D * D * 4); a.take("cd_b", D * 4);
  a.take("co_w", (size_t)c.num_labels * D * 4); a.take("co_b", (size_t)c.num_labels * 4);
  a.take("cdt_w", D * D * es);
  a.take("head_kind", 4);
  *out = m;
  return MHIP_OK;
}

extern "C" int mhip_layoutlmv3_destroy(mhip_layoutlmv3* m) {
  if (!m) return MHIP_OK;
  mhip_quiesce(m->ctx);
  m->arena.release();
  delete m;
  return MHIP_OK;
}

extern "C" int mhip_layoutlmv3_set_resample(mhip_layoutlmv3* m, int filter) {
  if (!m) return MHIP_EINVAL;
  if (!mhip_pil_filter_ok(filter)) return mhip_fail(m->ctx, MHIP_EINVAL, "layoutlmv3: unknown resample filter %d (1 LANCZOS, 2 BILINEAR, 3 BICUBIC)", filter);
  m->resample = filter;
  return MHIP_OK;
}

extern "C" int mhip_layoutlmv3_set_tensor(mhip_layoutlmv3* m, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!m || !key) return MHIP_EINVAL;
  std::string k(key);
  auto ends = [&](const char* s) { const size_t n = strlen(s); return k.size() >= n && k.compare(k.size() - n, n, s) == 0; };
  if (ends("position_ids") || ends("visual_bbox")) return MHIP_OK;      // buffers older checkpoints carry; rebuilt from the config
  if (k.rfind(PFX, 0) != 0 && k.rfind("classifier.", 0) != 0) return mhip_fail(m->ctx, MHIP_EINVAL, "unknown state_dict key %s", key);
  m->ready = false;
  m->head = -1;
  return m->store.set(m->ctx, k, data, shape, ndim);
}

extern "C" int mhip_layoutlmv3_alloc_arena(mhip_layoutlmv3* m) {
  if (!m) return MHIP_EINVAL;
  int rc = m->arena.alloc(m->ctx);
  if (rc) return rc;
  m->head = -1;
  m->ready = true;
  return MHIP_OK;
}

extern "C" int mhip_layoutlmv3_arena(mhip_layoutlmv3* m, void** dev, size_t* bytes) {
  if (!m) return MHIP_EINVAL;
  if (dev) *dev = m->arena.dev;
  if (bytes) *bytes = m->arena.bytes;
  return MHIP_OK;
}

extern "C" int mhip_layoutlmv3_finalize(mhip_layoutlmv3* m) {
  if (!m) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  const mhip_layoutlmv3_config& c = m->cfg;
  const int D = c.hidden, F = c.ffn, prec = m->precision, M2 = c.max_2d_position_embeddings, NV = m->n_vis();
  Arena& a = m->arena;
  const TensorStore& st = m->store;
  a.begin_fill();
  const std::string E = std::string(PFX) + "embeddings.";
  const HostTensor* word = st.find(ctx, E + "word_embeddings.weight", {c.vocab, D});
  const HostTensor* type = st.find(ctx, E + "token_type_embeddings.weight", {c.type_vocab, D});
  const HostTensor* pos = st.find(ctx, E + "position_embeddings.weight", {c.max_position_embeddings, D});
  const HostTensor* xe = st.find(ctx, E + "x_position_embeddings.weight", {M2, c.coordinate_size});
  const HostTensor* ye = st.find(ctx, E + "y_position_embeddings.weight", {M2, c.coordinate_size});
  const HostTensor* he = st.find(ctx, E + "h_position_embeddings.weight", {M2, c.shape_size});
  const HostTensor* we = st.find(ctx, E + "w_position_embeddings.weight", {M2, c.shape_size});
  const HostTensor* ltg = st.find(ctx, E + "LayerNorm.weight", {D});
  const HostTensor* ltb = st.find(ctx, E + "LayerNorm.bias", {D});
  const HostTensor* lag = st.find(ctx, std::string(PFX) + "LayerNorm.weight", {D});
  const HostTensor* lab = st.find(ctx, std::string(PFX) + "LayerNorm.bias", {D});
  const HostTensor* lvg = st.find(ctx, std::string(PFX) + "norm.weight", {D});
  const HostTensor* lvb = st.find(ctx, std::string(PFX) + "norm.bias", {D});
  const HostTensor* pw = st.find(ctx, std::string(PFX) + "patch_embed.proj.weight", {D, 3, 16, 16});
  const HostTensor* pb = st.find(ctx, std::string(PFX) + "patch_embed.proj.bias", {D});
  const HostTensor* cls = st.find(ctx, std::string(PFX) + "cls_token", {1, 1, D});
  const HostTensor* pv = st.find(ctx, std::string(PFX) + "pos_embed", {1, NV, D});
  const HostTensor* r1 = st.find(ctx, std::string(PFX) + "encoder.rel_pos_bias.weight", {c.heads, c.rel_pos_bins});
  const HostTensor* rx = st.find(ctx, std::string(PFX) + "encoder.rel_pos_x_bias.weight", {c.heads, c.rel_2d_pos_bins});
  const HostTensor* ry = st.find(ctx, std::string(PFX) + "encoder.rel_pos_y_bias.weight", {c.heads, c.rel_2d_pos_bins});
  const bool linear = st.t.count("classifier.weight") != 0;
  const HostTensor* cdw = linear ? nullptr : st.find(ctx, "classifier.dense.weight", {D, D});
  const HostTensor* cdb = linear ? nullptr : st.find(ctx, "classifier.dense.bias", {D});
  const HostTensor* cow = st.find(ctx, linear ? "classifier.weight" : "classifier.out_proj.weight", {c.num_labels, D});
  const HostTensor* cob = st.find(ctx, linear ? "classifier.bias" : "classifier.out_proj.bias", {c.num_labels});
  // a linear head serves token tagging only: refuse here what the token head does not cover
  if (linear && c.num_labels > mhip_token_head_max_labels(D))
    return mhip_fail(ctx, MHIP_EINVAL, "layoutlmv3: num_labels %d beyond the %d the token head covers at hidden %d", c.num_labels,
                     mhip_token_head_max_labels(D), D);
  if (linear && st.t.count("classifier.dense.weight")) return mhip_fail(ctx, MHIP_ESTATE, "layoutlmv3: the state holds both classifier.weight and classifier.dense");
  if (!word || !type || !pos || !xe || !ye || !he || !we || !ltg || !ltb || !lag || !lab || !lvg || !lvb || !pw || !pb || !cls ||
      !pv || !r1 || !rx || !ry || (!linear && (!cdw || !cdb)) || !cow || !cob)
    return MHIP_ESTATE;
  Arena::put(prec, a.h("word"), word->data.data(), word->numel());
  memcpy(a.h("type0"), type->data.data(), D * 4);                  // token_type_ids are zeros on this path
  memcpy(a.h("pos"), pos->data.data(), pos->numel() * 4);
  memcpy(a.h("xe"), xe->data.data(), xe->numel() * 4);
  memcpy(a.h("ye"), ye->data.data(), ye->numel() * 4);
  memcpy(a.h("he"), he->data.data(), he->numel() * 4);
  memcpy(a.h("we"), we->data.data(), we->numel() * 4);
  memcpy(a.h("ln_text_g"), ltg->data.data(), D * 4); memcpy(a.h("ln_text_b"), ltb->data.data(), D * 4);
  memcpy(a.h("ln_all_g"), lag->data.data(), D * 4); memcpy(a.h("ln_all_b"), lab->data.data(), D * 4);
  memcpy(a.h("ln_vis_g"), lvg->data.data(), D * 4); memcpy(a.h("ln_vis_b"), lvb->data.data(), D * 4);
  Arena::put(prec, a.h("pe_w"), pw->data.data(), pw->numel());
  memcpy(a.h("pe_b"), pb->data.data(), D * 4);
  memcpy(a.h("pos_vis"), pv->data.data() + D, (size_t)(NV - 1) * D * 4);
  for (int d = 0; d < D; ++d) ((float*)a.h("cls"))[d] = cls->data[d] + pv->data[d];
  // the three bias matrices folded into difference-indexed tables, in the units of the scores (1 / sqrt(64), base-2 exponent)
  mhip_attn_bias_fold(r1->data.data(), rx->data.data(), ry->data.data(), c.heads, c.rel_pos_bins, c.max_rel_pos, c.rel_2d_pos_bins,
                      c.max_rel_2d_pos, m->dp(), m->dx(), ATTN_SCORE_SCALE, (float*)a.h("bias_tab"));
  for (int i = 0; i < c.layers; ++i) {
    const HostTensor* qw = st.find(ctx, lyr(i, "attention.self.query.weight"), {D, D});
    const HostTensor* qb = st.find(ctx, lyr(i, "attention.self.query.bias"), {D});
    const HostTensor* kw = st.find(ctx, lyr(i, "attention.self.key.weight"), {D, D});
    const HostTensor* kb = st.find(ctx, lyr(i, "attention.self.key.bias"), {D});
    const HostTensor* vw = st.find(ctx, lyr(i, "attention.self.value.weight"), {D, D});
    const HostTensor* vb = st.find(ctx, lyr(i, "attention.self.value.bias"), {D});
    const HostTensor* ow = st.find(ctx, lyr(i, "attention.output.dense.weight"), {D, D});
    const HostTensor* ob = st.find(ctx, lyr(i, "attention.output.dense.bias"), {D});
    const HostTensor* g1 = st.find(ctx, lyr(i, "attention.output.LayerNorm.weight"), {D});
    const HostTensor* b1 = st.find(ctx, lyr(i, "attention.output.LayerNorm.bias"), {D});
    const HostTensor* iw = st.find(ctx, lyr(i, "intermediate.dense.weight"), {F, D});
    const HostTensor* ib = st.find(ctx, lyr(i, "intermediate.dense.bias"), {F});
    const HostTensor* dw = st.find(ctx, lyr(i, "output.dense.weight"), {D, F});
    const HostTensor* db = st.find(ctx, lyr(i, "output.dense.bias"), {D});
    const HostTensor* g2 = st.find(ctx, lyr(i, "output.LayerNorm.weight"), {D});
    const HostTensor* b2 = st.find(ctx, lyr(i, "output.LayerNorm.bias"), {D});
    if (!qw || !qb || !kw || !kb || !vw || !vb || !ow || !ob || !g1 || !b1 || !iw || !ib || !dw || !db || !g2 || !b2) return MHIP_ESTATE;
    EncoderBlockWeights w;      // post-LN: ln1 follows the attention, ln2 the MLP
    w.wq = qw->data.data(); w.wk = kw->data.data(); w.wv = vw->data.data();
    w.bq = qb->data.data(); w.bk = kb->data.data(); w.bv = vb->data.data();
    w.wo = ow->data.data(); w.bo = ob->data.data();
    w.ln1_g = g1->data.data(); w.ln1_b = b1->data.data(); w.ln2_g = g2->data.data(); w.ln2_b = b2->data.data();
    w.w1 = iw->data.data(); w.b1 = ib->data.data(); w.w2 = dw->data.data(); w.b2 = db->data.data();
    encoder_block_fill(a, prec, i, D, F, w);
  }
  if (!linear) {
    memcpy(a.h("cd_w"), cdw->data.data(), cdw->numel() * 4); memcpy(a.h("cd_b"), cdb->data.data(), D * 4);
    Arena::put(prec, a.h("cdt_w"), cdw->data.data(), cdw->numel());
  }
  const int kind = linear ? HEAD_LINEAR : HEAD_DENSE;
  memcpy(a.h("head_kind"), &kind, 4);
  memcpy(a.h("co_w"), cow->data.data(), cow->numel() * 4); memcpy(a.h("co_b"), cob->data.data(), (size_t)c.num_labels * 4);
  int rc = a.upload(ctx);
  if (rc) return rc;
  m->head = kind;
  m->ready = true;
  m->store.t.clear();
  return MHIP_OK;
}

// ---------------------------------------------------------------------------------------------------- forward
extern "C" int mhip_layoutlmv3_classify(mhip_layoutlmv3* m, const uint8_t* base_dev, const mhip_crop_desc* pages, int n,
                                        const int32_t* ids, const int32_t* bbox, const int32_t* mask, float* logits_out) {
  if (!m || !base_dev || !logits_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = lmv3_check_call(m, pages, n, ids, bbox, mask, TASK_CLASSIFY);
  if (rc) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<int> tok;
  std::vector<uint32_t> qcode, kcode;
  if ((rc = lmv3_prepare(m, n, ids, bbox, mask, tok, qcode, kcode))) return rc;
  Lmv3Run run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { lmv3_carve(m, ws, pages, n, n, TASK_CLASSIFY, false, &run); }))) return rc;
  if ((rc = lmv3_run(m, base_dev, pages, n, lmv3_identity(n), tok, qcode, kcode, TASK_CLASSIFY, run))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(logits_out, run.logits, (size_t)n * m->cfg.num_labels * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_layoutlmv3_hidden_host(mhip_layoutlmv3* m, const uint8_t* pages_host, size_t pages_bytes,
                                           const mhip_crop_desc* pages, int n, const int32_t* ids, const int32_t* bbox,
                                           const int32_t* mask, float* logits_out, float* hidden_out, uint8_t* resized_out) {
  if (!m || !pages_host || !pages_bytes) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = lmv3_check_call(m, pages, n, ids, bbox, mask, TASK_CLASSIFY);
  if (rc) return rc;
  if ((rc = lmv3_check_pages(m, pages, n, pages_bytes))) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<int> tok;
  std::vector<uint32_t> qcode, kcode;
  if ((rc = lmv3_prepare(m, n, ids, bbox, mask, tok, qcode, kcode))) return rc;
  Lmv3Run run;
  uint8_t* base = nullptr;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
         base = ws.take<uint8_t>(pages_bytes);
         lmv3_carve(m, ws, pages, n, n, TASK_CLASSIFY, false, &run);
       })))
    return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(base, pages_host, pages_bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = lmv3_run(m, base, pages, n, lmv3_identity(n), tok, qcode, kcode, TASK_CLASSIFY, run))) return rc;
  const size_t D = m->cfg.hidden, S = m->cfg.input_size, seq = m->seq(), NP = m->npad();
  if (logits_out) MHIP_HIP(ctx, hipMemcpyAsync(logits_out, run.logits, (size_t)n * m->cfg.num_labels * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (hidden_out)
    MHIP_HIP(ctx, hipMemcpy2DAsync(hidden_out, seq * D * 4, run.h, NP * D * 4, seq * D * 4, n, hipMemcpyDeviceToHost, ctx->stream));
  if (resized_out) MHIP_HIP(ctx, hipMemcpyAsync(resized_out, run.resized, (size_t)n * S * S * 3, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

// ---------------------------------------------------------------------------------------------------- token tagging
extern "C" int mhip_layoutlmv3_tag(mhip_layoutlmv3* m, const uint8_t* base_dev, const mhip_crop_desc* pages, int n_pages,
                                   const int32_t* window_page, int n_win, const int32_t* ids, const int32_t* bbox,
                                   const int32_t* mask, int32_t* label_out, float* score_out, float* logits_out) {
  if (!m || !base_dev || !label_out || !score_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = lmv3_check_call(m, pages, n_win, ids, bbox, mask, TASK_TAG);
  if (rc) return rc;
  std::vector<int> map, tok;
  std::vector<uint32_t> qcode, kcode;
  if ((rc = lmv3_check_windows(m, window_page, n_win, n_pages, map))) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = lmv3_prepare(m, n_win, ids, bbox, mask, tok, qcode, kcode))) return rc;
  Lmv3Run run;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) { lmv3_carve(m, ws, pages, n_pages, n_win, TASK_TAG, logits_out != nullptr, &run); })))
    return rc;
  if ((rc = lmv3_run(m, base_dev, pages, n_pages, map, tok, qcode, kcode, TASK_TAG, run))) return rc;
  return lmv3_tag_out(m, n_win, run, label_out, score_out, logits_out);
}

extern "C" int mhip_layoutlmv3_tag_host(mhip_layoutlmv3* m, const uint8_t* pages_host, size_t pages_bytes,
                                        const mhip_crop_desc* pages, int n_pages, const int32_t* window_page, int n_win,
                                        const int32_t* ids, const int32_t* bbox, const int32_t* mask, int32_t* label_out,
                                        float* score_out, float* logits_out) {
  if (!m || !pages_host || !pages_bytes || !label_out || !score_out) return MHIP_EINVAL;
  mhip_ctx* ctx = m->ctx;
  int rc = lmv3_check_call(m, pages, n_win, ids, bbox, mask, TASK_TAG);
  if (rc) return rc;
  std::vector<int> map, tok;
  std::vector<uint32_t> qcode, kcode;
  if ((rc = lmv3_check_windows(m, window_page, n_win, n_pages, map))) return rc;
  if ((rc = lmv3_check_pages(m, pages, n_pages, pages_bytes))) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = lmv3_prepare(m, n_win, ids, bbox, mask, tok, qcode, kcode))) return rc;
  Lmv3Run run;
  uint8_t* base = nullptr;
  if ((rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
         base = ws.take<uint8_t>(pages_bytes);
         lmv3_carve(m, ws, pages, n_pages, n_win, TASK_TAG, logits_out != nullptr, &run);
       })))
    return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(base, pages_host, pages_bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = lmv3_run(m, base, pages, n_pages, map, tok, qcode, kcode, TASK_TAG, run))) return rc;
  return lmv3_tag_out(m, n_win, run, label_out, score_out, logits_out);
}

// ---------------------------------------------------------------------------------------------------- the token head alone
extern "C" int mhip_token_head_host(mhip_ctx* ctx, int precision, int rows, int D, int L, const float* hidden, const float* dense_w,
                                    const float* dense_b, const float* out_w, const float* out_b, int32_t* label_out,
                                    float* score_out, float* logits_out) {
  if (!ctx || !hidden || !out_w || !out_b || !label_out || !score_out || (dense_w == nullptr) != (dense_b == nullptr)) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (rows < 1 || rows > (1 << 20) || D < 256 || D % 256 || D > 1024 || L < 1 || L > mhip_token_head_max_labels(D))
    return mhip_fail(ctx, MHIP_EINVAL, "token_head: rows=%d D=%d labels=%d (D a multiple of 256 up to 1024, at most %d labels)", rows, D, L,
                     D >= 256 ? mhip_token_head_max_labels(D) : 0);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t es = precision == MHIP_PREC_F16 ? 2 : 4, RD = (size_t)rows * D;
  const bool dense = dense_w != nullptr;
  float *dx = nullptr, *dy = nullptr, *dob = nullptr, *dow = nullptr, *ddb = nullptr, *dscore = nullptr, *dlogits = nullptr;
  char *dxt = nullptr, *ddw = nullptr;
  int* dlabel = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dow = ws.take<float>((size_t)L * D * 4); dob = ws.take<float>((size_t)L * 4);
    dlabel = ws.take<int>((size_t)rows * 4); dscore = ws.take<float>((size_t)rows * 4);
    dlogits = logits_out ? ws.take<float>((size_t)rows * L * 4) : nullptr;
    if (dense) {
      dxt = ws.take((RD + 128 * (size_t)D) * es); ddw = ws.take((size_t)D * D * es); ddb = ws.take<float>((size_t)D * 4);
      dy = ws.take<float>(RD * 4);
    } else {
      dx = ws.take<float>(RD * 4);
    }
  });
  if (rc) return rc;
  std::vector<char> xt, wt;
  if (dense) {      // the GEMM's operands in the element type, as the model holds them
    xt.resize(RD * es); wt.resize((size_t)D * D * es);
    Arena::put(precision, xt.data(), hidden, RD);
    Arena::put(precision, wt.data(), dense_w, (size_t)D * D);
    MHIP_HIP(ctx, hipMemcpyAsync(dxt, xt.data(), xt.size(), hipMemcpyHostToDevice, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(ddw, wt.data(), wt.size(), hipMemcpyHostToDevice, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(ddb, dense_b, (size_t)D * 4, hipMemcpyHostToDevice, ctx->stream));
  } else {
    MHIP_HIP(ctx, hipMemcpyAsync(dx, hidden, RD * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  MHIP_HIP(ctx, hipMemcpyAsync(dow, out_w, (size_t)L * D * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dob, out_b, (size_t)L * 4, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the sources are host temporaries in pageable memory
  if (dense && (rc = mhip_gemm(ctx, precision, dxt, ddw, rows, D, D, nullptr, ddb, dy, ACT_NONE, 1))) return rc;
  TokenHeadDesc t;
  t.x = dense ? dy : dx; t.w = dow; t.b = dob; t.label = dlabel; t.score = dscore; t.logits = dlogits;
  t.rows = rows; t.seg = rows; t.seg_stride = rows; t.D = D; t.L = L; t.use_tanh = dense ? 1 : 0;
  if ((rc = mhip_launch_token_head(ctx, t))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(label_out, dlabel, (size_t)rows * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(score_out, dscore, (size_t)rows * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (logits_out) MHIP_HIP(ctx, hipMemcpyAsync(logits_out, dlogits, (size_t)rows * L * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

// ---------------------------------------------------------------------------------------------------- the attention kernels alone
static_assert(MHIP_ATTN_SLACK_ROWS == ATTN_SLACK_ROWS, "the header's slack is the kernel's");

// One mhip_launch_attention / mhip_launch_attention_bias on caller-supplied host operands, every row of them the caller's (see
// include/marie_hip.h).  The shape is judged by the launcher alone; what is checked here is what this entry's own buffers and
// the packing of the codes need.
extern "C" int mhip_attention_host(mhip_ctx* ctx, const mhip_attention_host_desc* hd) {
  if (!ctx) return MHIP_EINVAL;
  if (!hd || !hd->q || !hd->k || !hd->vt || !hd->out) return mhip_fail(ctx, MHIP_EINVAL, "attention_host: null operand");
  const mhip_attention_host_desc& h = *hd;
  if (h.precision != MHIP_PREC_F16 && h.precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", h.precision);
  if (h.layout != MHIP_ATTN_LAYOUT_FUSED && h.layout != MHIP_ATTN_LAYOUT_SPLIT)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_host: unknown layout %d", h.layout);
  if (h.layout == MHIP_ATTN_LAYOUT_FUSED && h.npad_q != h.npad_k)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_host: the fused layout has one row pitch (npad_q %d, npad_k %d)", h.npad_q, h.npad_k);
  if (h.images < 0 || h.heads < 0 || h.heads > 64 || h.npad_q < 0 || h.npad_k < 0 || h.npad_q > 65536 || h.npad_k > 65536 || h.images > 4096)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_host: images %d, heads %d, npad %d / %d", h.images, h.heads, h.npad_q, h.npad_k);
  const bool biased = h.w1 != nullptr;
  const size_t es = h.precision == MHIP_PREC_F16 ? 2 : 4, D = (size_t)h.heads * 64;
  const size_t Rq = (size_t)h.images * h.npad_q + ATTN_SLACK_ROWS, Rk = (size_t)h.images * h.npad_k + ATTN_SLACK_ROWS;
  const size_t nvt = D * h.images * h.npad_k + ATTN_SLACK_ROWS;
  std::vector<uint32_t> qcode, kcode;
  std::vector<float> tab;
  if (biased) {
    if (!h.wx || !h.wy || !h.qcode || !h.kcode) return mhip_fail(ctx, MHIP_EINVAL, "attention_host: null bias operand");
    if (h.bins_1d < 4 || h.bins_1d % 4 || h.bins_2d < 4 || h.bins_2d % 4 || h.max_1d <= h.bins_1d / 4 || h.max_2d <= h.bins_2d / 4 ||
        h.dp < 0 || h.dx < 0 || h.dp > 65536 || h.dx > 65536)
      return mhip_fail(ctx, MHIP_EINVAL, "attention_host: bad bias arguments");
    // a code outside its table would be read outside it: pos | x << 12 | y << 22, a masked key's pos = 2 dp + 1
    qcode.resize(Rq); kcode.resize(Rk);
    auto pack = [&](const int32_t* c, bool valid, uint32_t* dst) {
      if (c[0] < 0 || c[0] > h.dp || c[1] < 0 || c[1] > h.dx || c[2] < 0 || c[2] > h.dx) return false;
      *dst = (valid ? (uint32_t)c[0] : (uint32_t)(2 * h.dp + 1)) | ((uint32_t)c[1] << 12) | ((uint32_t)c[2] << 22);
      return true;
    };
    for (size_t r = 0; r < Rq; ++r)
      if (!pack(h.qcode + 3 * r, true, &qcode[r])) return mhip_fail(ctx, MHIP_EINVAL, "attention_host: code of query row %zu outside [0, dp] / [0, dx]", r);
    for (size_t r = 0; r < Rk; ++r)
      if (!pack(h.kcode + 4 * r, h.kcode[4 * r + 3] != 0, &kcode[r])) return mhip_fail(ctx, MHIP_EINVAL, "attention_host: code of key row %zu outside [0, dp] / [0, dx]", r);
    tab.resize(D / 64 * mhip_attn_bias_table_len(h.dp, h.dx));
    mhip_attn_bias_fold(h.w1, h.wx, h.wy, h.heads, h.bins_1d, h.max_1d, h.bins_2d, h.max_2d, h.dp, h.dx, ATTN_SCORE_SCALE, tab.data());
  }
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  // operands in the element type: q | k rows of pitch 2 D (fused) or q rows then k rows of pitch D (split); V^T as it came
  const bool fused = h.layout == MHIP_ATTN_LAYOUT_FUSED;
  const size_t ldq = fused ? 2 * D : D, koff = fused ? D : Rq * D;
  std::vector<char> qk((Rq + Rk) * D * es), vt(nvt * es);
  auto put = [&](char* dst, size_t at, float val) {
    if (es == 2) ((_Float16*)dst)[at] = (_Float16)val; else ((float*)dst)[at] = val;
  };
  for (size_t r = 0; r < Rq; ++r)
    for (size_t d = 0; d < D; ++d) put(qk.data(), r * ldq + d, h.q[r * D + d]);
  for (size_t r = 0; r < Rk; ++r)
    for (size_t d = 0; d < D; ++d) put(qk.data(), koff + r * ldq + d, h.k[r * D + d]);
  for (size_t i = 0; i < nvt; ++i) put(vt.data(), i, h.vt[i]);
  const size_t out_bytes = Rq * D * es;
  char *dqk = nullptr, *dvt = nullptr, *dao = nullptr;
  uint32_t *dqc = nullptr, *dkc = nullptr;
  float* dtab = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dqk = ws.take(qk.size()); dvt = ws.take(vt.size()); dao = ws.take(out_bytes);
    dqc = ws.take<uint32_t>(qcode.size() * 4); dkc = ws.take<uint32_t>(kcode.size() * 4);
    dtab = ws.take<float>(tab.size() * 4);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dqk, qk.data(), qk.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dvt, vt.data(), vt.size(), hipMemcpyHostToDevice, ctx->stream));
  if (biased) {
    MHIP_HIP(ctx, hipMemcpyAsync(dqc, qcode.data(), qcode.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(dkc, kcode.data(), kcode.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(dtab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  MHIP_HIP(ctx, hipMemsetAsync(dao, 0xff, out_bytes, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the sources are host temporaries in pageable memory
  AttnBiasDesc ad;
  if (fused) {
    ad.a = encoder_attn_desc(dqk, dvt, dao, (int)D, es, h.images, h.heads, h.npad_k, h.n_keys);
    ad.a.n_queries = h.n_queries;
  } else {
    ad.a.q = dqk; ad.a.k = dqk + koff * es; ad.a.vt = dvt; ad.a.out = dao;
    ad.a.ldq = ad.a.ldk = ad.a.ldo = (int)D; ad.a.ldv = h.images * h.npad_k;
    ad.a.images = h.images; ad.a.heads = h.heads; ad.a.npad_q = h.npad_q; ad.a.npad_k = h.npad_k;
    ad.a.n_queries = h.n_queries; ad.a.n_keys = h.n_keys;
  }
  ad.qcode = dqc; ad.kcode = dkc; ad.tab = dtab; ad.dp = h.dp; ad.dx = h.dx;
  if ((rc = biased ? mhip_launch_attention_bias(ctx, h.precision, ad) : mhip_launch_attention(ctx, h.precision, ad.a))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(h.out, dao, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

// The biased kernel at the model's layout: one image of ceil8(n_tok) rows, zero padding and slack, the padding keys masked, dp / dx
// the largest position / coordinate.  A wrapper of mhip_attention_host.
extern "C" int mhip_attention_bias_host(mhip_ctx* ctx, int precision, int heads, int n_tok, const float* q, const float* k,
                                        const float* v, const int32_t* pos, const int32_t* x, const int32_t* y,
                                        const int32_t* valid, const float* w1, const float* wx, const float* wy, int bins_1d,
                                        int max_1d, int bins_2d, int max_2d, float* out) {
  if (!ctx || !q || !k || !v || !pos || !x || !y || !valid || !w1 || !wx || !wy || !out) return MHIP_EINVAL;
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  if (heads < 1 || heads > 64 || n_tok < 1 || n_tok > 65536 || bins_1d < 4 || bins_1d % 4 || bins_2d < 4 || bins_2d % 4 ||
      max_1d <= bins_1d / 4 || max_2d <= bins_2d / 4)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_bias: bad arguments");
  int dp = 0, dx = 0;
  for (int i = 0; i < n_tok; ++i) {
    if (pos[i] < 0 || pos[i] > 1023 || x[i] < 0 || x[i] > 1023 || y[i] < 0 || y[i] > 1023)
      return mhip_fail(ctx, MHIP_EINVAL, "attention_bias: position / coordinate of token %d outside [0, 1023]", i);
    dp = std::max(dp, pos[i]);
    dx = std::max(dx, std::max(x[i], y[i]));
  }
  const size_t D = (size_t)heads * 64, NP = ((size_t)n_tok + 7) / 8 * 8, R = NP + ATTN_SLACK_ROWS;
  std::vector<float> hq(R * D, 0.f), hk(R * D, 0.f), hvt(D * NP + ATTN_SLACK_ROWS, 0.f);
  for (size_t t = 0; t < (size_t)n_tok; ++t)
    for (size_t d = 0; d < D; ++d) {
      hq[t * D + d] = q[t * D + d] * ATTN_SCORE_SCALE;
      hk[t * D + d] = k[t * D + d];
      hvt[d * NP + t] = v[t * D + d];
    }
  std::vector<int32_t> qcode(R * 3, 0), kcode(R * 4, 0);      // rows behind the tokens: code 0, masked as keys
  for (int t = 0; t < n_tok; ++t) {
    qcode[3 * t] = kcode[4 * t] = pos[t];
    qcode[3 * t + 1] = kcode[4 * t + 1] = x[t];
    qcode[3 * t + 2] = kcode[4 * t + 2] = y[t];
    kcode[4 * t + 3] = valid[t] != 0;
  }
  const bool is16 = precision == MHIP_PREC_F16;
  std::vector<char> raw(R * D * (is16 ? 2 : 4));
  mhip_attention_host_desc hd{};
  hd.precision = precision; hd.layout = MHIP_ATTN_LAYOUT_FUSED;
  hd.images = 1; hd.heads = heads; hd.n_queries = hd.n_keys = n_tok; hd.npad_q = hd.npad_k = (int)NP;
  hd.q = hq.data(); hd.k = hk.data(); hd.vt = hvt.data(); hd.qcode = qcode.data(); hd.kcode = kcode.data();
  hd.w1 = w1; hd.wx = wx; hd.wy = wy; hd.bins_1d = bins_1d; hd.max_1d = max_1d; hd.bins_2d = bins_2d; hd.max_2d = max_2d;
  hd.dp = dp; hd.dx = dx; hd.out = raw.data();
  const int rc = mhip_attention_host(ctx, &hd);
  if (rc) return rc;
  for (size_t i = 0; i < (size_t)n_tok * D; ++i) out[i] = is16 ? (float)((const _Float16*)raw.data())[i] : ((const float*)raw.data())[i];
  return MHIP_OK;
}
