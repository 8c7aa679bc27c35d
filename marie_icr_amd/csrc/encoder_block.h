// encoder_block.h — the transformer encoder layer the ViT (vit_api.hip), LayoutLMv3 (layoutlmv3_api.hip), CLIP (clip_api.hip,
// cliptext_api.hip) and BERT (berttext_api.hip) towers share, host side: its arena entries and how the checkpoint's weights are packed into them, its workspace, and the
// attention half of a layer
//   q|k = ht Wqk^T + b        V^T = Wv ht^T        ao = attention(q, k, V^T)
// The LayerNorms, the residual wiring and the MLP activation differ between the towers and stay in the model files; the two
// CLIP towers agree on them too (pre-LN, quick-GELU, fp32 stream) and share clip_encoder_layers below.
#pragma once
#include "weights_util.h"

// head_dim^-0.5 (64 -> 1/8) and the exp -> exp2 change of base: attn_flash.hip takes its scores in these units, so the factor is
// folded into W_q and b_q (and into LayoutLMv3's bias tables)
constexpr float ATTN_SCORE_SCALE = 0.125f * 1.4426950408889634f;

inline std::string enc_blk(int i, const char* s) { return "l" + std::to_string(i) + "." + s; }

// the entries of block i every tower has (D: width, F: MLP width, es: bytes of a GEMM element).  gated: fc1 is the doubled,
// bias-free matrix of a gated MLP ([2 F][D]: the activated half, then the linear half) and there is no fc1_b entry
inline void encoder_block_take(Arena& a, int i, size_t D, size_t F, size_t es, bool gated = false) {
  a.take(enc_blk(i, "ln1_g"), D * 4); a.take(enc_blk(i, "ln1_b"), D * 4);
  a.take(enc_blk(i, "qk_w"), 2 * D * D * es); a.take(enc_blk(i, "qk_b"), 2 * D * 4);
  a.take(enc_blk(i, "v_w"), D * D * es);
  a.take(enc_blk(i, "ao_w"), D * D * es); a.take(enc_blk(i, "ao_b"), D * 4);
  a.take(enc_blk(i, "ln2_g"), D * 4); a.take(enc_blk(i, "ln2_b"), D * 4);
  if (gated) a.take(enc_blk(i, "fc1_w"), 2 * F * D * es);
  else { a.take(enc_blk(i, "fc1_w"), F * D * es); a.take(enc_blk(i, "fc1_b"), F * 4); }
  a.take(enc_blk(i, "fc2_w"), D * F * es); a.take(enc_blk(i, "fc2_b"), D * 4);
}

// one block's weights as the checkpoint holds them, fp32
struct EncoderBlockWeights {
  const float *wq = nullptr, *wk = nullptr, *wv = nullptr;      // [D][D] each
  const float *bq = nullptr, *bk = nullptr, *bv = nullptr;      // [D] each; null = zeros
  const float *wo = nullptr, *bo = nullptr;                     // output projection [D][D], [D]
  const float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  const float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;      // [F][D], [F], [D][F], [D]; gated: w1 [2 F][D], no b1
  bool gated = false;
};

// fills the entries of encoder_block_take: q (scaled) | k back to back, v apart, and the value bias moved behind the soft-max —
// its rows sum to one, so  W_o (ctx + b_v) + b_o = W_o ctx + (b_o + W_o b_v).  score_scale: head_dim^-0.5 * log2(e) of the tower's heads
inline void encoder_block_fill(Arena& a, int prec, int i, int D, int F, const EncoderBlockWeights& w, float score_scale = ATTN_SCORE_SCALE) {
  const size_t es = prec == MHIP_PREC_F16 ? 2 : 4, DD = (size_t)D * D;
  const std::vector<float> zeros(D, 0.f);
  const float *bq = w.bq ? w.bq : zeros.data(), *bk = w.bk ? w.bk : zeros.data(), *bv = w.bv ? w.bv : zeros.data();
  std::vector<float> wq(DD);
  for (size_t e = 0; e < DD; ++e) wq[e] = w.wq[e] * score_scale;
  Arena::put(prec, a.h(enc_blk(i, "qk_w")), wq.data(), DD);
  Arena::put(prec, a.h(enc_blk(i, "qk_w")) + DD * es, w.wk, DD);
  float* qkb = (float*)a.h(enc_blk(i, "qk_b"));
  for (int d = 0; d < D; ++d) { qkb[d] = bq[d] * score_scale; qkb[D + d] = bk[d]; }
  Arena::put(prec, a.h(enc_blk(i, "v_w")), w.wv, DD);
  Arena::put(prec, a.h(enc_blk(i, "ao_w")), w.wo, DD);
  float* aob = (float*)a.h(enc_blk(i, "ao_b"));
  for (int o = 0; o < D; ++o) {
    double acc = w.bo[o];
    for (int k = 0; k < D; ++k) acc += (double)w.wo[(size_t)o * D + k] * bv[k];
    aob[o] = (float)acc;
  }
  memcpy(a.h(enc_blk(i, "ln1_g")), w.ln1_g, (size_t)D * 4); memcpy(a.h(enc_blk(i, "ln1_b")), w.ln1_b, (size_t)D * 4);
  memcpy(a.h(enc_blk(i, "ln2_g")), w.ln2_g, (size_t)D * 4); memcpy(a.h(enc_blk(i, "ln2_b")), w.ln2_b, (size_t)D * 4);
  Arena::put(prec, a.h(enc_blk(i, "fc1_w")), w.w1, (size_t)(w.gated ? 2 : 1) * F * D);
  if (!w.gated) memcpy(a.h(enc_blk(i, "fc1_b")), w.b1, (size_t)F * 4);
  Arena::put(prec, a.h(enc_blk(i, "fc2_w")), w.w2, (size_t)D * F);
  memcpy(a.h(enc_blk(i, "fc2_b")), w.b2, (size_t)D * 4);
}

// block i of a CLIP tower as the OpenAI checkpoints hold it, `prefix` + "N.{ln_1, attn.in_proj_*, attn.out_proj, ln_2, mlp.c_fc,
// mlp.c_proj}": in_proj holds q, k, v one after another.  false (the error is set) when a tensor is missing or misshapen
inline bool clip_resblock_weights(mhip_ctx* ctx, const TensorStore& st, const std::string& prefix, int i, int D, int F, EncoderBlockWeights* w) {
  const std::string p = prefix + std::to_string(i) + ".";
  const HostTensor* iw = st.find(ctx, p + "attn.in_proj_weight", {3 * D, D});
  const HostTensor* ib = st.find(ctx, p + "attn.in_proj_bias", {3 * D});
  const HostTensor* ow = st.find(ctx, p + "attn.out_proj.weight", {D, D});
  const HostTensor* ob = st.find(ctx, p + "attn.out_proj.bias", {D});
  const HostTensor* g1 = st.find(ctx, p + "ln_1.weight", {D});
  const HostTensor* b1 = st.find(ctx, p + "ln_1.bias", {D});
  const HostTensor* g2 = st.find(ctx, p + "ln_2.weight", {D});
  const HostTensor* b2 = st.find(ctx, p + "ln_2.bias", {D});
  const HostTensor* fw = st.find(ctx, p + "mlp.c_fc.weight", {F, D});
  const HostTensor* fb = st.find(ctx, p + "mlp.c_fc.bias", {F});
  const HostTensor* dw = st.find(ctx, p + "mlp.c_proj.weight", {D, F});
  const HostTensor* db = st.find(ctx, p + "mlp.c_proj.bias", {D});
  if (!iw || !ib || !ow || !ob || !g1 || !b1 || !g2 || !b2 || !fw || !fb || !dw || !db) return false;
  const size_t DD = (size_t)D * D;
  w->wq = iw->data.data(); w->wk = w->wq + DD; w->wv = w->wq + 2 * DD;
  w->bq = ib->data.data(); w->bk = w->bq + D; w->bv = w->bq + 2 * D;
  w->wo = ow->data.data(); w->bo = ob->data.data();
  w->ln1_g = g1->data.data(); w->ln1_b = b1->data.data(); w->ln2_g = g2->data.data(); w->ln2_b = b2->data.data();
  w->w1 = fw->data.data(); w->b1 = fb->data.data(); w->w2 = dw->data.data(); w->b2 = db->data.data();
  return true;
}

// the buffers of the layers of one call of R = images * npad token rows, element type T
struct EncoderWs {
  char* ht = nullptr;    // [R][D] the layer's input rows (a LayerNorm's output)
  char* qk = nullptr;    // [R + ATTN_SLACK_ROWS][2 D] q | k rows
  char* vt = nullptr;    // [D][R] (+ ATTN_SLACK_ROWS elements) V^T
  char* ao = nullptr;    // [R][D] attention output
  char* hid = nullptr;   // [R][F] mlp hidden; also the patch matrix [<= R][K0]
};

inline void encoder_ws_carve(Carver& ws, size_t R, size_t D, size_t F, size_t K0, size_t es, EncoderWs* w) {
  w->ht = ws.take(R * D * es);
  w->qk = ws.take((R + ATTN_SLACK_ROWS) * 2 * D * es);
  w->vt = ws.take((D * R + ATTN_SLACK_ROWS) * es);
  w->ao = ws.take(R * D * es);
  w->hid = ws.take(R * std::max(F, K0) * es);
}

// the slack of qk and vt is read by the last image's final tiles (and masked): keep it finite
inline int encoder_ws_clear_slack(mhip_ctx* ctx, const EncoderWs& w, size_t R, size_t D, size_t es) {
  MHIP_HIP(ctx, hipMemsetAsync(w.qk + R * 2 * D * es, 0, (size_t)ATTN_SLACK_ROWS * 2 * D * es, ctx->stream));
  MHIP_HIP(ctx, hipMemsetAsync(w.vt + D * R * es, 0, ATTN_SLACK_ROWS * es, ctx->stream));
  return MHIP_OK;
}

// self-attention of `images` sequences of n_tok tokens in npad rows each over q | k rows of pitch 2 D and V^T of pitch images * npad
inline AttnDesc encoder_attn_desc(const void* qk, const void* vt, void* ao, int D, size_t es, int images, int heads, int npad, int n_tok) {
  AttnDesc ad;
  ad.q = qk; ad.k = (const char*)qk + (size_t)D * es; ad.vt = vt; ad.out = ao;
  ad.ldq = ad.ldk = 2 * D; ad.ldv = images * npad; ad.ldo = D;
  ad.images = images; ad.heads = heads; ad.npad_q = ad.npad_k = npad; ad.n_queries = ad.n_keys = n_tok;
  return ad;
}

// q|k and V^T of block i from w.ht; ad is encoder_attn_desc of w's buffers, which carries D (ldo) and R (ldv)
inline int encoder_block_qkv(mhip_ctx* ctx, int prec, const Arena& a, int i, const EncoderWs& w, const AttnDesc& ad) {
  const int D = ad.ldo, R = ad.ldv;
  int rc;
  if ((rc = mhip_gemm(ctx, prec, w.ht, a.d(enc_blk(i, "qk_w")), R, 2 * D, D, nullptr, a.d<float>(enc_blk(i, "qk_b")), w.qk, ACT_NONE, 0))) return rc;
  return mhip_gemm(ctx, prec, a.d(enc_blk(i, "v_w")), w.ht, D, R, D, nullptr, nullptr, w.vt, ACT_NONE, 0);   // V^T = W_v X^T
}

// The host entries that run one attention kernel alone (the kernel tests): q, k, v fp32 [R = B * npad][D = heads * head_dim] on the
// host -> out fp32 [R][D].  Carves an EncoderWs, the fp32 output and what `more(Carver&)` takes, writes q | k rows of pitch 2 D and
// V^T [D][R] as the tower's GEMMs write them, and runs `launch(AttnDesc)` on them
template <typename More, typename Launch>
int encoder_attention_host(mhip_ctx* ctx, int prec, const float* q, const float* k, const float* v, int B, int heads, int head_dim, int npad,
                           float* out, More&& more, Launch&& launch) {
  const size_t es = prec == MHIP_PREC_F16 ? 2 : 4, D = (size_t)heads * head_dim, R = (size_t)B * npad;
  EncoderWs w;
  float* dout = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) { encoder_ws_carve(ws, R, D, 64, 0, es, &w); dout = ws.take<float>(R * D * 4); more(ws); });
  if (rc) return rc;
  std::vector<float> qk(R * 2 * D), vt(D * R);
  for (size_t r = 0; r < R; ++r) {
    memcpy(&qk[r * 2 * D], q + r * D, D * 4);
    memcpy(&qk[r * 2 * D + D], k + r * D, D * 4);
    for (size_t d = 0; d < D; ++d) vt[d * R + r] = v[r * D + d];
  }
  std::vector<char> qkt(qk.size() * es), vtt(vt.size() * es);
  Arena::put(prec, qkt.data(), qk.data(), qk.size());
  Arena::put(prec, vtt.data(), vt.data(), vt.size());
  MHIP_HIP(ctx, hipMemcpyAsync(w.qk, qkt.data(), qkt.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(w.vt, vtt.data(), vtt.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the sources are host temporaries in pageable memory
  if ((rc = launch(encoder_attn_desc(w.qk, w.vt, w.ao, (int)D, es, B, heads, npad, npad)))) {
    (void)hipStreamSynchronize(ctx->stream);      // a refusing launch may have enqueued copies from the caller's memory: none outlives the call
    return rc;
  }
  if ((rc = mhip_launch_convert_rows(ctx, prec, w.ao, dout, (int)R, (int)D))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(out, dout, R * D * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

// the causal attention of the CLIP text tower over the same buffers (attn_seq.hip)
struct AttnCausalDesc {
  AttnDesc a;
};

// the attention half of block i, w.ht -> w.ao: plain, with LayoutLMv3's bias and key mask (bd.a the descriptor), causal, or over
// sequences of their own length (attn_seq.hip)
inline int encoder_block_attention(mhip_ctx* ctx, int prec, const Arena& a, int i, const EncoderWs& w, const AttnDesc& ad) {
  const int rc = encoder_block_qkv(ctx, prec, a, i, w, ad);
  return rc ? rc : mhip_launch_attention(ctx, prec, ad);
}
inline int encoder_block_attention(mhip_ctx* ctx, int prec, const Arena& a, int i, const EncoderWs& w, const AttnBiasDesc& bd) {
  const int rc = encoder_block_qkv(ctx, prec, a, i, w, bd.a);
  return rc ? rc : mhip_launch_attention_bias(ctx, prec, bd);
}
inline int encoder_block_attention(mhip_ctx* ctx, int prec, const Arena& a, int i, const EncoderWs& w, const AttnCausalDesc& cd) {
  const int rc = encoder_block_qkv(ctx, prec, a, i, w, cd.a);
  return rc ? rc : mhip_launch_attention_causal(ctx, prec, cd.a);
}
inline int encoder_block_attention(mhip_ctx* ctx, int prec, const Arena& a, int i, const EncoderWs& w, const AttnShortDesc& sd) {
  const int rc = encoder_block_qkv(ctx, prec, a, i, w, sd.a);
  if (rc) return rc;
  // up to 128 rows a sequence the keys stay in LDS; past that they are streamed
  return sd.a.npad_k <= 128 ? mhip_launch_attention_short(ctx, prec, sd) : mhip_launch_attention_long(ctx, prec, sd);
}

// The layers of a CLIP tower (vision: AttnDesc, text: AttnCausalDesc) on the fp32 stream h [R][D]:
//   ht = LN1(h)   ao = attention(ht)          h += ao Wo^T + (bo + Wo bv)
//   ht = LN2(h)   hid = quick_gelu(ht W1^T + b1)              h += hid W2^T + b2
// tap(i + 1) runs after layer i
template <typename AD, typename Tap>
int clip_encoder_layers(mhip_ctx* ctx, int prec, const Arena& a, int depth, int D, int F, float ln_eps, size_t R, float* h,
                        const EncoderWs& w, const AD& ad, Tap&& tap) {
  int rc;
  for (int i = 0; i < depth; ++i) {
    if ((rc = mhip_launch_row_layernorm(ctx, MHIP_K_CLIPVIS_EMBED, prec, h, 0, nullptr, a.d<float>(enc_blk(i, "ln1_g")), a.d<float>(enc_blk(i, "ln1_b")), nullptr, w.ht, (int)R, D, ln_eps))) return rc;
    if ((rc = encoder_block_attention(ctx, prec, a, i, w, ad))) return rc;
    if ((rc = mhip_gemm(ctx, prec, w.ao, a.d(enc_blk(i, "ao_w")), (long long)R, D, D, nullptr, a.d<float>(enc_blk(i, "ao_b")), h, ACT_NONE, 1, h))) return rc;
    if ((rc = mhip_launch_row_layernorm(ctx, MHIP_K_CLIPVIS_EMBED, prec, h, 0, nullptr, a.d<float>(enc_blk(i, "ln2_g")), a.d<float>(enc_blk(i, "ln2_b")), nullptr, w.ht, (int)R, D, ln_eps))) return rc;
    if ((rc = mhip_gemm(ctx, prec, w.ht, a.d(enc_blk(i, "fc1_w")), (long long)R, F, D, nullptr, a.d<float>(enc_blk(i, "fc1_b")), w.hid, ACT_NONE, 0))) return rc;
    if ((rc = mhip_launch_quick_gelu(ctx, prec, w.hid, (long long)R * F))) return rc;
    if ((rc = mhip_gemm(ctx, prec, w.hid, a.d(enc_blk(i, "fc2_w")), (long long)R, D, F, nullptr, a.d<float>(enc_blk(i, "fc2_b")), h, ACT_NONE, 1, h))) return rc;
    if ((rc = tap(i + 1))) return rc;
  }
  return MHIP_OK;
}
