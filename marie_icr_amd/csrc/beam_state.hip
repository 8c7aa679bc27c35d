// beam_state.hip — the generator's per-step bookkeeping on the device.
//
// TextRecognitionGenerator._generate (marie/models/unilm/trocr/generator.py:127-362) interleaves the decoder forward with
// small, branchy list work per sentence: finalize_hypos over the eos candidates among the first `beam` (:225-248), the `beam`
// best live candidates become the next step's rows (:297-343), the finished hypotheses are sorted by score at the end (:362-372).
// Done on the host that work costs a stream drain per step (candidates down, tokens / parents up).  Here one thread per crop
// does it where the candidates already are; the host only watches a "crops remaining" counter, one step late.
// Finished crops keep their rows (no batch compaction: the reference's :256-289 shrink the batch, which changes no result).
#include <math.h>

#include "common.h"

namespace {

__global__ void beam_init_kernel(BeamState st, int* anc0, int anc_ld) {
  const int M = st.bsz * st.beam, ld = st.max_len + 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M * ld) {
    const int v = (i % ld) == 0 ? st.eos : st.pad;
    st.tokens[0][i] = v;
    st.tokens[1][i] = v;
  }
  if (i < M * anc_ld) anc0[i] = (i % anc_ld) == 0 ? i / anc_ld : 0;      // step 0: every hypothesis reads its own slot
  if (i < M) {
    st.last_tok[i] = st.eos;
    st.parent[i] = i;
    st.cum[i] = 0.f;
    st.ignore[i] = 0;
  }
  if (i < st.bsz) {
    st.finished[i] = 0;
    st.fin_count[i] = 0;
  }
  if (i == 0) *st.remaining = st.bsz;
}

__global__ void beam_select_kernel(BeamState st, int cur, int step) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= st.bsz) return;
  const int beam = st.beam, K2 = 2 * beam, ld = st.max_len + 2, ML = st.max_len;
  if (st.finished[s]) {
    for (int b = 0; b < beam; ++b) { st.parent[s * beam + b] = s * beam + b; st.last_tok[s * beam + b] = st.eos; }
    return;
  }
  const float* cs = st.cand_scores + (size_t)s * K2;
  const int* ct = st.cand_tokens + (size_t)s * K2;
  const int* cb = st.cand_beams + (size_t)s * K2;
  const int* told = st.tokens[cur];
  int* tnew = st.tokens[cur ^ 1];
  bool eos_mask[8];
  for (int j = 0; j < K2; ++j) eos_mask[j] = ct[j] == st.eos && cs[j] != -INFINITY;
  for (int j = 0; j < beam; ++j)
    if (st.ignore[s * beam + j]) eos_mask[j] = false;
  // finalize_hypos: eos candidates among the first `beam`
  int nfin = st.fin_count[s];
  for (int j = 0; j < beam; ++j) {
    if (!eos_mask[j] || nfin >= beam) continue;
    const int src = s * beam + cb[j];
    int* to = st.fin_tokens + ((size_t)s * beam + nfin) * (ML + 1);
    for (int t = 0; t < step; ++t) to[t] = told[(size_t)src * ld + 1 + t];
    to[step] = st.eos;
    st.fin_len[s * beam + nfin] = step + 1;
    st.fin_score[s * beam + nfin] = cs[j] / (float)(step + 1);          // normalize_scores, len_penalty 1
    ++nfin;
  }
  st.fin_count[s] = nfin;
  if ((nfin == beam || step == ML) && (nfin > 0 || step == ML)) {
    st.finished[s] = 1;
    atomicSub(st.remaining, 1);
    for (int b = 0; b < beam; ++b) { st.parent[s * beam + b] = s * beam + b; st.last_tok[s * beam + b] = st.eos; }
    return;
  }
  // active hypotheses: the `beam` best candidates that are not finished ones
  for (int j = 0; j < beam; ++j) eos_mask[j] = eos_mask[j] || st.ignore[s * beam + j];
  int order[8], nact = 0;
  for (int j = 0; j < K2 && nact < beam; ++j)
    if (!eos_mask[j]) order[nact++] = j;
  int nign = 0;
  for (int j = 0; j < K2 && nact + nign < beam; ++j)
    if (eos_mask[j]) order[nact + nign++] = j;      // fewer than `beam` live candidates: the rest are ignored slots
  for (int b = 0; b < beam; ++b) {
    const int j = order[b], row = s * beam + b, src = s * beam + cb[j];
    st.ignore[row] = b >= nact;
    for (int t = 0; t <= step; ++t) tnew[(size_t)row * ld + t] = told[(size_t)src * ld + t];
    tnew[(size_t)row * ld + step + 1] = ct[j];
    st.parent[row] = src;
    st.last_tok[row] = ct[j];
    st.cum[row] = cs[j];
  }
}

__global__ void beam_best_kernel(BeamState st, int* tokens_out, int* lengths_out, float* scores_out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= st.bsz) return;
  const int ML = st.max_len, beam = st.beam;
  // highest score, the first finalized wins ties (torch.sort(descending) over the score list, generator.py:364-368)
  int best = -1;
  for (int j = 0; j < st.fin_count[s]; ++j)
    if (best < 0 || st.fin_score[s * beam + j] > st.fin_score[s * beam + best]) best = j;
  int* to = tokens_out + (size_t)s * (ML + 1);
  for (int t = 0; t <= ML; ++t) to[t] = st.pad;
  if (best < 0) { lengths_out[s] = 0; scores_out[s] = -INFINITY; return; }
  const int len = st.fin_len[s * beam + best];
  const int* from = st.fin_tokens + ((size_t)s * beam + best) * (ML + 1);
  for (int t = 0; t < len && t <= ML; ++t) to[t] = from[t];
  lengths_out[s] = len;
  scores_out[s] = st.fin_score[s * beam + best];
}

}  // namespace

void mhip_beam_state_carve(Carver& ws, int bsz, int beam, int max_len, int pad, int eos, BeamState* st) {
  const size_t M = (size_t)bsz * beam;
  st->bsz = bsz; st->beam = beam; st->max_len = max_len; st->pad = pad; st->eos = eos;
  st->tokens[0] = ws.take<int>(M * (max_len + 2) * 4);
  st->tokens[1] = ws.take<int>(M * (max_len + 2) * 4);
  st->last_tok = ws.take<int>(M * 4);
  st->parent = ws.take<int>(M * 4);
  st->cum = ws.take<float>(M * 4);
  st->ignore = ws.take<unsigned char>(M);
  st->finished = ws.take<unsigned char>(bsz);
  st->fin_count = ws.take<int>((size_t)bsz * 4);
  st->fin_tokens = ws.take<int>(M * (max_len + 1) * 4);
  st->fin_len = ws.take<int>(M * 4);
  st->fin_score = ws.take<float>(M * 4);
  st->remaining = ws.take<int>(4);
}

int mhip_launch_beam_init(mhip_ctx* ctx, const BeamState& st, int* anc0, int anc_ld) {
  const long long M = (long long)st.bsz * st.beam;
  const long long total = std::max(M * (st.max_len + 2), M * anc_ld);
  PROF_LAUNCH(ctx, MHIP_K_DEC_OPS, hipLaunchKernelGGL(beam_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, st, anc0, anc_ld));
  CHECK_LAUNCH(ctx, "beam_init");
  return 0;
}

int mhip_launch_beam_select(mhip_ctx* ctx, const BeamState& st, int cur, int step) {
  PROF_LAUNCH(ctx, MHIP_K_DEC_OPS, hipLaunchKernelGGL(beam_select_kernel, dim3((st.bsz + 63) / 64), dim3(64), 0, ctx->stream, st, cur, step));
  CHECK_LAUNCH(ctx, "beam_select");
  return 0;
}

int mhip_launch_beam_best(mhip_ctx* ctx, const BeamState& st, int* tokens_out, int* lengths_out, float* scores_out) {
  PROF_LAUNCH(ctx, MHIP_K_DEC_OPS, hipLaunchKernelGGL(beam_best_kernel, dim3((st.bsz + 63) / 64), dim3(64), 0, ctx->stream, st, tokens_out, lengths_out, scores_out));
  CHECK_LAUNCH(ctx, "beam_best");
  return 0;
}

// ---- the search alone, on host inputs (kernel-level tests) -------------------------------------------------------------------
namespace {

constexpr int BEAM_GUARD = 16;       // elements behind each candidate list of mhip_beam_candidates_host

// what neither launcher judges but a search needs to stay inside its buffers, and the generator's own assertion (generator.py:63)
int beam_host_args(mhip_ctx* ctx, const char* who, int max_len, int min_len, int vocab, int ld, int beam, int bsz) {
  if (beam < 1 || beam > 4 || vocab < 2 * beam) return mhip_fail(ctx, MHIP_EINVAL, "%s: beam %d vocab %d", who, beam, vocab);
  if (ld % 8 || ld < (vocab + 7) / 8 * 8) return mhip_fail(ctx, MHIP_EINVAL, "%s: the pitch %d is not the vocabulary %d rounded up to 8 columns or more", who, ld, vocab);
  if (bsz < 1 || max_len < 0) return mhip_fail(ctx, MHIP_EINVAL, "%s: bsz %d max_len %d", who, bsz, max_len);
  if (min_len > max_len) return mhip_fail(ctx, MHIP_EINVAL, "%s: min_len %d > max_len %d", who, min_len, max_len);
  return MHIP_OK;
}

}  // namespace

extern "C" int mhip_beam_candidates_host(mhip_ctx* ctx, int logits_f16, const void* logits, const float* cum, int step, int max_len,
                                         int min_len, int pad, int eos, int vocab, int ld, int beam, int bsz, float* cand_scores,
                                         int32_t* cand_tokens, int32_t* cand_beams) {
  if (!ctx || !logits || !cum || !cand_scores || !cand_tokens || !cand_beams) return MHIP_EINVAL;
  int rc = beam_host_args(ctx, "beam_candidates_host", max_len, min_len, vocab, ld, beam, bsz);
  if (rc) return rc;
  if (step < 0) return mhip_fail(ctx, MHIP_EINVAL, "beam_candidates_host: step %d", step);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t M = (size_t)bsz * beam, lbytes = M * ld * (logits_f16 ? 2 : 4), obytes = (M * 2 + BEAM_GUARD) * 4;
  char* dl = nullptr;
  float *dcum = nullptr, *ds = nullptr;
  int *dt = nullptr, *db = nullptr;
  rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dl = ws.take(lbytes); dcum = ws.take<float>(M * 4);
    ds = ws.take<float>(obytes); dt = ws.take<int>(obytes); db = ws.take<int>(obytes);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dl, logits, lbytes, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(dcum, cum, M * 4, hipMemcpyHostToDevice, ctx->stream));
  for (void* p : {(void*)ds, (void*)dt, (void*)db}) MHIP_HIP(ctx, hipMemsetAsync(p, 0xff, obytes, ctx->stream));
  BeamCandDesc bc;
  bc.logits = dl; bc.logits_f16 = logits_f16 != 0; bc.ld = ld; bc.vocab = vocab; bc.beam = beam; bc.bsz = bsz; bc.cum = dcum;
  bc.step = step; bc.max_len = max_len; bc.min_len = min_len; bc.pad = pad; bc.eos = eos;
  bc.cand_scores = ds; bc.cand_tokens = dt; bc.cand_beams = db;
  if ((rc = mhip_launch_beam_candidates(ctx, bc))) return rc;
  std::vector<char> hs(obytes), ht(obytes), hb(obytes);      // staged: a failing copy leaves the caller's arrays untouched
  MHIP_HIP(ctx, hipMemcpyAsync(hs.data(), ds, obytes, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(ht.data(), dt, obytes, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(hb.data(), db, obytes, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(cand_scores, hs.data(), obytes); memcpy(cand_tokens, ht.data(), obytes); memcpy(cand_beams, hb.data(), obytes);
  return MHIP_OK;
}

extern "C" int mhip_beam_search_host(mhip_ctx* ctx, int logits_f16, const void* logits, const float* in_scores, const int32_t* in_tokens,
                                     const int32_t* in_beams, int max_len, int min_len, int pad, int eos, int vocab, int ld, int beam,
                                     int bsz, int extra_steps, mhip_beam_trace* out) {
  if (!ctx || !out) return MHIP_EINVAL;
  const mhip_beam_trace& o = *out;
  if (!o.cand_scores || !o.cand_tokens || !o.cand_beams || !o.parent || !o.last_tok || !o.cum || !o.ignore || !o.finished ||
      !o.fin_count || !o.tokens || !o.anc || !o.remaining || !o.fin_tokens || !o.fin_len || !o.fin_score || !o.out_tokens ||
      !o.out_len || !o.out_score)
    return MHIP_EINVAL;
  if (!logits && (!in_scores || !in_tokens || !in_beams)) return MHIP_EINVAL;
  int rc = beam_host_args(ctx, "beam_search_host", max_len, min_len, vocab, ld, beam, bsz);
  if (rc) return rc;
  if (extra_steps < 0 || extra_steps > 2) return mhip_fail(ctx, MHIP_EINVAL, "beam_search_host: extra_steps %d", extra_steps);
  const int ML = max_len, K2 = 2 * beam, anc_ld = ML + 2;
  if (!logits)      // beam_select addresses token rows by a candidate's beam
    for (size_t i = 0; i < (size_t)(ML + 1) * bsz * K2; ++i)
      if (in_beams[i] < 0 || in_beams[i] >= beam) return mhip_fail(ctx, MHIP_EINVAL, "beam_search_host: candidate %zu names beam %d", i, in_beams[i]);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t M = (size_t)bsz * beam, es = logits_f16 ? 2 : 4, lbytes = logits ? M * ld * es : 0;
  const size_t cbytes = (size_t)bsz * K2 * 4, tbytes = M * (ML + 2) * 4, fbytes = M * (ML + 1) * 4;
  char* dl = nullptr;
  int* anc[2] = {nullptr, nullptr};
  float *cs = nullptr, *out_score = nullptr;
  int *ct = nullptr, *cb = nullptr, *out_tok = nullptr, *out_len = nullptr;
  BeamState st;
  // the decode buffers the search touches, in trocr_decode_carve's order
  rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    dl = ws.take(lbytes);
    for (int i = 0; i < 2; ++i) anc[i] = ws.take<int>(tbytes);
    cs = ws.take<float>(cbytes); ct = ws.take<int>(cbytes); cb = ws.take<int>(cbytes);
    mhip_beam_state_carve(ws, bsz, beam, ML, pad, eos, &st);
    out_tok = ws.take<int>((size_t)bsz * (ML + 1) * 4);
    out_len = ws.take<int>((size_t)bsz * 4);
    out_score = ws.take<float>((size_t)bsz * 4);
  });
  if (rc) return rc;
  st.cand_scores = cs; st.cand_tokens = ct; st.cand_beams = cb;
  // never-written cells show as 0xff: anc[1] has no initial state, fin_* are written as hypotheses finalise
  MHIP_HIP(ctx, hipMemsetAsync(anc[1], 0xff, tbytes, ctx->stream));
  MHIP_HIP(ctx, hipMemsetAsync(st.fin_tokens, 0xff, fbytes, ctx->stream));
  MHIP_HIP(ctx, hipMemsetAsync(st.fin_len, 0xff, M * 4, ctx->stream));
  MHIP_HIP(ctx, hipMemsetAsync(st.fin_score, 0xff, M * 4, ctx->stream));
  if ((rc = mhip_launch_beam_init(ctx, st, anc[0], anc_ld))) return rc;
  int cur = 0, tcur = 0, remaining = bsz, extra = extra_steps, steps = 0;
  for (int step = 0; step <= ML; ++step) {
    if (remaining == 0 && extra-- <= 0) break;
    if (step > 0) {
      if ((rc = mhip_launch_ancestry(ctx, anc[cur], anc[cur ^ 1], st.parent, (int)M, anc_ld, step - 1))) return rc;
      cur ^= 1;
    }
    const size_t coff = (size_t)step * bsz * K2;
    if (logits) {
      MHIP_HIP(ctx, hipMemcpyAsync(dl, (const char*)logits + (size_t)step * lbytes, lbytes, hipMemcpyHostToDevice, ctx->stream));
      BeamCandDesc bc;
      bc.logits = dl; bc.logits_f16 = logits_f16 != 0; bc.ld = ld; bc.vocab = vocab; bc.beam = beam; bc.bsz = bsz; bc.cum = st.cum;
      bc.step = step; bc.max_len = ML; bc.min_len = min_len; bc.pad = pad; bc.eos = eos;
      bc.cand_scores = cs; bc.cand_tokens = ct; bc.cand_beams = cb;
      if ((rc = mhip_launch_beam_candidates(ctx, bc))) return rc;
    } else {
      MHIP_HIP(ctx, hipMemcpyAsync(cs, in_scores + coff, cbytes, hipMemcpyHostToDevice, ctx->stream));
      MHIP_HIP(ctx, hipMemcpyAsync(ct, in_tokens + coff, cbytes, hipMemcpyHostToDevice, ctx->stream));
      MHIP_HIP(ctx, hipMemcpyAsync(cb, in_beams + coff, cbytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = mhip_launch_beam_select(ctx, st, tcur, step))) return rc;
    tcur ^= 1;
    auto down = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream); };
    MHIP_HIP(ctx, down(o.cand_scores + coff, cs, cbytes));
    MHIP_HIP(ctx, down(o.cand_tokens + coff, ct, cbytes));
    MHIP_HIP(ctx, down(o.cand_beams + coff, cb, cbytes));
    MHIP_HIP(ctx, down(o.parent + step * M, st.parent, M * 4));
    MHIP_HIP(ctx, down(o.last_tok + step * M, st.last_tok, M * 4));
    MHIP_HIP(ctx, down(o.cum + step * M, st.cum, M * 4));
    MHIP_HIP(ctx, down(o.ignore + step * M, st.ignore, M));
    MHIP_HIP(ctx, down(o.finished + (size_t)step * bsz, st.finished, bsz));
    MHIP_HIP(ctx, down(o.fin_count + (size_t)step * bsz, st.fin_count, (size_t)bsz * 4));
    MHIP_HIP(ctx, down(o.tokens + step * M * (ML + 2), st.tokens[tcur], tbytes));
    MHIP_HIP(ctx, down(o.anc + step * M * (ML + 2), anc[cur], tbytes));
    MHIP_HIP(ctx, down(o.remaining + step, st.remaining, 4));
    MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    remaining = o.remaining[step];
    steps = step + 1;
  }
  if ((rc = mhip_launch_beam_best(ctx, st, out_tok, out_len, out_score))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(o.fin_tokens, st.fin_tokens, fbytes, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(o.fin_len, st.fin_len, M * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(o.fin_score, st.fin_score, M * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(o.out_tokens, out_tok, (size_t)bsz * (ML + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(o.out_len, out_len, (size_t)bsz * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(o.out_score, out_score, (size_t)bsz * 4, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out->steps = steps;
  return MHIP_OK;
}
