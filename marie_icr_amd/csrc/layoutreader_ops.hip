// layoutreader_ops.hip — the kernels of the LayoutReader reading-order model (layoutreader_api.hip): the layout-only embedding
// front, the decode attention of the pointer decoder over its key / value caches, and the pointer head's scores and decision.
//
// Replaces, in marie/models/unilm/layoutreader/s2s_ft/modeling_decoding.py: LayoutlmEmbeddings.forward with
// layoutlm_only_layout_flag (no word table), the attention of BertSelfAttention.forward for the one or two rows a greedy step of
// LayoutlmForSeq2SeqDecoder.forward feeds (there K and V of the whole history are projected again at every step; here they are
// cached), BertPredictionHeadTransform's LayerNorm with the einsum against the source embedding of LayoutlmSPLMPredictionHead,
// and the torch.max / torch.gather that turn the scores into the next step's token.
//
// lr_embed: one wave per row, 16 bytes a lane (the row's load, LayerNorm and store, here and in lr_pointer_scores: row_ops.h; the
//   row LayerNorms of the layers: row_ops.hip's kernel, counted in berttext_embed).  A row is described by 8 ints in HBM (x0, y0, x1, y1, position id, type id, two
//   spare): the source rows' come from the host, a step's rows are written by lr_pointer_select of the step before, so the 511
//   steps are enqueued back to back and no decision travels to the host in between.
// lr_decode_attn: one workgroup per (page, head), NQ = 1 or 2 query rows, head dim 64.  The keys of query row i are
//   [cache rows < src_len[page]] [cache rows tgt_base .. tgt_base + tgt_len[row]) [fresh rows 0 .. i of the page] — the fresh
//   rows are the step's own k / v, read from the q|k|v product.  With `keep`, fresh rows 0 .. NQ - 2 (the pointed token; never the
//   mask row) are copied into the cache slot behind the page's targets by the same workgroup, which no workgroup of the launch
//   reads.  Scores: one key per thread, its 64 elements read straight to registers in 16-byte loads; fp32 soft-max over the
//   score row held in LDS; output: a thread owns a 16-byte column chunk of every 32nd (f16) / 16th (fp32) key, partial sums
//   joined in LDS in a fixed order.  Nothing depends on the other pages of a launch: a page's rows are the same bits alone or
//   batched.  q arrives scaled by head_dim^-0.5 * log2(e).
// lr_pointer_scores: score[j] = LN(x) . E[page][j] + bias[j]; a wave normalises x in registers and keeps it there for its rows.
// lr_pointer_select: arg-max with the lowest index on ties, the decision, and the next step's two rows.
#include <algorithm>

#include "igemm_common.h"
#include "row_ops.h"

using namespace igemm;

namespace {

constexpr int LR_THREADS = 256;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct EmbedArgs {
  const int* tok;
  const float *pos, *xe, *ye, *he, *we, *type, *g, *b;
  float* h;
  int rows, D, max_position, max_2d, type_vocab;
  float eps;
};

// h[row] = LN(pos[p] + x[x0] + y[y0] + x[x1] + y[y1] + h[y1 - y0] + w[x1 - x0] + type[t]); the indices are clamped into their
// tables (the host entries have checked the source boxes; a step's rows repeat them)
template <typename T>
__global__ __launch_bounds__(LR_THREADS) void lr_embed_kernel(EmbedArgs a, T* __restrict__ ht) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  const int* t = a.tok + (size_t)row * LR_TOK_INTS;
  const int m2 = a.max_2d - 1, D = a.D;
  const int x0 = clampi(t[0], 0, m2), y0 = clampi(t[1], 0, m2), x1 = clampi(t[2], 0, m2), y1 = clampi(t[3], 0, m2);
  const float* src[8] = {a.pos + (size_t)clampi(t[4], 0, a.max_position - 1) * D,
                         a.xe + (size_t)x0 * D,
                         a.ye + (size_t)y0 * D,
                         a.xe + (size_t)x1 * D,
                         a.ye + (size_t)y1 * D,
                         a.he + (size_t)clampi(y1 - y0, 0, m2) * D,
                         a.we + (size_t)clampi(x1 - x0, 0, m2) * D,
                         a.type + (size_t)clampi(t[5], 0, a.type_vocab - 1) * D};
  float4v v[ROW_GROUPS];
  row_load(v, src[0], D, lane);
#pragma unroll
  for (int s = 1; s < 8; ++s) row_add(v, src[s], D, lane);
  row_layernorm(v, D, lane, a.g, a.b, a.eps);
  row_store<T>(v, a.h + (size_t)row * D, ht ? ht + (size_t)row * D : nullptr, D, lane);
}

// ------------------------------------------------------------------------------------------------------- decode attention
template <typename T>
struct DecArgs {
  const T *q, *k, *v;      // the step's rows [pages * NQ][ld], head h at column h * 64
  T *kc, *vc;              // [pages][cache_rows][D]
  T* out;                  // [pages * NQ][ldo]
  const int* src_len;      // [pages]
  const int* tgt_len;      // [pages * NQ]
  int ld, ldo, D, cache_rows, tgt_base, keep;
};

template <typename T, int NQ>
__global__ __launch_bounds__(LR_THREADS) void lr_decode_attn_kernel(DecArgs<T> p, int heads) {
  typedef Tr<T> X;
  typedef typename X::chunk_t chunk_t;
  constexpr int E = X::E;            // elements of a 16-byte chunk
  constexpr int NC = 64 / E;         // chunks of a head's row
  constexpr int KG = LR_THREADS / NC;
  __shared__ float qs[NQ][64];
  __shared__ float sc[NQ][LR_ATTN_MAX_KEYS];
  __shared__ float red[KG][NQ][64];
  __shared__ float part[4][NQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int head = blockIdx.x % heads, page = blockIdx.x / heads;
  const size_t frow = (size_t)page * NQ, crow = (size_t)page * p.cache_rows;
  const int hc = head * 64;
  // the host entries have checked the lengths; the clamps keep a stray value inside the caches and the score rows
  const int ns = clampi(p.src_len[page], 0, p.tgt_base);
  int tl[NQ], tmax = 0;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    tl[i] = clampi(p.tgt_len[frow + i], 0, p.cache_rows - p.tgt_base);
    tmax = max(tmax, tl[i]);
  }
  tmax = min(tmax, LR_ATTN_MAX_KEYS - NQ - ns);
  const int nk = ns + tmax + NQ;

  if (tid < NQ * 64) qs[tid >> 6][lane] = (float)p.q[(frow + (tid >> 6)) * p.ld + hc + lane];
  if (p.keep) {
    // fresh rows 0 .. NQ - 2 -> the cache slot behind the page's targets
    for (int e = tid; e < (NQ - 1) * 2 * NC; e += LR_THREADS) {
      const int f = e / (2 * NC), which = (e / NC) & 1, c = (e % NC) * E;
      const int slot = p.tgt_base + tmax + f;
      if (slot < p.cache_rows) {
        const T* src = (which ? p.v : p.k) + (frow + f) * p.ld + hc + c;
        T* dst = (which ? p.vc : p.kc) + (crow + slot) * p.D + hc + c;
        *(chunk_t*)dst = *(const chunk_t*)src;
      }
    }
  }
  __syncthreads();

  auto key_row = [&](const T* cache, const T* fresh, int j) -> const T* {
    if (j < ns) return cache + (crow + j) * p.D + hc;
    if (j < ns + tmax) return cache + (crow + p.tgt_base + (j - ns)) * p.D + hc;
    return fresh + (frow + (j - ns - tmax)) * p.ld + hc;
  };

  // scores: a key per thread
  for (int j = tid; j < nk; j += LR_THREADS) {
    const T* kr = key_row(p.kc, p.k, j);
    float acc[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc[i] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const chunk_t kv = *(const chunk_t*)(kr + c * E);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float kf = (float)kv[e];
#pragma unroll
        for (int i = 0; i < NQ; ++i) acc[i] = fmaf(kf, qs[i][c * E + e], acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const bool seen = j < ns || (j < ns + tmax ? j - ns < tl[i] : j - ns - tmax <= i);
      sc[i][j] = seen ? acc[i] : -INFINITY;
    }
  }
  __syncthreads();

  // fp32 soft-max of every row; its own fresh row is a key of every query, so the maximum is finite
  float inv[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    float m = -INFINITY;
    for (int j = tid; j < nk; j += LR_THREADS) m = fmaxf(m, sc[i][j]);
#pragma unroll
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) part[wave][i] = m;
    __syncthreads();
    m = fmaxf(fmaxf(part[0][i], part[1][i]), fmaxf(part[2][i], part[3][i]));
    __syncthreads();
    float l = 0.f;
    for (int j = tid; j < nk; j += LR_THREADS) {
      const float e = __builtin_amdgcn_exp2f(sc[i][j] - m);
      sc[i][j] = e;
      l += e;
    }
    l = wave_sum(l);
    if (lane == 0) part[wave][i] = l;
    __syncthreads();
    inv[i] = 1.f / ((part[0][i] + part[1][i]) + (part[2][i] + part[3][i]));
    __syncthreads();
  }

  // output: thread (kg, c) sums chunk c over the keys kg, kg + KG, ...
  {
    const int c = tid % NC, kg = tid / NC;
    float acc[NQ][E];
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
      for (int e = 0; e < E; ++e) acc[i][e] = 0.f;
    for (int j = kg; j < nk; j += KG) {
      float pr[NQ];
      bool any = false;
#pragma unroll
      for (int i = 0; i < NQ; ++i) { pr[i] = sc[i][j]; any = any || pr[i] != 0.f; }
      if (!any) continue;
      const chunk_t vv = *(const chunk_t*)(key_row(p.vc, p.v, j) + c * E);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float vf = (float)vv[e];
#pragma unroll
        for (int i = 0; i < NQ; ++i) acc[i][e] = fmaf(pr[i], vf, acc[i][e]);
      }
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
      for (int e = 0; e < E; ++e) red[kg][i][c * E + e] = acc[i][e];
  }
  __syncthreads();
  if (tid < NQ * 64) {
    const int i = tid >> 6;
    float o = 0.f;
    for (int kg = 0; kg < KG; ++kg) o += red[kg][i][lane];
    p.out[(frow + i) * p.ldo + hc + lane] = (T)(o * inv[i]);
  }
}

// ------------------------------------------------------------------------------------------------------- pointer head
constexpr int PS_ROWS = 16;      // source rows a workgroup scores: 4 per wave

// sc[page][j] = LN(x[page * nq + nq - 1]) . E[page][j] + bias[j], j < S
__global__ __launch_bounds__(LR_THREADS) void lr_pointer_scores_kernel(const float* __restrict__ x, int nq, const float* __restrict__ g,
                                                                       const float* __restrict__ b, float eps,
                                                                       const float* __restrict__ Em, int e_rows,
                                                                       const float* __restrict__ bias, int S, int D,
                                                                       float* __restrict__ sc, long long sc_stride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, page = blockIdx.y;
  float4v v[ROW_GROUPS];
  row_load(v, x + ((size_t)page * nq + nq - 1) * D, D, lane);
  row_layernorm(v, D, lane, g, b, eps);
  for (int r = 0; r < PS_ROWS / 4; ++r) {
    const int j = blockIdx.x * PS_ROWS + wave * (PS_ROWS / 4) + r;
    if (j >= S) break;
    const float* er = Em + ((size_t)page * e_rows + j) * D;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < ROW_GROUPS; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < D) {
        const float4v e = *(const float4v*)(er + c);
        s += (v[i][0] * e[0] + v[i][1] * e[1]) + (v[i][2] * e[2] + v[i][3] * e[3]);
      }
    }
    s = wave_sum(s);
    if (lane == 0) sc[(size_t)page * sc_stride + j] = s + bias[j];
  }
}

// decision[page][t] = the lowest index of the maximum of sc[page]; the rows step t + 1 feeds: the box of the pointed (or forced)
// source row at position src_len + t, and the mask row at src_len + t + 1, both of the target type
__global__ __launch_bounds__(LR_THREADS) void lr_pointer_select_kernel(const float* __restrict__ sc, long long sc_stride, int S,
                                                                       const int* __restrict__ forced, int t, int T,
                                                                       const int* __restrict__ src_tok, int e_rows,
                                                                       const int* __restrict__ src_len, int tgt_type,
                                                                       int* __restrict__ decisions, int* __restrict__ next_tok) {
  __shared__ float bv[4];
  __shared__ int bi[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, page = blockIdx.x;
  const float* s = sc + (size_t)page * sc_stride;
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int j = tid; j < S; j += LR_THREADS) {
    const float v = s[j];
    if (v > best || (v == best && j < idx)) { best = v; idx = j; }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(idx, o);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  if (lane == 0) { bv[wave] = best; bi[wave] = idx; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
    idx = clampi(idx, 0, S - 1);      // a row of NaNs decides 0
    decisions[(size_t)page * T + t] = idx;
    const int feed = forced ? clampi(forced[(size_t)page * T + t], 0, S - 1) : idx;
    const int* box = src_tok + ((size_t)page * e_rows + feed) * LR_TOK_INTS;
    int* nt = next_tok + (size_t)page * 2 * LR_TOK_INTS;
    const int pos = src_len[page] + t;
    nt[0] = box[0]; nt[1] = box[1]; nt[2] = box[2]; nt[3] = box[3]; nt[4] = pos; nt[5] = tgt_type; nt[6] = 0; nt[7] = 0;
    nt[8] = 0; nt[9] = 0; nt[10] = 0; nt[11] = 0; nt[12] = pos + 1; nt[13] = tgt_type; nt[14] = 0; nt[15] = 0;
  }
}

template <typename T>
void launch_decode(mhip_ctx* ctx, const LrDecAttnDesc& d) {
  DecArgs<T> a;
  a.q = (const T*)d.q; a.k = (const T*)d.k; a.v = (const T*)d.v; a.kc = (T*)d.kc; a.vc = (T*)d.vc; a.out = (T*)d.out;
  a.src_len = d.src_len; a.tgt_len = d.tgt_len;
  a.ld = d.ld; a.ldo = d.ldo; a.D = d.heads * 64; a.cache_rows = d.cache_rows; a.tgt_base = d.tgt_base; a.keep = d.keep;
  dim3 grid((unsigned)(d.pages * d.heads)), block(LR_THREADS);
  if (d.nq == 1) PROF_LAUNCH(ctx, MHIP_K_DEC_OPS, hipLaunchKernelGGL((lr_decode_attn_kernel<T, 1>), grid, block, 0, ctx->stream, a, d.heads));
  else PROF_LAUNCH(ctx, MHIP_K_DEC_OPS, hipLaunchKernelGGL((lr_decode_attn_kernel<T, 2>), grid, block, 0, ctx->stream, a, d.heads));
}

}  // namespace

int mhip_launch_lr_embed(mhip_ctx* ctx, int precision, const LrEmbedDesc& d) {
  if (d.rows <= 0 || !row_width_ok(d.D) || d.max_position < 1 || d.max_2d < 1 || d.type_vocab < 1 || !d.tok || !d.h)
    return mhip_fail(ctx, MHIP_EINVAL, "lr_embed: rows=%d D=%d", d.rows, d.D);
  EmbedArgs a;
  a.tok = d.tok; a.pos = d.pos; a.xe = d.xe; a.ye = d.ye; a.he = d.he; a.we = d.we; a.type = d.type; a.g = d.g; a.b = d.b;
  a.h = d.h; a.rows = d.rows; a.D = d.D; a.max_position = d.max_position; a.max_2d = d.max_2d; a.type_vocab = d.type_vocab;
  a.eps = d.eps;
  dim3 grid((d.rows + 3) / 4), block(LR_THREADS);
  if (precision == MHIP_PREC_F16) PROF_LAUNCH(ctx, MHIP_K_DEC_OPS, hipLaunchKernelGGL(lr_embed_kernel<_Float16>, grid, block, 0, ctx->stream, a, (_Float16*)d.ht));
  else PROF_LAUNCH(ctx, MHIP_K_DEC_OPS, hipLaunchKernelGGL(lr_embed_kernel<float>, grid, block, 0, ctx->stream, a, (float*)d.ht));
  CHECK_LAUNCH(ctx, "lr_embed");
  return 0;
}

int mhip_launch_lr_decode_attention(mhip_ctx* ctx, int precision, const LrDecAttnDesc& d) {
  if (d.pages <= 0 || d.heads <= 0 || (long long)d.pages * d.heads > 0x7fffffffLL || (d.nq != 1 && d.nq != 2) || d.tgt_base < 1 ||
      d.tgt_base > LR_ATTN_MAX_KEYS - 2 || d.cache_rows < d.tgt_base || !d.src_len || !d.tgt_len)
    return mhip_fail(ctx, MHIP_EINVAL, "lr_decode_attention: bad shape (%d pages, %d heads, %d query rows, caches of %d rows, targets from %d)",
                     d.pages, d.heads, d.nq, d.cache_rows, d.tgt_base);
  const int esz = precision == MHIP_PREC_F16 ? 2 : 4;
  if ((d.ld * esz) % 16 || (d.heads * 64 * esz) % 16 || ((uintptr_t)d.q & 15) || ((uintptr_t)d.k & 15) || ((uintptr_t)d.v & 15) ||
      ((uintptr_t)d.kc & 15) || ((uintptr_t)d.vc & 15))
    return mhip_fail(ctx, MHIP_EINVAL, "lr_decode_attention: rows must keep 16-byte alignment");
  if (precision == MHIP_PREC_F16) launch_decode<_Float16>(ctx, d);
  else launch_decode<float>(ctx, d);
  CHECK_LAUNCH(ctx, "lr_decode_attention");
  return 0;
}

int mhip_launch_lr_pointer_scores(mhip_ctx* ctx, const float* x, int nq, const float* g, const float* b, float eps, const float* E,
                                  int e_rows, const float* bias, int S, int D, int pages, float* sc, long long sc_stride) {
  if (pages <= 0 || pages > 65535 || S < 1 || e_rows < S || nq < 1 || !row_width_ok(D) || sc_stride < S)
    return mhip_fail(ctx, MHIP_EINVAL, "lr_pointer_scores: pages=%d S=%d D=%d", pages, S, D);
  dim3 grid((S + PS_ROWS - 1) / PS_ROWS, pages), block(LR_THREADS);
  PROF_LAUNCH(ctx, MHIP_K_DEC_OPS, hipLaunchKernelGGL(lr_pointer_scores_kernel, grid, block, 0, ctx->stream, x, nq, g, b, eps, E, e_rows, bias, S, D, sc, sc_stride));
  CHECK_LAUNCH(ctx, "lr_pointer_scores");
  return 0;
}

int mhip_launch_lr_pointer_select(mhip_ctx* ctx, const float* sc, long long sc_stride, int S, const int* forced, int t, int T,
                                  const int* src_tok, int e_rows, const int* src_len, int tgt_type, int pages, int* decisions,
                                  int* next_tok) {
  if (pages <= 0 || S < 1 || e_rows < S || t < 0 || t >= T || !decisions || !next_tok)
    return mhip_fail(ctx, MHIP_EINVAL, "lr_pointer_select: pages=%d S=%d step %d of %d", pages, S, t, T);
  PROF_LAUNCH(ctx, MHIP_K_DEC_OPS, hipLaunchKernelGGL(lr_pointer_select_kernel, dim3(pages), dim3(LR_THREADS), 0, ctx->stream, sc, sc_stride, S, forced, t, T, src_tok, e_rows, src_len, tgt_type, decisions, next_tok));
  CHECK_LAUNCH(ctx, "lr_pointer_select");
  return 0;
}
