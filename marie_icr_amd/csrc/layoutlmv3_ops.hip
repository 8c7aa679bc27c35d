// layoutlmv3_ops.hip — the pieces of LayoutLMv3 the ViT / TrOCR paths do not have: the tables of its learned relative-position
// attention bias, the text + layout embedding gather, the classification head and the token-classification head.
//
// Replaces, in transformers/models/layoutlmv3/modeling_layoutlmv3.py: LayoutLMv3Encoder._cal_1d_pos_emb / _cal_2d_pos_emb
// (never materialised: see below), LayoutLMv3TextEmbeddings.forward, the LayerNorms of LayoutLMv3Model.forward /
// forward_image, LayoutLMv3ClassificationHead.forward, and the head of LayoutLMv3ForTokenClassification.forward together with
// the arg-max / soft-max the document indexer takes of its logits (marie/components/document_indexer/transformers.py:556-568).
//
// The bias of a score depends on (i, j) only through three integer differences, p_j - p_i, x0_j - x0_i, y1_j - y1_i, so
// per head three difference-indexed tables replace the [heads][n][n] tensors the library builds (3 x 24 MB a page): they are
// folded with the head weights and the score scale once (mhip_attn_bias_fold).  The attention that reads them
// (mhip_launch_attention_bias) is the biased instance of the one attention kernel, in attn_flash.hip.
#include "igemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------- embeddings
// LayerNorm of the row a wave holds (nv float4 groups per lane), two-pass in registers
__device__ __forceinline__ void wave_layernorm(float4v v[4], int nv, int D, int lane, const float* __restrict__ g,
                                               const float* __restrict__ b, float eps) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
#pragma unroll
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv)
#pragma unroll
      for (int k = 0; k < 4; ++k) { const float d = v[i][k] - mean; q += d * d; }
#pragma unroll
  for (int o = 32; o; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = 1.f / sqrtf(q / (float)D + eps);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv) {
      const int c = (i * 64 + lane) * 4;
      const float4v gg = *(const float4v*)(g + c), bb = *(const float4v*)(b + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[i][k] = (v[i][k] - mean) * rstd * gg[k] + bb[k];
    }
}

struct EmbedArgs {
  const int* tok;
  const int* win_page;
  const void* word;
  const float *type0, *pos, *xe, *ye, *he, *we, *g_text, *b_text, *patches, *cls, *g_vis, *b_vis, *g_all, *b_all;
  float* h;
  void* ht;
  int rows, max_text, n_vis, npad, D, coord, shape;
  float eps, eps_vis;
};

// one wave per row of the sequence: text rows gather word + token type + position + the six layout embeddings and take the
// embeddings' LayerNorm, visual rows take the patch projection (or the cls row) and `norm`; both then take the model's
// LayerNorm over the concatenated sequence.  Rows past the sequence (npad) are zeros.  A "page" of rows is one window of text;
// its patch rows are those of the page image win_page names (windows of one page share them).
template <typename T>
__global__ __launch_bounds__(256) void lmv3_embed_kernel(EmbedArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  const int page = row / a.npad, t = row % a.npad;
  const int D = a.D, nv = D >> 8;
  float4v v[4];
  if (t < a.max_text) {
    const int* tk = a.tok + ((size_t)page * a.max_text + t) * 8;
    const int id = tk[0], pid = tk[1];
    const int c4 = 4 * a.coord;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nv) {
        const int c = (i * 64 + lane) * 4;
        float4v w;
        if (sizeof(T) == 2) {
          typedef _Float16 half4 __attribute__((ext_vector_type(4)));
          const half4 hw = *(const half4*)((const _Float16*)a.word + (size_t)id * D + c);
          w = (float4v){(float)hw[0], (float)hw[1], (float)hw[2], (float)hw[3]};
        } else {
          w = *(const float4v*)((const float*)a.word + (size_t)id * D + c);
        }
        // segment of the concatenated layout embedding this group of four columns lies in
        const float* sp;
        if (c < c4) {
          const int seg = c / a.coord, cc = c - seg * a.coord;
          sp = ((seg & 1) ? a.ye : a.xe) + (size_t)tk[2 + seg] * a.coord + cc;
        } else {
          const int seg = (c - c4) / a.shape, cc = c - c4 - seg * a.shape;
          sp = (seg ? a.we : a.he) + (size_t)tk[6 + seg] * a.shape + cc;
        }
        v[i] = ((w + *(const float4v*)(a.type0 + c)) + *(const float4v*)(a.pos + (size_t)pid * D + c)) + *(const float4v*)sp;
      }
    wave_layernorm(v, nv, D, lane, a.g_text, a.b_text, a.eps);
  } else if (t < a.max_text + a.n_vis) {
    const int vi = t - a.max_text;
    const float* src = vi == 0 ? a.cls : a.patches + ((size_t)a.win_page[page] * (a.n_vis - 1) + vi - 1) * D;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nv) v[i] = *(const float4v*)(src + (i * 64 + lane) * 4);
    wave_layernorm(v, nv, D, lane, a.g_vis, a.b_vis, a.eps_vis);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float4v){0.f, 0.f, 0.f, 0.f};
  }
  if (t < a.max_text + a.n_vis) wave_layernorm(v, nv, D, lane, a.g_all, a.b_all, a.eps);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv) {
      const size_t o = (size_t)row * D + (i * 64 + lane) * 4;
      *(float4v*)(a.h + o) = v[i];
      T o4[4] = {(T)v[i][0], (T)v[i][1], (T)v[i][2], (T)v[i][3]};
      if (sizeof(T) == 2) *(uint64_t*)((T*)a.ht + o) = *(uint64_t*)o4;
      else *(float4v*)((T*)a.ht + o) = *(float4v*)o4;
    }
}

// ------------------------------------------------------------------------------------------------------- head
// one workgroup per page: y = tanh(W_d x + b_d) (x = row 0 of the page), logits = W_o y + b_o.  A wave per output, lanes along k.
__global__ __launch_bounds__(256) void lmv3_head_kernel(const float* __restrict__ h, int npad, int D, const float* __restrict__ dw,
                                                        const float* __restrict__ db, const float* __restrict__ ow,
                                                        const float* __restrict__ ob, int labels, float* __restrict__ logits) {
  __shared__ float xs[1024], ys[1024];
  const int page = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = h + (size_t)page * npad * D;
  for (int d = threadIdx.x; d < D; d += 256) xs[d] = x[d];
  __syncthreads();
  for (int j = wave; j < D; j += 4) {
    float acc = 0.f;
    for (int k = lane; k < D; k += 64) acc += dw[(size_t)j * D + k] * xs[k];
#pragma unroll
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) ys[j] = tanhf(acc + db[j]);
  }
  __syncthreads();
  for (int j = wave; j < labels; j += 4) {
    float acc = 0.f;
    for (int k = lane; k < D; k += 64) acc += ow[(size_t)j * D + k] * ys[k];
#pragma unroll
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) logits[(size_t)page * labels + j] = acc + ob[j];
  }
}

// ------------------------------------------------------------------------------------------------------- token head
// logits = W_o f(x) + b_o for every text row (f = tanh for the dense head, whose D x D product has run as a GEMM; identity for the
// linear head), then the decision the indexer takes of them: label = lowest index of the maximum, score = 1 / sum exp(z - z_max).
// fp32 throughout.  W_o is staged in LDS once per workgroup (rows of D + 8 floats: the eight labels a wave works on at a time
// fall in eight different bank groups); a workgroup then takes TH_ROWS rows, a wave one row at a time: the row is read once
// from HBM into LDS, eight lanes share a label (lane g sums k = g, g + 8, ...), eight labels a pass.
constexpr int TH_ROWS = 32;        // rows per workgroup
constexpr int TH_GROUP = 8;        // lanes per label
constexpr int TH_PASSES = 8;       // passes of 64 / TH_GROUP labels: 64 labels at the most

struct TokenHeadArgs {
  const float* x;
  const float *w, *b;
  int* label;
  float* score;
  float* logits;
  int rows, seg, seg_stride, D, L, use_tanh;
};

__global__ __launch_bounds__(256) void lmv3_token_head_kernel(TokenHeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) float th_smem[];
  const int D = a.D, L = a.L, ldw = D + 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane & (TH_GROUP - 1), jl = lane / TH_GROUP;
  float* ws = th_smem;
  float* xs = th_smem + (size_t)L * ldw + (size_t)wave * D;
  for (int e = threadIdx.x * 4; e < L * D; e += 1024) {
    const int j = e / D, k = e - j * D;
    *(float4v*)(ws + (size_t)j * ldw + k) = *(const float4v*)(a.w + e);
  }
  const int row0 = blockIdx.x * TH_ROWS;
  for (int it = 0; it < TH_ROWS / 4; ++it) {
    const int r = row0 + it * 4 + wave;
    const bool live = r < a.rows;
    __syncthreads();                      // W_o staged (first turn); the previous row of this wave consumed
    if (live) {
      const float* x = a.x + ((size_t)(r / a.seg) * a.seg_stride + r % a.seg) * D;
      for (int k = lane * 4; k < D; k += 256) {
        float4v v = *(const float4v*)(x + k);
        if (a.use_tanh) v = (float4v){tanhf(v[0]), tanhf(v[1]), tanhf(v[2]), tanhf(v[3])};
        *(float4v*)(xs + k) = v;
      }
    }
    __syncthreads();
    if (!live) continue;                  // the barriers above are reached by every wave: TH_ROWS / 4 turns each
    float z[TH_PASSES];
    float best = -INFINITY;
    int best_j = 0;
#pragma unroll
    for (int p = 0; p < TH_PASSES; ++p) {
      z[p] = -INFINITY;
      if (p * (64 / TH_GROUP) < L) {
        const int j = p * (64 / TH_GROUP) + jl;
        float acc = 0.f;
        if (j < L) {
          const float* wr = ws + (size_t)j * ldw;
          for (int k = g; k < D; k += TH_GROUP) acc += wr[k] * xs[k];
        }
#pragma unroll
        for (int o = TH_GROUP / 2; o; o >>= 1) acc += __shfl_xor(acc, o);
        if (j < L) {
          z[p] = acc + a.b[j];
          if (a.logits && g == 0) a.logits[(size_t)r * L + j] = z[p];
          if (z[p] > best) { best = z[p]; best_j = j; }
        }
      }
    }
    // the maximum over the eight label lanes, ties to the lowest index
#pragma unroll
    for (int o = TH_GROUP; o < 64; o <<= 1) {
      const float ob = __shfl_xor(best, o);
      const int oj = __shfl_xor(best_j, o);
      if (ob > best || (ob == best && oj < best_j)) { best = ob; best_j = oj; }
    }
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < TH_PASSES; ++p)
      if (p * (64 / TH_GROUP) + jl < L) s += expf(z[p] - best);
#pragma unroll
    for (int o = TH_GROUP; o < 64; o <<= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
      a.label[r] = best_j;
      a.score[r] = 1.f / s;
    }
  }
}

}  // namespace

// LayoutLMv3Encoder.relative_position_bucket(bidirectional=True) of one difference.  The logarithmic half is evaluated in
// float32, operation by operation as the library's tensor expression is: its truncation decides the bucket borders.
int mhip_relative_position_bucket(int relative_position, int num_buckets, int max_distance) {
  int ret = 0;
  num_buckets /= 2;
  if (relative_position > 0) ret += num_buckets;
  const int n = relative_position < 0 ? -relative_position : relative_position;
  const int max_exact = num_buckets / 2;
  if (n < max_exact) return ret + n;
  volatile float v = logf((float)n / (float)max_exact);
  v = v / (float)log((double)max_distance / (double)max_exact);
  v = v * (float)(num_buckets - max_exact);
  int large = max_exact + (int)v;
  if (large > num_buckets - 1) large = num_buckets - 1;
  return ret + large;
}

void mhip_attn_bias_fold(const float* w1, const float* wx, const float* wy, int heads, int bins_1d, int max_1d, int bins_2d,
                         int max_2d, int dp, int dx, float scale, float* tab) {
  const int len = mhip_attn_bias_table_len(dp, dx), off_x = 3 * dp + 2, off_y = off_x + 2 * dx + 1;
  std::vector<int> b1(2 * dp + 1), b2(2 * dx + 1);
  for (int i = 0; i <= 2 * dp; ++i) b1[i] = mhip_relative_position_bucket(i - dp, bins_1d, max_1d);
  for (int i = 0; i <= 2 * dx; ++i) b2[i] = mhip_relative_position_bucket(i - dx, bins_2d, max_2d);
  for (int h = 0; h < heads; ++h) {
    float* t = tab + (size_t)h * len;
    for (int i = 0; i <= 2 * dp; ++i) t[i] = w1[h * bins_1d + b1[i]] * scale;
    for (int i = 2 * dp + 1; i < off_x; ++i) t[i] = MHIP_ATTN_MASKED;
    for (int i = 0; i <= 2 * dx; ++i) {
      t[off_x + i] = wx[h * bins_2d + b2[i]] * scale;
      t[off_y + i] = wy[h * bins_2d + b2[i]] * scale;
    }
  }
}

int mhip_launch_lmv3_embed(mhip_ctx* ctx, int precision, const Lmv3EmbedDesc& d) {
  if (d.D % 256 != 0 || d.D > 1024 || d.pages <= 0 || d.coord % 4 || d.shape % 4 || 4 * d.coord + 2 * d.shape != d.D ||
      d.npad < d.max_text + d.n_vis || !d.win_page)
    return mhip_fail(ctx, MHIP_EINVAL, "lmv3_embed: D=%d coord=%d shape=%d", d.D, d.coord, d.shape);
  EmbedArgs a;
  a.tok = d.tok; a.win_page = d.win_page; a.word = d.word; a.type0 = d.type0; a.pos = d.pos; a.xe = d.xe; a.ye = d.ye; a.he = d.he; a.we = d.we;
  a.g_text = d.g_text; a.b_text = d.b_text; a.patches = d.patches; a.cls = d.cls; a.g_vis = d.g_vis; a.b_vis = d.b_vis;
  a.g_all = d.g_all; a.b_all = d.b_all; a.h = d.h; a.ht = d.ht;
  a.rows = d.pages * d.npad; a.max_text = d.max_text; a.n_vis = d.n_vis; a.npad = d.npad; a.D = d.D; a.coord = d.coord;
  a.shape = d.shape; a.eps = d.eps; a.eps_vis = d.eps_vis;
  dim3 grid((a.rows + 3) / 4), block(256);
  if (precision == MHIP_PREC_F16) PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(lmv3_embed_kernel<_Float16>, grid, block, 0, ctx->stream, a));
  else PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(lmv3_embed_kernel<float>, grid, block, 0, ctx->stream, a));
  CHECK_LAUNCH(ctx, "lmv3_embed");
  return 0;
}

int mhip_launch_lmv3_head(mhip_ctx* ctx, const float* h, int pages, int npad, int D, const float* dw, const float* db,
                          const float* ow, const float* ob, int labels, float* logits) {
  if (pages <= 0 || D > 1024 || labels < 1) return mhip_fail(ctx, MHIP_EINVAL, "lmv3_head: pages=%d D=%d labels=%d", pages, D, labels);
  PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(lmv3_head_kernel, dim3(pages), dim3(256), 0, ctx->stream, h, npad, D, dw, db, ow, ob, labels, logits));
  CHECK_LAUNCH(ctx, "lmv3_head");
  return 0;
}

// labels the token head covers at width D: TH_PASSES passes of eight, and W_o (rows of D + 8 floats) beside the four rows of x in
// the 160 KiB of LDS a workgroup may take
int mhip_token_head_max_labels(int D) {
  if (D < 4) return 0;
  const long long room = (163840ll - 4ll * D * 4) / ((D + 8) * 4ll);
  return (int)std::min<long long>(TH_PASSES * (64 / TH_GROUP), std::max<long long>(room, 0));
}

int mhip_launch_token_head(mhip_ctx* ctx, const TokenHeadDesc& d) {
  if (d.rows <= 0 || d.D < 4 || d.D % 4 || d.L < 1 || d.L > mhip_token_head_max_labels(d.D) || d.seg < 1 || d.seg_stride < d.seg ||
      !d.x || !d.w || !d.b || !d.label || !d.score)
    return mhip_fail(ctx, MHIP_EINVAL, "token_head: rows=%d D=%d labels=%d (at most %d labels at this width)", d.rows, d.D, d.L,
                     mhip_token_head_max_labels(d.D));
  TokenHeadArgs a;
  a.x = d.x; a.w = d.w; a.b = d.b; a.label = d.label; a.score = d.score; a.logits = d.logits;
  a.rows = d.rows; a.seg = d.seg; a.seg_stride = d.seg_stride; a.D = d.D; a.L = d.L; a.use_tanh = d.use_tanh;
  const size_t lds = ((size_t)d.L * (d.D + 8) + 4 * (size_t)d.D) * 4;
  if (lds > 65536)      // per device and cheap: set on every such launch
    MHIP_HIP(ctx, hipFuncSetAttribute((const void*)lmv3_token_head_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  dim3 grid((d.rows + TH_ROWS - 1) / TH_ROWS), block(256);
  PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(lmv3_token_head_kernel, grid, block, lds, ctx->stream, a));
  CHECK_LAUNCH(ctx, "token_head");
  return 0;
}
