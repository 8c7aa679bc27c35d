// berttext_ops.hip — the kernels of the BERT sentence encoders (berttext_api.hip) the other towers do not have: the embedding +
// LayerNorm front (its row load, LayerNorm and store are row_ops.h's), GEGLU and masked pooling.  (Their attention over sequences
// of different lengths, attn_short and attn_long, is attn_seq.hip; the post-LayerNorms of the layers are row_ops.hip's kernel,
// counted in berttext_embed.)
//
// Replaces, in transformers/models/bert/modeling_bert.py: BertEmbeddings.forward (and the embeddings of RoBERTa and MPNet, whose
// position rows start at pad_id + 1, and of DistilBERT and MPNet, which have no token types), the LayerNorms of BertSelfOutput /
// BertOutput;
// of JinaBERT the gated MLP's activation; and the Pooling (mean / cls) and Normalize modules of sentence_transformers.
#include "igemm_common.h"
#include "row_ops.h"

using namespace igemm;

namespace {

// ------------------------------------------------------------------------------------------------------- rows
// h[seq][t] = LN((word[ids[seq][t]] + type0) + pos[pos_offset + t]) (type0 null: no token types; pos null: no position table), one
// wave per row, 16 bytes a lane
template <typename T>
__global__ __launch_bounds__(256) void berttext_embed_kernel(const float* __restrict__ word, const float* __restrict__ type0,
                                                             const float* __restrict__ pos, const float* __restrict__ g,
                                                             const float* __restrict__ b, const int* __restrict__ ids,
                                                             float* __restrict__ h, T* __restrict__ ht, int rows, int npad, int D,
                                                             float eps, int pos_offset) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* src = word + (size_t)ids[row] * D;
  const float* pp = pos ? pos + (size_t)(pos_offset + row % npad) * D : nullptr;
  float4v v[ROW_GROUPS];
  row_load(v, src, D, lane);
  if (type0) row_add(v, type0, D, lane);
  if (pp) row_add(v, pp, D, lane);
  row_layernorm(v, D, lane, g, b, eps);
  row_store<T>(v, h + (size_t)row * D, ht ? ht + (size_t)row * D : nullptr, D, lane);
}

// ------------------------------------------------------------------------------------------------------- GEGLU
// out[r][f] = gelu_erf(x[r][f]) * x[r][F + f], 16 bytes a lane, evaluated in fp32
template <typename T>
__global__ __launch_bounds__(256) void geglu_kernel(const T* __restrict__ x, T* __restrict__ out, long long R, int F) {
  constexpr int V = 16 / sizeof(T);
  const int fc = F / V;
  const long long total = R * fc;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long r = e / fc;
    const int f = (int)(e % fc) * V;
    uint4v ra = *(const uint4v*)(x + r * 2 * F + f), rb = *(const uint4v*)(x + r * 2 * F + F + f);
    const T* a = (const T*)&ra;
    const T* b = (const T*)&rb;
    uint4v ro;
    T* o = (T*)&ro;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = (T)(gelu_erf((float)a[j]) * (float)b[j]);
    *(uint4v*)(out + r * F + f) = ro;
  }
}

// ------------------------------------------------------------------------------------------------------- pooling
// emb[b] = sum over t < len[b] of h[b][t] / len[b] (mean) or h[b][0] (cls), then / max(|emb[b]|, 1e-12) with `normalize`.  One
// workgroup a sequence, a thread per float4 of columns: the rows are summed one after another, so the order is len's alone.
__global__ __launch_bounds__(256) void berttext_pool_kernel(const float* __restrict__ h, const int* __restrict__ len, int npad, int D,
                                                            int cls, int normalize, float* __restrict__ emb) {
  __shared__ float part[4];
  const int b = blockIdx.x, c = threadIdx.x * 4, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = h + (size_t)b * npad * D;
  float4v acc = {0.f, 0.f, 0.f, 0.f};
  if (c < D) {
    if (cls) {
      acc = *(const float4v*)(x + c);
    } else {
      const int n = min(max(len[b], 1), npad);
      for (int t = 0; t < n; ++t) acc += *(const float4v*)(x + (size_t)t * D + c);
      acc = acc / fmaxf((float)n, 1e-9f);
    }
  }
  if (normalize) {
    const float q = wave_sum((acc[0] * acc[0] + acc[1] * acc[1]) + (acc[2] * acc[2] + acc[3] * acc[3]));
    if (lane == 0) part[wave] = q;
    __syncthreads();
    acc = acc / fmaxf(sqrtf((part[0] + part[1]) + (part[2] + part[3])), 1e-12f);
  }
  if (c < D) *(float4v*)(emb + (size_t)b * D + c) = acc;
}

// ------------------------------------------------------------------------------------------------------- the global token's query
// out[b][o] = bias[o] + sum_k x[b * x_rows][k] w[o][k]: a wave per output, 16 bytes a lane and step, fp32 sums
template <typename T>
__global__ __launch_bounds__(256) void first_row_linear_kernel(const T* __restrict__ x, long long x_rows, const T* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ out, int N, int K) {
  constexpr int V = 16 / sizeof(T);
  const int b = blockIdx.y, o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (o >= N) return;
  const T* xr = x + (size_t)b * x_rows * K;
  const T* wr = w + (size_t)o * K;
  float acc = 0.f;
  for (int k = lane * V; k < K; k += 64 * V) {
    const uint4v rx = *(const uint4v*)(xr + k), rw = *(const uint4v*)(wr + k);
    const T* xv = (const T*)&rx;
    const T* wv = (const T*)&rw;
#pragma unroll
    for (int j = 0; j < V; ++j) acc += (float)xv[j] * (float)wv[j];
  }
  acc = wave_sum(acc);
  if (lane == 0) out[(size_t)b * N + o] = acc + (bias ? bias[o] : 0.f);
}

// ------------------------------------------------------------------------------------------------------- classification head
// One workgroup a text: x = h[b * h_rows] -> y = tanh(dense_w x + dense_b) -> logits = out_w y + out_b -> scores.  A wave per
// output, a float4 a lane and step; the soft-max's maximum and sum are taken by every thread over the L logits in LDS, in order
__global__ __launch_bounds__(256) void cls_head_kernel(const float* __restrict__ h, long long h_rows, const float* __restrict__ dense_w,
                                                       const float* __restrict__ dense_b, const float* __restrict__ out_w,
                                                       const float* __restrict__ out_b, int D, int L, int function,
                                                       float* __restrict__ logits, float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) float xs[1024];
  __shared__ __attribute__((aligned(16))) float ys[1024];
  __shared__ float ls[CLS_HEAD_MAX_LABELS];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = h + (size_t)b * h_rows * D;
  for (int c = tid; c < D; c += 256) xs[c] = x[c];
  __syncthreads();
  for (int o = wave; o < D; o += 4) {
    const float* wr = dense_w + (size_t)o * D;
    float acc = 0.f;
    for (int k = lane * 4; k < D; k += 256) {
      const float4v a = *(const float4v*)(wr + k), v = *(const float4v*)(xs + k);
      acc += (a[0] * v[0] + a[1] * v[1]) + (a[2] * v[2] + a[3] * v[3]);
    }
    acc = wave_sum(acc);
    if (lane == 0) ys[o] = tanhf(acc + dense_b[o]);
  }
  __syncthreads();
  for (int o = wave; o < L; o += 4) {
    const float* wr = out_w + (size_t)o * D;
    float acc = 0.f;
    for (int k = lane * 4; k < D; k += 256) {
      const float4v a = *(const float4v*)(wr + k), v = *(const float4v*)(ys + k);
      acc += (a[0] * v[0] + a[1] * v[1]) + (a[2] * v[2] + a[3] * v[3]);
    }
    acc = wave_sum(acc);
    if (lane == 0) ls[o] = acc + out_b[o];
  }
  __syncthreads();
  float mx = 0.f, inv = 1.f;
  if (function == 1) {
    mx = -INFINITY;
    for (int o = 0; o < L; ++o) mx = fmaxf(mx, ls[o]);
    float sum = 0.f;
    for (int o = 0; o < L; ++o) sum += expf(ls[o] - mx);
    inv = 1.f / sum;
  }
  for (int o = tid; o < L; o += 256) {
    const float z = ls[o];
    logits[(size_t)b * L + o] = z;
    scores[(size_t)b * L + o] = function == 1 ? expf(z - mx) * inv : function == 2 ? 1.f / (1.f + expf(-z)) : z;
  }
}

}  // namespace

int mhip_launch_first_row_linear(mhip_ctx* ctx, int precision, const void* x, long long x_rows, const void* w, const float* bias, float* out,
                                 int B, int N, int K) {
  if (!x || !w || !out || B <= 0 || B > 65535 || N <= 0 || K < 8 || K % 8 || x_rows < 1 || ((uintptr_t)x & 15) || ((uintptr_t)w & 15))
    return mhip_fail(ctx, MHIP_EINVAL, "first_row_linear: B=%d N=%d K=%d (K a multiple of 8, 16-byte rows)", B, N, K);
  dim3 grid((N + 3) / 4, B), block(256);
  if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_BERTTEXT_POOL, hipLaunchKernelGGL(first_row_linear_kernel<_Float16>, grid, block, 0, ctx->stream, (const _Float16*)x, x_rows, (const _Float16*)w, bias, out, N, K));
  else
    PROF_LAUNCH(ctx, MHIP_K_BERTTEXT_POOL, hipLaunchKernelGGL(first_row_linear_kernel<float>, grid, block, 0, ctx->stream, (const float*)x, x_rows, (const float*)w, bias, out, N, K));
  CHECK_LAUNCH(ctx, "first_row_linear");
  return 0;
}

int mhip_launch_cls_head(mhip_ctx* ctx, const float* h, long long h_rows, const float* dense_w, const float* dense_b, const float* out_w,
                         const float* out_b, int B, int D, int L, int function, float* logits, float* scores) {
  if (!h || !dense_w || !dense_b || !out_w || !out_b || !logits || !scores || B <= 0 || D < 4 || D % 4 || D > 1024 || L < 1 ||
      L > CLS_HEAD_MAX_LABELS || h_rows < 1 || function < 0 || function > 2)
    return mhip_fail(ctx, MHIP_EINVAL, "cls_head: B=%d D=%d L=%d function=%d (D a multiple of 4 up to 1024, L up to %d, function 0 .. 2)", B, D, L,
                     function, CLS_HEAD_MAX_LABELS);
  // counted with the pooling: the profiler's list is pinned, and both are the call's last kernel over B rows
  PROF_LAUNCH(ctx, MHIP_K_BERTTEXT_POOL, hipLaunchKernelGGL(cls_head_kernel, dim3(B), dim3(256), 0, ctx->stream, h, h_rows, dense_w, dense_b, out_w, out_b, D, L, function, logits, scores));
  CHECK_LAUNCH(ctx, "cls_head");
  return 0;
}

int mhip_launch_berttext_embed(mhip_ctx* ctx, int precision, const float* word, const float* type0, const float* pos, const float* g,
                               const float* b, float eps, const int* ids, float* h, void* ht, int B, int npad, int D, int pos_offset) {
  if (B <= 0 || npad < 1 || !row_width_ok(D) || pos_offset < 0) return mhip_fail(ctx, MHIP_EINVAL, "berttext_embed: B=%d npad=%d D=%d", B, npad, D);
  const int rows = B * npad;
  dim3 grid((rows + 3) / 4), block(256);
  if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_BERTTEXT_EMBED, hipLaunchKernelGGL(berttext_embed_kernel<_Float16>, grid, block, 0, ctx->stream, word, type0, pos, g, b, ids, h, (_Float16*)ht, rows, npad, D, eps, pos_offset));
  else
    PROF_LAUNCH(ctx, MHIP_K_BERTTEXT_EMBED, hipLaunchKernelGGL(berttext_embed_kernel<float>, grid, block, 0, ctx->stream, word, type0, pos, g, b, ids, h, (float*)ht, rows, npad, D, eps, pos_offset));
  CHECK_LAUNCH(ctx, "berttext_embed");
  return 0;
}

int mhip_launch_geglu(mhip_ctx* ctx, int precision, const void* x, void* out, long long R, int F) {
  if (R <= 0 || F < 8 || F % 8 || ((uintptr_t)x & 15) || ((uintptr_t)out & 15)) return mhip_fail(ctx, MHIP_EINVAL, "geglu: R=%lld F=%d (a multiple of 8, 16-byte rows)", R, F);
  const int V = precision == MHIP_PREC_F16 ? 8 : 4;
  dim3 grid(grid_for(R * (F / V), 256)), block(256);
  if (precision == MHIP_PREC_F16) PROF_LAUNCH(ctx, MHIP_K_GEGLU, hipLaunchKernelGGL(geglu_kernel<_Float16>, grid, block, 0, ctx->stream, (const _Float16*)x, (_Float16*)out, R, F));
  else PROF_LAUNCH(ctx, MHIP_K_GEGLU, hipLaunchKernelGGL(geglu_kernel<float>, grid, block, 0, ctx->stream, (const float*)x, (float*)out, R, F));
  CHECK_LAUNCH(ctx, "geglu");
  return 0;
}

int mhip_launch_berttext_pool(mhip_ctx* ctx, const float* h, const int* len, int B, int npad, int D, int cls, int normalize, float* emb) {
  if (B <= 0 || npad < 1 || !row_width_ok(D) || (!cls && !len)) return mhip_fail(ctx, MHIP_EINVAL, "berttext_pool: B=%d npad=%d D=%d", B, npad, D);
  PROF_LAUNCH(ctx, MHIP_K_BERTTEXT_POOL, hipLaunchKernelGGL(berttext_pool_kernel, dim3(B), dim3(256), 0, ctx->stream, h, len, npad, D, cls, normalize, emb));
  CHECK_LAUNCH(ctx, "berttext_pool");
  return 0;
}
