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

}  // namespace

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
