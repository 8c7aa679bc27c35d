// clip_ops.hip — the pieces of the CLIP vision tower the other ViT paths do not have: patch extraction with CLIP's per-channel
// normalisation, the token embedding fused with pre_layrnorm, quick-GELU, the post_layernorm + projection head, and the cosine
// of embedding pairs.  (The LayerNorms of the layers are row_ops.hip's kernel, counted in clipvis_embed.)
//
// Replaces, in transformers/models/clip/modeling_clip.py: CLIPVisionEmbeddings.forward + CLIPVisionTransformer.pre_layrnorm,
// the two LayerNorms of CLIPEncoderLayer, QuickGELUActivation, post_layernorm + CLIPVisionModelWithProjection.visual_projection
// (the same arithmetic as clip/model.py: VisionTransformer.forward), the Normalize of the image processor, and the
// nn.CosineSimilarity of VQNNFTemplateMatcher.score (marie/components/template_matching/vqnnf_template_matching.py:342-347).
// (GEMMs are conv_igemm.hip; the softmax attention is attn_flash.hip.)
//
// Token layout as in vit_ops.hip: every image owns `npad` rows (npad % 8 == 0): row 0 = class token, rows 1..n_tok-1 = patches,
// the rest zeros.  The residual stream h is fp32.  All row kernels: one wave per row, loaded, normalised and stored by row_ops.h.
#include <algorithm>

#include "igemm_common.h"
#include "row_ops.h"

namespace {

// ------------------------------------------------------------------------------------------------------- patches
// clips u8 [B][S][S][3] (channel order as stored; `swap_rb`: stored channel 2 - c is model channel c)
// -> A[b * np + py * G + px][k = (c * P + y) * P + x] = (pixel / 255 - mean[c]) / std[c]
struct ChannelNorm { float mean[3], stdv[3]; };

template <typename T>
__global__ __launch_bounds__(256) void clipvis_patchify_kernel(const uint8_t* __restrict__ imgs, int S, int G, int P, int swap_rb,
                                                                ChannelNorm nrm, T* __restrict__ outs, int ld) {
  const uint8_t* img = imgs + (size_t)blockIdx.y * S * S * 3;
  T* out = outs + (size_t)blockIdx.y * G * G * ld;
  const int kchunks = 3 * P * P / 8;                 // 8 consecutive x of one (c, y)
  const long long total = (long long)G * G * kchunks;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int kc = (int)(e % kchunks), patch = (int)(e / kchunks);
    const int k0 = kc * 8;
    const int c = k0 / (P * P), y = (k0 / P) % P, x0 = k0 % P;
    const int py = patch / G, px = patch % G;
    const int sc = swap_rb ? 2 - c : c;
    const float mean = c == 0 ? nrm.mean[0] : (c == 1 ? nrm.mean[1] : nrm.mean[2]);
    const float stdv = c == 0 ? nrm.stdv[0] : (c == 1 ? nrm.stdv[1] : nrm.stdv[2]);
    const uint8_t* src = img + ((size_t)(py * P + y) * S + px * P + x0) * 3 + sc;
    T v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)(((float)src[j * 3] / 255.f - mean) / stdv);
    T* dst = out + (size_t)patch * ld + k0;
    if (sizeof(T) == 2) *(uint4v*)dst = *(uint4v*)v;
    else { *(uint4v*)dst = *(uint4v*)v; *(uint4v*)(dst + 4) = *(uint4v*)(v + 4); }
  }
}

// ------------------------------------------------------------------------------------------------------- embedding
// h[img][0] = LN(cls + pos[0]); h[img][t] = LN(patches[img][t - 1] + pos[t]) for 1 <= t < n_tok; rows n_tok.. npad-1 = 0
__global__ __launch_bounds__(256) void clipvis_embed_kernel(const float* __restrict__ patches, const float* __restrict__ cls,
                                                            const float* __restrict__ pos, const float* __restrict__ g,
                                                            const float* __restrict__ b, float* __restrict__ h, int rows,
                                                            int npad, int n_tok, int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int img = row / npad, t = row % npad;
  float4v v[ROW_GROUPS] = {};
  if (t < n_tok) {
    row_load(v, t == 0 ? cls : patches + ((size_t)img * (n_tok - 1) + t - 1) * D, D, lane);
    row_add(v, pos + (size_t)t * D, D, lane);
    row_layernorm(v, D, lane, g, b, eps);
  }
  row_store<float>(v, h + (size_t)row * D, nullptr, D, lane);
}

// ------------------------------------------------------------------------------------------------------- quick-GELU
// x <- x * sigmoid(1.702 x) in place, 16 bytes a lane (n % (16 / sizeof(T)) == 0), evaluated in fp32
__device__ __forceinline__ float quick_gelu(float x) { return x / (1.f + __expf(-1.702f * x)); }

template <typename T>
__global__ __launch_bounds__(256) void quick_gelu_kernel(T* __restrict__ x, long long n) {
  constexpr int V = 16 / sizeof(T);
  for (long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * V; e < n; e += (long long)gridDim.x * 256 * V) {
    uint4v raw = *(const uint4v*)(x + e);
    T* v = (T*)&raw;
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = (T)quick_gelu((float)v[j]);
    *(uint4v*)(x + e) = raw;
  }
}

// ------------------------------------------------------------------------------------------------------- head
// y = LN(h[img][row_of ? row_of[img] : 0]) (post_layernorm / ln_final), emb[img][j] = sum_k y[k] * proj_t[j][k] (no bias).  proj_t is the projection transposed,
// [E][D] fp32: a wave per output, lanes along k.  A workgroup takes HEAD_COLS outputs of one image and normalises the row for
// itself (one row: cheaper than a pass that stores it); one workgroup an image left 64 of them walking the whole matrix
// (134 us at B = 64).
constexpr int HEAD_COLS = 32;

__global__ __launch_bounds__(256) void clipvis_head_kernel(const float* __restrict__ h, int npad, int D, const float* __restrict__ g,
                                                           const float* __restrict__ b, float eps, const float* __restrict__ proj_t,
                                                           int E, float* __restrict__ emb, const int* __restrict__ row_of) {
  __shared__ __attribute__((aligned(16))) float ys[1024];
  const int img = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave == 0) {
    float4v v[ROW_GROUPS];
    row_load(v, h + ((size_t)img * npad + (row_of ? row_of[img] : 0)) * D, D, lane);
    row_layernorm(v, D, lane, g, b, eps);
    row_store<float>(v, ys, nullptr, D, lane);
  }
  __syncthreads();
  const int j0 = blockIdx.y * HEAD_COLS, j1 = min(j0 + HEAD_COLS, E);
  for (int j = j0 + wave; j < j1; j += 4) {
    const float* w = proj_t + (size_t)j * D;
    float acc = 0.f;
    for (int k = lane * 4; k < D; k += 256) {
      const float4v ww = *(const float4v*)(w + k), yy = *(const float4v*)(ys + k);
      acc += (ww[0] * yy[0] + ww[1] * yy[1]) + (ww[2] * yy[2] + ww[3] * yy[3]);
    }
    acc = wave_sum(acc);
    if (lane == 0) emb[(size_t)img * E + j] = acc;
  }
}

// ------------------------------------------------------------------------------------------------------- pair cosine
// out[p] = x . y / max(|x| |y|, 1e-8) for x = emb[a[p]], y = emb[b[p]]; one wave per pair.  |x| |y| is taken as
// sqrt(|x|^2 |y|^2): a pair of one vector with itself gives exactly 1.
__global__ __launch_bounds__(256) void pair_cosine_kernel(const float* __restrict__ emb, int E, const int* __restrict__ pa,
                                                          const int* __restrict__ pb, int n_pairs, float* __restrict__ out) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= n_pairs) return;
  const float* x = emb + (size_t)pa[p] * E;
  const float* y = emb + (size_t)pb[p] * E;
  float xy = 0.f, xx = 0.f, yy = 0.f;
  for (int k = lane; k < E; k += 64) {
    const float a = x[k], c = y[k];
    xy += a * c; xx += a * a; yy += c * c;
  }
  xy = wave_sum(xy); xx = wave_sum(xx); yy = wave_sum(yy);
  if (lane == 0) out[p] = xy / fmaxf(sqrtf(xx * yy), 1e-8f);
}

}  // namespace

int mhip_launch_clipvis_patchify(mhip_ctx* ctx, int precision, const uint8_t* imgs, int B, int S, int P, int swap_rb,
                                 const float mean[3], const float stdv[3], void* out, int ld) {
  if (B <= 0 || P < 8 || P % 8 || S < P || S % P || ld < 3 * P * P) return mhip_fail(ctx, MHIP_EINVAL, "clipvis_patchify: B=%d S=%d P=%d", B, S, P);
  ChannelNorm n;
  for (int c = 0; c < 3; ++c) { n.mean[c] = mean[c]; n.stdv[c] = stdv[c]; }
  const int G = S / P;
  const long long total = (long long)G * G * (3 * P * P / 8);
  dim3 grid((unsigned)std::min<long long>((total + 255) / 256, 4096), B), block(256);
  if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_CLIPVIS_PATCHIFY, hipLaunchKernelGGL(clipvis_patchify_kernel<_Float16>, grid, block, 0, ctx->stream, imgs, S, G, P, swap_rb, n, (_Float16*)out, ld));
  else
    PROF_LAUNCH(ctx, MHIP_K_CLIPVIS_PATCHIFY, hipLaunchKernelGGL(clipvis_patchify_kernel<float>, grid, block, 0, ctx->stream, imgs, S, G, P, swap_rb, n, (float*)out, ld));
  CHECK_LAUNCH(ctx, "clipvis_patchify");
  return 0;
}

int mhip_launch_clipvis_embed(mhip_ctx* ctx, const float* patches, const float* cls, const float* pos, const float* g, const float* b,
                              float* h, int B, int npad, int n_tok, int D, float eps) {
  if (B <= 0 || !row_width_ok(D) || n_tok < 2 || npad < n_tok) return mhip_fail(ctx, MHIP_EINVAL, "clipvis_embed: B=%d D=%d tokens %d/%d", B, D, n_tok, npad);
  const int rows = B * npad;
  PROF_LAUNCH(ctx, MHIP_K_CLIPVIS_EMBED, hipLaunchKernelGGL(clipvis_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, ctx->stream, patches, cls, pos, g, b, h, rows, npad, n_tok, D, eps));
  CHECK_LAUNCH(ctx, "clipvis_embed");
  return 0;
}

int mhip_launch_quick_gelu(mhip_ctx* ctx, int precision, void* x, long long n) {
  const int V = precision == MHIP_PREC_F16 ? 8 : 4;
  if (n <= 0 || n % V || ((uintptr_t)x & 15)) return mhip_fail(ctx, MHIP_EINVAL, "quick_gelu: n=%lld must be a multiple of %d on a 16-byte boundary", n, V);
  dim3 grid(grid_for(n / V, 256)), block(256);
  if (precision == MHIP_PREC_F16) PROF_LAUNCH(ctx, MHIP_K_QUICK_GELU, hipLaunchKernelGGL(quick_gelu_kernel<_Float16>, grid, block, 0, ctx->stream, (_Float16*)x, n));
  else PROF_LAUNCH(ctx, MHIP_K_QUICK_GELU, hipLaunchKernelGGL(quick_gelu_kernel<float>, grid, block, 0, ctx->stream, (float*)x, n));
  CHECK_LAUNCH(ctx, "quick_gelu");
  return 0;
}

int mhip_launch_clipvis_head(mhip_ctx* ctx, const float* h, int B, int npad, int D, const float* g, const float* b, float eps,
                             const float* proj_t, int E, float* emb, const int* row_of) {
  if (B <= 0 || npad < 1 || !row_width_ok(D) || E < 1 || E > 65535 * HEAD_COLS) return mhip_fail(ctx, MHIP_EINVAL, "clipvis_head: B=%d D=%d E=%d", B, D, E);
  PROF_LAUNCH(ctx, MHIP_K_CLIPVIS_HEAD, hipLaunchKernelGGL(clipvis_head_kernel, dim3(B, (E + HEAD_COLS - 1) / HEAD_COLS), dim3(256), 0, ctx->stream, h, npad, D, g, b, eps, proj_t, E, emb, row_of));
  CHECK_LAUNCH(ctx, "clipvis_head");
  return 0;
}

int mhip_launch_pair_cosine(mhip_ctx* ctx, const float* emb, int E, const int* pair_a, const int* pair_b, int n_pairs, float* out) {
  if (E < 1 || n_pairs <= 0) return mhip_fail(ctx, MHIP_EINVAL, "pair_cosine: E=%d pairs=%d", E, n_pairs);
  PROF_LAUNCH(ctx, MHIP_K_PAIR_COSINE, hipLaunchKernelGGL(pair_cosine_kernel, dim3((n_pairs + 3) / 4), dim3(256), 0, ctx->stream, emb, E, pair_a, pair_b, n_pairs, out));
  CHECK_LAUNCH(ctx, "pair_cosine");
  return 0;
}
