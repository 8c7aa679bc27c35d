// vit_ops.hip — the non-GEMM pieces of the ViT encoder stack shared by the DiT detector backbone and the TrOCR encoder:
// patch extraction, token <-> feature-map moves, bicubic position-embedding resize.
//
// Replaces, in marie/boxes/dit/ditod/beit.py: PatchEmbed's patch gather + bicubic pos-emb resize (:362-376), and the token ->
// NCHW tap reshape of forward_features (:730-732).  (GEMMs — qkv, proj, fc1, fc2, patch projection — are conv_igemm.hip; the
// softmax attention is attn_flash.hip; Block's nn.LayerNorm is row_ops.hip's kernel, counted in vit_ops.)
//
// Token layout: every image owns `npad` consecutive rows (npad % 8 == 0): row 0 = cls, rows 1..n_tok-1 = patches,
// the rest padding (finite values, masked as keys).  The residual stream is fp32; GEMM operands are T (f16 / fp32).
#include <algorithm>

#include "igemm_common.h"

using namespace igemm;

namespace {

// ------------------------------------------------------------------------------------------------------- patches
// resized page u8 [th][tw][3] (channel order as stored; `swap_rb` selects which stored channel is model channel 0)
// -> A[row0 + py*wp + px][k = (c*P + y)*P + x] = (pixel - mean) / std, or 0 outside (th, tw)   (zero canvas padding)
template <typename T>
__global__ __launch_bounds__(256) void patchify_kernel(const uint8_t* __restrict__ imgs, int th, int tw, int hp, int wp,
                                                        int P, int swap_rb, float mean, float stdv, T* __restrict__ outs,
                                                        int ld) {
  const uint8_t* img = imgs + (size_t)blockIdx.y * th * tw * 3;        // image blockIdx.y of the batch
  T* out = outs + (size_t)blockIdx.y * hp * wp * ld;
  const int kchunks = 3 * P * P / 8;                 // 8 consecutive x of one (c, y)
  const long long total = (long long)hp * wp * kchunks;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int kc = (int)(e % kchunks);
    const int patch = (int)(e / kchunks);
    const int k0 = kc * 8;
    const int c = k0 / (P * P), y = (k0 / P) % P, x0 = k0 % P;
    const int py = patch / wp, px = patch % wp;
    const int iy = py * P + y, sc = swap_rb ? 2 - c : c;
    T v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ix = px * P + x0 + j;
      float f = 0.f;
      if (iy < th && ix < tw) f = ((float)img[((size_t)iy * tw + ix) * 3 + sc] - mean) / stdv;
      v[j] = (T)f;
    }
    T* dst = out + (size_t)patch * ld + k0;
    if (sizeof(T) == 2) *(uint4v*)dst = *(uint4v*)v;
    else { *(uint4v*)dst = *(uint4v*)v; *(uint4v*)(dst + 4) = *(uint4v*)(v + 4); }
  }
}

// x[img][0] = cls + pos[0]; rows n_tok.. npad-1 = 0   (fp32 residual stream)
template <typename XT>
__global__ void token_init_kernel(XT* x, const float* cls_row, int B, int npad, int n_tok, int D) {
  const int rows_per = 1 + (npad - n_tok);
  const long long total = (long long)B * rows_per * D;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int d = (int)(e % D);
    const int r = (int)((e / D) % rows_per), b = (int)(e / ((long long)D * rows_per));
    const int row = r == 0 ? 0 : n_tok + r - 1;
    x[((size_t)b * npad + row) * D + d] = (XT)(r == 0 ? cls_row[d] : 0.f);
  }
}

// The split stream (x = hi + lo, two f16 planes; conv_igemm's EPI_SPLIT keeps it): cls row and pad rows of every image, and their
// row statistics per 64-column chunk — (sum, centred sum of squares), the cls row's precomputed on the host (cls_stats[chunk][2])
__global__ void token_init_split_kernel(_Float16* hi, _Float16* lo, const float* cls_row, const float* cls_stats, float* stats,
                                        int stats_ld, int B, int npad, int n_tok, int D) {
  const int rows_per = 1 + (npad - n_tok);
  const long long total = (long long)B * rows_per * D;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int d = (int)(e % D);
    const int r = (int)((e / D) % rows_per), b = (int)(e / ((long long)D * rows_per));
    const int row = r == 0 ? 0 : n_tok + r - 1;
    const float v = r == 0 ? cls_row[d] : 0.f;
    const _Float16 h = (_Float16)v;
    const size_t o = ((size_t)b * npad + row) * D + d;
    hi[o] = h;
    lo[o] = (_Float16)(v - (float)h);
    if ((d & 63) == 0) {
      const int c = d >> 6;
      float* st = stats + ((size_t)c * stats_ld + (size_t)b * npad + row) * 2;
      st[0] = r == 0 ? cls_stats[c * 2] : 0.f;
      st[1] = r == 0 ? cls_stats[c * 2 + 1] : 0.f;
    }
  }
}

// row statistics of the split stream -> rstd and mean * rstd per row.  stats[(chunk * ld + row) * 2] = (sum, centred sum of squares)
// of the row over the 64 columns of the chunk; merged the pairwise way (Chan et al.): no cancellation of large means.
__global__ void ln_finalize_kernel(const float* __restrict__ stats, int chunks, int ld, float* __restrict__ rstd,
                                   float* __restrict__ mur, int rows, int D, float eps) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float s[16], q[16], tot = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if (c < chunks) {
      const float2 v = *(const float2*)(stats + ((size_t)c * ld + r) * 2);
      s[c] = v.x; q[c] = v.y; tot += v.x;
    }
  const float mean = tot / (float)D;
  float m2 = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if (c < chunks) { const float d = s[c] * (1.f / 64.f) - mean; m2 += q[c] + 64.f * d * d; }
  const float rs = 1.f / sqrtf(m2 / (float)D + eps);
  rstd[r] = rs;
  mur[r] = mean * rs;
}

__global__ void split_f16_kernel(const float* __restrict__ in, _Float16* __restrict__ hi, _Float16* __restrict__ lo, long long n) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const float v = in[e];
    const _Float16 h = (_Float16)v;
    hi[e] = h;
    lo[e] = (_Float16)(v - (float)h);
  }
}

__global__ void join_f16_kernel(const _Float16* __restrict__ hi, const _Float16* __restrict__ lo, float* __restrict__ out, long long n) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) out[e] = (float)hi[e] + (float)lo[e];
}

// fp32 tokens (without cls) -> T feature map rows [B][n_tok-1][D]
template <typename T, typename XT>
__global__ void tokens_to_map_kernel(const XT* __restrict__ x, T* __restrict__ out, int B, int npad, int np, int D) {
  const long long total = (long long)B * np * (D / 4);
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int c4 = (int)(e % (D / 4));
    const long long r = e / (D / 4);
    const int pidx = (int)(r % np), b = (int)(r / np);
    const XT* src = x + ((size_t)b * npad + 1 + pidx) * D + c4 * 4;
    T o4[4] = {(T)src[0], (T)src[1], (T)src[2], (T)src[3]};
    T* dst = out + ((size_t)b * np + pidx) * D + c4 * 4;
    if (sizeof(T) == 2) *(uint64_t*)dst = *(uint64_t*)o4;
    else *(float4v*)dst = *(float4v*)o4;
  }
}

// torch F.interpolate(mode="bicubic", align_corners=False) of a [gh][gw][D] table to [hp][wp][D]  (A = -0.75,
// source index scale*(dst+0.5)-0.5 unclamped, taps clamped to the border), fp32.
__device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
  const float A = -0.75f;
  float x = t + 1.f;
  c[0] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
  x = t;
  c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 1.f - t;
  c[2] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 2.f - t;
  c[3] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
}

__global__ void posemb_bicubic_kernel(const float* __restrict__ tab, int gh, int gw, float* __restrict__ out, int hp,
                                      int wp, int D) {
  const long long total = (long long)hp * wp * D;
  const float sy = (float)gh / (float)hp, sx = (float)gw / (float)wp;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int d = (int)(e % D);
    const int ox = (int)((e / D) % wp), oy = (int)(e / ((long long)D * wp));
    const float ry = sy * ((float)oy + 0.5f) - 0.5f, rx = sx * ((float)ox + 0.5f) - 0.5f;
    const int iy = (int)floorf(ry), ix = (int)floorf(rx);
    float cy[4], cx[4];
    cubic_coeffs(ry - (float)iy, cy);
    cubic_coeffs(rx - (float)ix, cx);
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int yy = min(max(iy - 1 + a, 0), gh - 1);
      float row = 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int xx = min(max(ix - 1 + b, 0), gw - 1);
        row += tab[((size_t)yy * gw + xx) * D + d] * cx[b];
      }
      acc += row * cy[a];
    }
    out[e] = acc;
  }
}

// T rows -> fp32 rows (test / host read-back path)
template <typename T>
__global__ void convert_rows_kernel(const T* __restrict__ in, float* __restrict__ out, long long n) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) out[e] = (float)in[e];
}

__global__ void narrow_f16_kernel(const float* __restrict__ in, _Float16* __restrict__ out, long long n) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) out[e] = (_Float16)in[e];
}

// nested 2x2 row order (depth `nest`) -> raster NHWC, optionally adding the 2x nearest-upsampled coarser level
// (FPN top-down path: F.interpolate(scale_factor=2, mode="nearest") + lateral).  OT = T or float.
template <typename T, typename OT>
__global__ void unnest_kernel(const T* __restrict__ in, const T* __restrict__ coarse, OT* __restrict__ out, int B, int H,
                              int W, int C, int nest) {
  const long long total = (long long)B * H * W * (C / 4);
  const int h0 = H >> nest, w0 = W >> nest;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int c4 = (int)(e % (C / 4));
    long long r = e / (C / 4);
    const int X = (int)(r % W);
    r /= W;
    const int Y = (int)(r % H), b = (int)(r / H);
    long long row = ((long long)b * h0 + (Y >> nest)) * w0 + (X >> nest);
    for (int l = nest - 1; l >= 0; --l) row = row * 4 + (((Y >> l) & 1) * 2 + ((X >> l) & 1));
    const T* src = in + row * C + c4 * 4;
    float v[4] = {(float)src[0], (float)src[1], (float)src[2], (float)src[3]};
    if (coarse) {
      const T* cs = coarse + (((long long)b * (H / 2) + (Y >> 1)) * (W / 2) + (X >> 1)) * C + c4 * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += (float)cs[k];
    }
    OT* dst = out + (((long long)b * H + Y) * W + X) * C + c4 * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = (OT)v[k];
  }
}

}  // namespace

int mhip_launch_patchify(mhip_ctx* ctx, int precision, const uint8_t* img, int B, int th, int tw, int hp, int wp, int P,
                         int swap_rb, float mean, float stdv, void* out, int ld) {
  if (P != 16 && P != 8) return mhip_fail(ctx, MHIP_EINVAL, "patchify: patch size %d", P);
  const long long total = (long long)hp * wp * (3 * P * P / 8);
  dim3 grid((unsigned)std::min<long long>((total + 255) / 256, 4096), B), block(256);
  if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(patchify_kernel<_Float16>, grid, block, 0, ctx->stream, img, th, tw, hp, wp, P, swap_rb, mean, stdv, (_Float16*)out, ld));
  else
    PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(patchify_kernel<float>, grid, block, 0, ctx->stream, img, th, tw, hp, wp, P, swap_rb, mean, stdv, (float*)out, ld));
  CHECK_LAUNCH(ctx, "patchify");
  return 0;
}

int mhip_launch_token_init(mhip_ctx* ctx, void* x, const float* cls_row, int B, int npad, int n_tok, int D, int x_f16) {
  const long long total = (long long)B * (1 + npad - n_tok) * D;
  if (x_f16)
    PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(token_init_kernel<_Float16>, dim3(grid_for(total, 256)), dim3(256), 0, ctx->stream, (_Float16*)x, cls_row, B, npad, n_tok, D));
  else
    PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(token_init_kernel<float>, dim3(grid_for(total, 256)), dim3(256), 0, ctx->stream, (float*)x, cls_row, B, npad, n_tok, D));
  CHECK_LAUNCH(ctx, "token_init");
  return 0;
}

int mhip_launch_token_init_split(mhip_ctx* ctx, void* hi, void* lo, const float* cls_row, const float* cls_stats, float* stats,
                                 int stats_ld, int B, int npad, int n_tok, int D) {
  if (D % 64 != 0 || D > 1024) return mhip_fail(ctx, MHIP_EINVAL, "token_init_split: D=%d", D);
  const long long total = (long long)B * (1 + npad - n_tok) * D;
  PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(token_init_split_kernel, dim3(grid_for(total, 256)), dim3(256), 0, ctx->stream, (_Float16*)hi, (_Float16*)lo, cls_row, cls_stats, stats, stats_ld, B, npad, n_tok, D));
  CHECK_LAUNCH(ctx, "token_init_split");
  return 0;
}

int mhip_launch_ln_finalize(mhip_ctx* ctx, const float* stats, int chunks, int ld, float* rstd, float* mur, int rows, int D, float eps) {
  if (chunks < 1 || chunks > 16 || chunks * 64 != D || rows <= 0) return mhip_fail(ctx, MHIP_EINVAL, "ln_finalize: chunks=%d D=%d rows=%d", chunks, D, rows);
  PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(ln_finalize_kernel, dim3((rows + 255) / 256), dim3(256), 0, ctx->stream, stats, chunks, ld, rstd, mur, rows, D, eps));
  CHECK_LAUNCH(ctx, "ln_finalize");
  return 0;
}

int mhip_launch_split_f16(mhip_ctx* ctx, const float* in, void* hi, void* lo, long long n) {
  PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(split_f16_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, in, (_Float16*)hi, (_Float16*)lo, n));
  CHECK_LAUNCH(ctx, "split_f16");
  return 0;
}

int mhip_launch_join_f16(mhip_ctx* ctx, const void* hi, const void* lo, float* out, long long n) {
  PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(join_f16_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, (const _Float16*)hi, (const _Float16*)lo, out, n));
  CHECK_LAUNCH(ctx, "join_f16");
  return 0;
}

int mhip_launch_tokens_to_map(mhip_ctx* ctx, int precision, const void* x, void* out, int B, int npad, int np, int D, int x_f16) {
  const long long total = (long long)B * np * (D / 4);
  dim3 grid(grid_for(total, 256)), block(256);
  if (precision == MHIP_PREC_F16 && x_f16)
    PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL((tokens_to_map_kernel<_Float16, _Float16>), grid, block, 0, ctx->stream, (const _Float16*)x, (_Float16*)out, B, npad, np, D));
  else if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL((tokens_to_map_kernel<_Float16, float>), grid, block, 0, ctx->stream, (const float*)x, (_Float16*)out, B, npad, np, D));
  else
    PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL((tokens_to_map_kernel<float, float>), grid, block, 0, ctx->stream, (const float*)x, (float*)out, B, npad, np, D));
  CHECK_LAUNCH(ctx, "tokens_to_map");
  return 0;
}

int mhip_launch_posemb_bicubic(mhip_ctx* ctx, const float* tab, int gh, int gw, float* out, int hp, int wp, int D) {
  const long long total = (long long)hp * wp * D;
  PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(posemb_bicubic_kernel, dim3(grid_for(total, 256)), dim3(256), 0, ctx->stream, tab, gh, gw, out, hp, wp, D));
  CHECK_LAUNCH(ctx, "posemb_bicubic");
  return 0;
}

int mhip_launch_convert_rows(mhip_ctx* ctx, int precision, const void* in, float* out, int rows, int D) {
  const long long n = (long long)rows * D;
  dim3 grid(grid_for(n, 256)), block(256);
  if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(convert_rows_kernel<_Float16>, grid, block, 0, ctx->stream, (const _Float16*)in, out, n));
  else
    PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(convert_rows_kernel<float>, grid, block, 0, ctx->stream, (const float*)in, out, n));
  CHECK_LAUNCH(ctx, "convert_rows");
  return 0;
}

int mhip_launch_narrow_f16(mhip_ctx* ctx, const float* in, void* out, long long n) {
  PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(narrow_f16_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, in, (_Float16*)out, n));
  CHECK_LAUNCH(ctx, "narrow_f16");
  return 0;
}

int mhip_launch_unnest(mhip_ctx* ctx, int precision, const void* in, const void* coarse, void* out, int out_f32, int B,
                       int H, int W, int C, int nest) {
  if (nest < 0 || nest > 2 || C % 4 || (H & ((1 << nest) - 1)) || (W & ((1 << nest) - 1)) || (coarse && ((H | W) & 1)))
    return mhip_fail(ctx, MHIP_EINVAL, "unnest: bad shape %dx%d nest %d", H, W, nest);
  const long long total = (long long)B * H * W * (C / 4);
  dim3 grid(grid_for(total, 256)), block(256);
#define UN(T, OT) PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL((unnest_kernel<T, OT>), grid, block, 0, ctx->stream, (const T*)in, (const T*)coarse, (OT*)out, B, H, W, C, nest))
  if (precision == MHIP_PREC_F16) { if (out_f32) UN(_Float16, float); else UN(_Float16, _Float16); }
  else UN(float, float);
#undef UN
  CHECK_LAUNCH(ctx, "unnest");
  return 0;
}
