// cliprn_ops.hip — the pieces of CLIP's ModifiedResNet tower (RN50 / RN101 / RN50x4) the other paths do not have: the stem's
// first convolution on uint8 clips, the 2 x 2 average pool, and the attention pool (token build, one-query attention, c_proj).
//
// Replaces, in clip/model.py: ModifiedResNet.conv1 + bn1 + relu1 with the Normalize of clip._transform in front, every
// nn.AvgPool2d (the stem's, Bottleneck.avgpool, the one in Bottleneck.downsample), and AttentionPool2d.forward.
// (Every other convolution, and the q and k | v projections of the attention pool, are conv_igemm.hip.)
//
// Activations are NHWC in the mode's element type T with the channel count rounded up to what conv_igemm takes (64 f16 /
// 32 f32 channels); the padding channels are zeros, and every kernel here keeps them zeros.
//
// Profile slots (the kernel table is not extended): the stem counts under conv_first, the pool under image_ops, the token
// build under clipvis_embed, the one-query attention under dec_ops, c_proj under clipvis_head.
#include "igemm_common.h"
#include "row_ops.h"

namespace {

template <typename T>
__device__ __forceinline__ void store8(T* dst, const float f[8]) {
  T v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (T)f[j];
  if (sizeof(T) == 2) *(uint4v*)dst = *(uint4v*)v;
  else { *(uint4v*)dst = *(uint4v*)v; *(uint4v*)(dst + 4) = *(uint4v*)(v + 4); }
}

// ------------------------------------------------------------------------------------------------------- stem
// clips u8 [B][S][S][3] (channel order as stored; `swap_rb`: stored channel 2 - c is model channel c) -> out [B][S/2][S/2][Cp] T
//   out[oy][ox][n] = relu(scale[n] * sum_{dy,dx,c} x[2 oy - 1 + dy][2 ox - 1 + dx][c] * w[(dy * 3 + dx) * 3 + c][n] + bias[n])
// with x = (pixel / 255 - mean[c]) / std[c] inside the clip and 0 outside it (the padding applies to the normalised tensor).
// K = 27: a direct kernel, a thread per (output pixel, 8 channels); the 27 x Cp weights and the epilogue vectors sit in LDS.
struct ChannelNorm { float mean[3], stdv[3]; };
constexpr int STEM_MAX_C = 64;

template <typename T>
__global__ __launch_bounds__(256) void cliprn_stem_kernel(const uint8_t* __restrict__ imgs, int S, int swap_rb, ChannelNorm nrm,
                                                          const float* __restrict__ w, const float* __restrict__ scale,
                                                          const float* __restrict__ bias, T* __restrict__ out, int Cp,
                                                          long long total) {
  __shared__ __attribute__((aligned(16))) float sw[29 * STEM_MAX_C];
  for (int i = threadIdx.x; i < 27 * Cp; i += 256) sw[i] = w[i];
  for (int i = threadIdx.x; i < Cp; i += 256) { sw[27 * Cp + i] = scale[i]; sw[28 * Cp + i] = bias[i]; }
  __syncthreads();
  const int So = S / 2, chunks = Cp / 8;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int chunk = (int)(e % chunks);
    const long long pix = e / chunks;
    const int ox = (int)(pix % So), oy = (int)((pix / So) % So);
    const uint8_t* img = imgs + (size_t)(pix / ((long long)So * So)) * S * S * 3;
    float x[27];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int iy = 2 * oy - 1 + dy, ix = 2 * ox - 1 + dx;
        const bool in = iy >= 0 && iy < S && ix >= 0 && ix < S;
        const uint8_t* src = img + ((size_t)(in ? iy : 0) * S + (in ? ix : 0)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v = ((float)src[swap_rb ? 2 - c : c] / 255.f - nrm.mean[c]) / nrm.stdv[c];
          x[(dy * 3 + dx) * 3 + c] = in ? v : 0.f;
        }
      }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* wc = sw + chunk * 8;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      const float4v w0 = *(const float4v*)(wc + k * Cp), w1 = *(const float4v*)(wc + k * Cp + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { acc[j] = __builtin_fmaf(x[k], w0[j], acc[j]); acc[4 + j] = __builtin_fmaf(x[k], w1[j], acc[4 + j]); }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaxf(__builtin_fmaf(acc[j], sw[27 * Cp + chunk * 8 + j], sw[28 * Cp + chunk * 8 + j]), 0.f);
    store8(out + (size_t)pix * Cp + chunk * 8, acc);
  }
}

// ------------------------------------------------------------------------------------------------------- average pool
// in [B][H][W][C] T -> out [B][H/2][W/2][C] T: the mean of every 2 x 2 window, summed in fp32; 16 bytes of channels a lane
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_nhwc_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W, int C,
                                                            long long total) {
  constexpr int V = 16 / sizeof(T);
  const int cv = C / V, Ho = H / 2, Wo = W / 2;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int c = (int)(e % cv) * V;
    const long long pix = e / cv;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
    const long long b = pix / ((long long)Wo * Ho);
    const T* src = in + (((size_t)b * H + 2 * oy) * W + 2 * ox) * C + c;
    const uint4v r00 = *(const uint4v*)src, r01 = *(const uint4v*)(src + C);
    const uint4v r10 = *(const uint4v*)(src + (size_t)W * C), r11 = *(const uint4v*)(src + (size_t)W * C + C);
    const T *a = (const T*)&r00, *bb = (const T*)&r01, *cc = (const T*)&r10, *d = (const T*)&r11;
    uint4v raw;
    T* o = (T*)&raw;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = (T)((((float)a[j] + (float)bb[j]) + ((float)cc[j] + (float)d[j])) * 0.25f);
    *(uint4v*)(out + (size_t)pix * C + c) = raw;
  }
}

// ------------------------------------------------------------------------------------------------------- attention pool
// 1. tokens.  x [B][HW][E] T (the last map) -> tok [B][HW + 1][E] T: row 0 = mean over the HW rows + pos[0], row t = x[t - 1] +
// pos[t]; xq [B][E] T = row 0 again, the operand of the q projection.  Sums and the position add are fp32.  A thread owns
// 16 bytes of channels of one clip and walks its rows in order.
template <typename T>
__global__ __launch_bounds__(256) void cliprn_tokens_kernel(const T* __restrict__ x, const float* __restrict__ pos, T* __restrict__ tok,
                                                            T* __restrict__ xq, int HW, int E) {
  constexpr int V = 16 / sizeof(T);
  const int c = (blockIdx.x * 256 + threadIdx.x) * V;
  if (c >= E) return;
  const size_t b = blockIdx.y;
  const T* xs = x + b * HW * E + c;
  T* ts = tok + b * (HW + 1) * E + c;
  float sum[V];
#pragma unroll
  for (int j = 0; j < V; ++j) sum[j] = 0.f;
  for (int t = 0; t < HW; ++t) {
    const uint4v raw = *(const uint4v*)(xs + (size_t)t * E);
    const T* v = (const T*)&raw;
    const float* p = pos + (size_t)(t + 1) * E + c;
    uint4v oraw;
    T* o = (T*)&oraw;
#pragma unroll
    for (int j = 0; j < V; ++j) { sum[j] += (float)v[j]; o[j] = (T)((float)v[j] + p[j]); }
    *(uint4v*)(ts + (size_t)(t + 1) * E) = oraw;
  }
  uint4v oraw;
  T* o = (T*)&oraw;
#pragma unroll
  for (int j = 0; j < V; ++j) o[j] = (T)(sum[j] / (float)HW + pos[c + j]);
  *(uint4v*)ts = oraw;
  *(uint4v*)(xq + b * E + c) = oraw;
}

// 2. one query per (clip, head).  q fp32 [B][E] (pre-scaled by 64^-0.5), kv fp32 [B * NT][2 E] (k | v), head h at columns
// h * 64 -> ao fp32 [B][E].  A wave takes every fourth key: lanes along the head's 64 columns, the score by a wave sum.  Scores
// and soft-max are fp32; the scores, then the probabilities, of the NT <= 257 keys sit in LDS.  Every k and v row of the head
// is read once, so the rows themselves are not staged.
constexpr int ATTNPOOL_MAX_KEYS = 257;

__global__ __launch_bounds__(256) void cliprn_attn1q_kernel(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ ao,
                                                            int NT, int E) {
  __shared__ float sc[ATTNPOOL_MAX_KEYS + 3];
  __shared__ float part[4][64];
  const int h = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t b = blockIdx.y;
  const float* rows = kv + b * NT * 2 * E + (size_t)h * 64 + lane;
  const float qv = q[b * E + h * 64 + lane];
  for (int t = wave; t < NT; t += 4) {
    const float s = wave_sum(qv * rows[(size_t)t * 2 * E]);
    if (lane == 0) sc[t] = s;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int t = lane; t < NT; t += 64) m = fmaxf(m, sc[t]);
#pragma unroll
  for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __syncthreads();                                   // every wave has its maximum before the scores are overwritten
  for (int t = threadIdx.x; t < NT; t += 256) sc[t] = expf(sc[t] - m);
  __syncthreads();
  float z = 0.f;
  for (int t = lane; t < NT; t += 64) z += sc[t];
  z = wave_sum(z);
  float acc = 0.f;
  for (int t = wave; t < NT; t += 4) acc = __builtin_fmaf(sc[t], rows[(size_t)t * 2 * E + E], acc);
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0) ao[b * E + h * 64 + lane] = ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) / z;
}

// 3. c_proj.  emb[b][j] = sum_k ao[b][k] w[j][k] + bias[j]; w [P][E] fp32 as the checkpoint holds it.  A wave per output, lanes
// along k; a workgroup takes CPROJ_COLS outputs of one clip with that clip's row in LDS.
constexpr int CPROJ_COLS = 32, CPROJ_MAX_E = 4096;

__global__ __launch_bounds__(256) void cliprn_cproj_kernel(const float* __restrict__ ao, int E, const float* __restrict__ w,
                                                           const float* __restrict__ bias, int P, float* __restrict__ emb) {
  __shared__ __attribute__((aligned(16))) float ys[CPROJ_MAX_E];
  const int img = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = threadIdx.x * 4; k < E; k += 1024) *(float4v*)(ys + k) = *(const float4v*)(ao + (size_t)img * E + k);
  __syncthreads();
  const int j0 = blockIdx.y * CPROJ_COLS, j1 = min(j0 + CPROJ_COLS, P);
  for (int j = j0 + wave; j < j1; j += 4) {
    const float* wr = w + (size_t)j * E;
    float acc = 0.f;
    for (int k = lane * 4; k < E; k += 256) {
      const float4v ww = *(const float4v*)(wr + k), yy = *(const float4v*)(ys + k);
      acc += (ww[0] * yy[0] + ww[1] * yy[1]) + (ww[2] * yy[2] + ww[3] * yy[3]);
    }
    acc = wave_sum(acc);
    if (lane == 0) emb[(size_t)img * P + j] = acc + bias[j];
  }
}

}  // namespace

int mhip_launch_cliprn_stem(mhip_ctx* ctx, int precision, const uint8_t* imgs, int B, int S, int swap_rb, const float mean[3],
                            const float stdv[3], const float* w27, const float* scale, const float* bias, void* out, int Cp) {
  if (B <= 0 || S < 2 || S % 2 || S > 4096 || Cp < 8 || Cp % 8 || Cp > STEM_MAX_C)
    return mhip_fail(ctx, MHIP_EINVAL, "cliprn_stem: B=%d S=%d (even) channels=%d (a multiple of 8 up to %d)", B, S, Cp, STEM_MAX_C);
  ChannelNorm n;
  for (int c = 0; c < 3; ++c) { n.mean[c] = mean[c]; n.stdv[c] = stdv[c]; }
  const long long total = (long long)B * (S / 2) * (S / 2) * (Cp / 8);
  dim3 grid(grid_for(total, 256)), block(256);
  if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_CONV_FIRST, hipLaunchKernelGGL(cliprn_stem_kernel<_Float16>, grid, block, 0, ctx->stream, imgs, S, swap_rb, n, w27, scale, bias, (_Float16*)out, Cp, total));
  else
    PROF_LAUNCH(ctx, MHIP_K_CONV_FIRST, hipLaunchKernelGGL(cliprn_stem_kernel<float>, grid, block, 0, ctx->stream, imgs, S, swap_rb, n, w27, scale, bias, (float*)out, Cp, total));
  CHECK_LAUNCH(ctx, "cliprn_stem");
  return 0;
}

int mhip_launch_avgpool_nhwc(mhip_ctx* ctx, int precision, int k, const void* in, void* out, int B, int H, int W, int C) {
  const int V = precision == MHIP_PREC_F16 ? 8 : 4;
  if (k != 2) return mhip_fail(ctx, MHIP_EINVAL, "avgpool_nhwc: k=%d (2 x 2 windows are built)", k);
  if (B <= 0 || H < k || W < k || H % k || W % k) return mhip_fail(ctx, MHIP_EINVAL, "avgpool_nhwc: B=%d map %d x %d is no multiple of the %d x %d window", B, H, W, k, k);
  if (C < V || C % V || (((uintptr_t)in | (uintptr_t)out) & 15)) return mhip_fail(ctx, MHIP_EINVAL, "avgpool_nhwc: C=%d must be a multiple of %d on 16-byte boundaries", C, V);
  const long long total = (long long)B * (H / 2) * (W / 2) * (C / V);
  dim3 grid(grid_for(total, 256)), block(256);
  if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_IMAGE_OPS, hipLaunchKernelGGL(avgpool2_nhwc_kernel<_Float16>, grid, block, 0, ctx->stream, (const _Float16*)in, (_Float16*)out, H, W, C, total));
  else
    PROF_LAUNCH(ctx, MHIP_K_IMAGE_OPS, hipLaunchKernelGGL(avgpool2_nhwc_kernel<float>, grid, block, 0, ctx->stream, (const float*)in, (float*)out, H, W, C, total));
  CHECK_LAUNCH(ctx, "avgpool_nhwc");
  return 0;
}

bool mhip_cliprn_attnpool_ok(int HW, int E, int P) {
  return HW >= 1 && HW + 1 <= ATTNPOOL_MAX_KEYS && E >= 64 && E % 64 == 0 && E <= CPROJ_MAX_E && P >= 1 && P <= 65535 * CPROJ_COLS;
}

int mhip_launch_cliprn_tokens(mhip_ctx* ctx, int precision, const void* x, const float* pos, void* tok, void* xq, int B, int HW, int E) {
  if (B <= 0 || B > 65535 || !mhip_cliprn_attnpool_ok(HW, E, 1)) return mhip_fail(ctx, MHIP_EINVAL, "cliprn_tokens: B=%d HW=%d E=%d", B, HW, E);
  const int V = precision == MHIP_PREC_F16 ? 8 : 4;
  dim3 grid((E / V + 255) / 256, B), block(256);
  if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_CLIPVIS_EMBED, hipLaunchKernelGGL(cliprn_tokens_kernel<_Float16>, grid, block, 0, ctx->stream, (const _Float16*)x, pos, (_Float16*)tok, (_Float16*)xq, HW, E));
  else
    PROF_LAUNCH(ctx, MHIP_K_CLIPVIS_EMBED, hipLaunchKernelGGL(cliprn_tokens_kernel<float>, grid, block, 0, ctx->stream, (const float*)x, pos, (float*)tok, (float*)xq, HW, E));
  CHECK_LAUNCH(ctx, "cliprn_tokens");
  return 0;
}

int mhip_launch_cliprn_attn1q(mhip_ctx* ctx, const float* q, const float* kv, float* ao, int B, int NT, int E) {
  if (B <= 0 || B > 65535 || !mhip_cliprn_attnpool_ok(NT - 1, E, 1)) return mhip_fail(ctx, MHIP_EINVAL, "cliprn_attn1q: B=%d keys=%d E=%d", B, NT, E);
  PROF_LAUNCH(ctx, MHIP_K_DEC_OPS, hipLaunchKernelGGL(cliprn_attn1q_kernel, dim3(E / 64, B), dim3(256), 0, ctx->stream, q, kv, ao, NT, E));
  CHECK_LAUNCH(ctx, "cliprn_attn1q");
  return 0;
}

int mhip_launch_cliprn_cproj(mhip_ctx* ctx, const float* ao, int B, int E, const float* w, const float* bias, int P, float* emb) {
  if (B <= 0 || !mhip_cliprn_attnpool_ok(1, E, P)) return mhip_fail(ctx, MHIP_EINVAL, "cliprn_cproj: B=%d E=%d P=%d", B, E, P);
  PROF_LAUNCH(ctx, MHIP_K_CLIPVIS_HEAD, hipLaunchKernelGGL(cliprn_cproj_kernel, dim3(B, (P + CPROJ_COLS - 1) / CPROJ_COLS), dim3(256), 0, ctx->stream, ao, E, w, bias, P, emb));
  CHECK_LAUNCH(ctx, "cliprn_cproj");
  return 0;
}
