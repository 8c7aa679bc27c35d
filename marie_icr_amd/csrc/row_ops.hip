// row_ops.hip — the stand-alone row LayerNorm of the towers: the pre-LayerNorms of the ViT, DiT and TrOCR encoders (fp32, f16 or
// split f16 stream in, GEMM operand out), the post-LayerNorms of BERT and LayoutReader (fp32 stream and GEMM operand out), and the
// LayerNorms of the CLIP towers (GEMM operand out).  One kernel, one launcher; the arithmetic is row_ops.h's.  (The TrOCR decoder
// and LayoutLMv3 keep layernorm2 of trocr_ops.hip: DESIGN.md §3, "The row kernels of the towers".)
//
// Replaces the nn.LayerNorm of: Block (marie/boxes/dit/ditod/beit.py:293,305), BertSelfOutput / BertOutput, CLIPEncoderLayer.
#include "row_ops.h"
#include "stage_host.h"

namespace {

// h = LN(x) (null: not written), ht its copy in the GEMM element type (null: not written); one wave per row.  x is fp32, or f16
// with an optional low plane (x = hi + lo).  h may be x: a wave holds its whole row in registers before it writes any of it and no
// other wave touches that row — which is why x and h carry no __restrict__.
template <typename T, typename XT>
__global__ __launch_bounds__(256) void row_layernorm_kernel(const XT* x, const _Float16* __restrict__ xlo, const float* __restrict__ g,
                                                            const float* __restrict__ b, float* h, T* __restrict__ ht, int rows, int D,
                                                            float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const size_t o = (size_t)row * D;
  float4v v[ROW_GROUPS];
  if constexpr (sizeof(XT) == 4) row_load(v, x + o, D, lane);
  else row_load(v, x + o, xlo ? xlo + o : nullptr, D, lane);
  row_layernorm(v, D, lane, g, b, eps);
  row_store<T>(v, h ? h + o : nullptr, ht ? ht + o : nullptr, D, lane);
}

}  // namespace

int mhip_launch_row_layernorm(mhip_ctx* ctx, int slot, int precision, const void* x, int x_f16, const void* x_lo, const float* g,
                              const float* b, float* h, void* ht, int rows, int D, float eps) {
  if (rows <= 0 || !row_width_ok(D)) return mhip_fail(ctx, MHIP_EINVAL, "row_layernorm: D=%d rows=%d", D, rows);
  if (!h && !ht) return mhip_fail(ctx, MHIP_EINVAL, "row_layernorm: neither output given");
  if (x_f16 && precision != MHIP_PREC_F16) return mhip_fail(ctx, MHIP_EINVAL, "row_layernorm: an f16 stream needs the f16 mode");
  if (x_lo && !x_f16) return mhip_fail(ctx, MHIP_EINVAL, "row_layernorm: a low plane belongs to an f16 high plane");
  dim3 grid((rows + 3) / 4), block(256);
  if (x_f16)
    PROF_LAUNCH(ctx, slot, hipLaunchKernelGGL((row_layernorm_kernel<_Float16, _Float16>), grid, block, 0, ctx->stream, (const _Float16*)x, (const _Float16*)x_lo, g, b, h, (_Float16*)ht, rows, D, eps));
  else if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, slot, hipLaunchKernelGGL((row_layernorm_kernel<_Float16, float>), grid, block, 0, ctx->stream, (const float*)x, (const _Float16*)nullptr, g, b, h, (_Float16*)ht, rows, D, eps));
  else
    PROF_LAUNCH(ctx, slot, hipLaunchKernelGGL((row_layernorm_kernel<float, float>), grid, block, 0, ctx->stream, (const float*)x, (const _Float16*)nullptr, g, b, h, (float*)ht, rows, D, eps));
  CHECK_LAUNCH(ctx, "row_layernorm");
  return 0;
}

// ------------------------------------------------------------------ stage entry (see include/marie_hip.h)
extern "C" int mhip_row_layernorm_host(mhip_ctx* ctx, int precision, const float* x, int x_f16, const float* x_lo, const float* g,
                                       const float* b, int rows, int D, float eps, int in_place, float* h, float* ht) {
  if (!ctx || !x || !g || !b || (!h && !ht)) return MHIP_EINVAL;
  if (int rc = mhip_stage_precision(ctx, precision)) return rc;
  if (rows < 1 || D < 1 || (in_place && (!h || x_f16))) return mhip_fail(ctx, MHIP_EINVAL, "row_layernorm_host: bad shape");
  const size_t n = (size_t)rows * D;
  StageIO io(ctx, precision);
  // in place: one guarded device buffer, x up and h back
  const int i_x = in_place ? io.add(x, h, n, 4, false) : (x_f16 ? io.in_act(x, n) : io.in_raw(x, n, 4));
  const int i_lo = x_lo ? io.in_act(x_lo, n) : -1;
  const int i_g = io.in_raw(g, D, 4), i_b = io.in_raw(b, D, 4);
  const int i_h = in_place ? i_x : (h ? io.out_raw(h, n, 4) : -1), i_t = ht ? io.out_act(ht, n) : -1;
  // test surface: the launch is counted in vit_ops whatever tower the test stands for
  return io.run([&] {
    return mhip_launch_row_layernorm(ctx, MHIP_K_VIT_OPS, precision, io.dev(i_x), x_f16, i_lo < 0 ? nullptr : io.dev(i_lo),
                                     io.dev<float>(i_g), io.dev<float>(i_b), i_h < 0 ? nullptr : io.dev<float>(i_h),
                                     i_t < 0 ? nullptr : io.dev(i_t), rows, D, eps);
  });
}
