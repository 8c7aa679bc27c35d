// pil_resize.hip — Pillow's 8-bit Image.resize (LANCZOS / BILINEAR / BICUBIC, antialiased) for whole pages and crops, bit-exact.
//
// Replaces: detectron2 ResizeShortestEdge -> ResizeTransform.apply_image's PIL bilinear resize reached from
// OptimizedDetectronPredictor.invoke_model (marie/detectron/detector.py:103-105), and TrOCR's
// ``im.convert("RGB").resize((384, 384), BICUBIC)`` (marie/document/trocr_ocr_processor.py:116-118), and the document
// splitter's LayoutLMv3ImageProcessor(resample=Image.LANCZOS) (marie/components/document_splitter/transformers.py:111-113).
//
// libImaging/Resample.c: per output coordinate a window [xmin, xmin+n) of weights filter((x - center + 0.5) * ss),
// normalised in double and rounded to 22-bit fixed point; horizontal pass rounded to uint8, then vertical pass.
// A tiny kernel builds the two coefficient tables on the device (IEEE double, contraction off — the same arithmetic as
// the C code); the passes are pure integer MACs, 3 interleaved channels per thread.  LANCZOS takes its sin from the device
// library where Pillow takes it from the host libm: no rounded coefficient has been seen to move (DESIGN.md §3 pil_resize).
#include <algorithm>
#include <vector>

#include "pil_resample.h"   // the arithmetic, and #pragma clang fp contract(off) for everything below

namespace {

// ---- the three kernel bodies; the index type I is long long for a whole page, int for a batch of fragments ---------------
// one row of the tables: bounds = {xmin, n}, kk[x] = fixed-point weight of tap x (0 beyond n)
__device__ __forceinline__ void coeffs_row(int in_size, int out_size, int xx, int filter, int ksize, int* __restrict__ bounds,
                                           int* __restrict__ kk) {
  const PilWindow win = window(filter, in_size, out_size, xx);
  for (int x = 0; x < ksize; ++x) kk[x] = x < win.n ? fixed_weight(filter, win, x) : 0;
  bounds[0] = win.xmin;
  bounds[1] = win.n;
}

// horizontal: src [sh] rows of src_stride bytes, RGB -> tmp [sh][dw][3]
template <typename I>
__device__ __forceinline__ void hpass_body(const uint8_t* __restrict__ src, size_t src_stride, int sh, int dw, int ksize,
                                           const int* __restrict__ bounds, const int* __restrict__ kk, uint8_t* __restrict__ tmp) {
  const I total = (I)sh * dw;
  for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < total; i += (I)gridDim.x * 256) {
    const int yy = (int)(i / dw), xx = (int)(i - (I)yy * dw);
    const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
    const int* k = kk + (size_t)xx * ksize;
    const uint8_t* p = src + (size_t)yy * src_stride + (size_t)xmin * 3;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int x = 0; x < n; ++x) {
      const int w = k[x];
      a0 += (int)p[3 * x] * w; a1 += (int)p[3 * x + 1] * w; a2 += (int)p[3 * x + 2] * w;
    }
    uint8_t* o = tmp + (size_t)i * 3;
    o[0] = clip8(a0); o[1] = clip8(a1); o[2] = clip8(a2);
  }
}

// vertical: tmp [..][dw][3] -> dst [dh][dw][3]
template <typename I>
__device__ __forceinline__ void vpass_body(const uint8_t* __restrict__ tmp, int dw, int dh, int ksize, const int* __restrict__ bounds,
                                           const int* __restrict__ kk, uint8_t* __restrict__ dst) {
  const I total = (I)dh * dw;
  for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < total; i += (I)gridDim.x * 256) {
    const int yy = (int)(i / dw), xx = (int)(i - (I)yy * dw);
    const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
    const int* k = kk + (size_t)yy * ksize;
    const uint8_t* p = tmp + ((size_t)ymin * dw + xx) * 3;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int y = 0; y < n; ++y) {
      const int w = k[y];
      const uint8_t* q = p + (size_t)y * dw * 3;
      a0 += (int)q[0] * w; a1 += (int)q[1] * w; a2 += (int)q[2] * w;
    }
    uint8_t* o = dst + (size_t)i * 3;
    o[0] = clip8(a0); o[1] = clip8(a1); o[2] = clip8(a2);
  }
}

// ---- one image -----------------------------------------------------------------------------------------------------------
// bounds[2*xx] = xmin, bounds[2*xx+1] = n ; kk[xx*ksize + x] = fixed-point weight
__global__ void pil_coeffs_kernel(int in_size, int out_size, int filter, int ksize, int* __restrict__ bounds,
                                  int* __restrict__ kk) {
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx >= out_size) return;
  coeffs_row(in_size, out_size, xx, filter, ksize, bounds + 2 * xx, kk + (size_t)xx * ksize);
}

__global__ __launch_bounds__(256) void pil_hpass_kernel(const uint8_t* __restrict__ src, int sh, size_t src_stride, int dw,
                                                        int ksize, const int* __restrict__ bounds,
                                                        const int* __restrict__ kk, uint8_t* __restrict__ tmp) {
  hpass_body<long long>(src, src_stride, sh, dw, ksize, bounds, kk, tmp);
}

__global__ __launch_bounds__(256) void pil_vpass_kernel(const uint8_t* __restrict__ tmp, int dw, int dh, int ksize,
                                                        const int* __restrict__ bounds, const int* __restrict__ kk,
                                                        uint8_t* __restrict__ dst) {
  vpass_body<long long>(tmp, dw, dh, ksize, bounds, kk, dst);
}

// ---- batched variant: n fragments of different sizes -> n images of one size, one launch per pass -------------------
struct FragDev {
  unsigned long long src_off;   // byte offset of the fragment's first pixel
  unsigned long long tmp_off;   // byte offset of its [h][dw][3] intermediate
  int h, w, row_stride;
};

// coefficient tables of all fragments: axis 0 = x (in_size = w), axis 1 = y (in_size = h); kmax taps per output
__global__ void pil_coeffs_batch_kernel(const FragDev* __restrict__ fr, int axis, int out_size, int filter, int kmax,
                                        int* __restrict__ bounds, int* __restrict__ kk) {
  const int f = blockIdx.y, xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx >= out_size) return;
  const size_t row = (size_t)f * out_size + xx;
  coeffs_row(axis ? fr[f].h : fr[f].w, out_size, xx, filter, kmax, bounds + row * 2, kk + row * kmax);
}

__global__ __launch_bounds__(256) void pil_hpass_batch_kernel(const uint8_t* __restrict__ base, const FragDev* __restrict__ fr,
                                                              int dw, int kmax, const int* __restrict__ bounds,
                                                              const int* __restrict__ kk, uint8_t* __restrict__ tmp) {
  const FragDev d = fr[blockIdx.y];
  hpass_body<int>(base + d.src_off, d.row_stride, d.h, dw, kmax, bounds + (size_t)blockIdx.y * dw * 2,
                  kk + (size_t)blockIdx.y * dw * kmax, tmp + d.tmp_off);
}

__global__ __launch_bounds__(256) void pil_vpass_batch_kernel(const uint8_t* __restrict__ tmp, const FragDev* __restrict__ fr,
                                                              int dw, int dh, int kmax, const int* __restrict__ bounds,
                                                              const int* __restrict__ kk, uint8_t* __restrict__ dst) {
  const FragDev d = fr[blockIdx.y];
  vpass_body<int>(tmp + d.tmp_off, dw, dh, kmax, bounds + (size_t)blockIdx.y * dh * 2, kk + (size_t)blockIdx.y * dh * kmax,
                  dst + (size_t)blockIdx.y * (dh * dw) * 3);
}

// the coefficient tables and the intermediate image of n resizes (tmp_bytes of horizontal-pass output) in `c`
struct PilScratch {
  uint8_t* tmp;
  int *bx, *kx, *by, *ky;
};
void pil_carve(Carver& c, int n, size_t tmp_bytes, int dh, int dw, int kx, int ky, PilScratch* s) {
  s->tmp = c.take<uint8_t>(tmp_bytes);
  s->bx = c.take<int>((size_t)n * dw * 8);
  s->kx = c.take<int>((size_t)n * dw * kx * 4);
  s->by = c.take<int>((size_t)n * dh * 8);
  s->ky = c.take<int>((size_t)n * dh * ky * 4);
}

// the scratch of mhip_pil_resize_fragments: sized with a null base, placed on the caller's scratch otherwise
struct FragScratch {
  FragDev* fr;
  PilScratch p;
  int kx = 1, ky = 1;
};
void frag_carve(Carver& c, const mhip_crop_desc* descs, int n, int dh, int dw, int filter, FragScratch* s) {
  size_t tmp_total = 0;
  for (int i = 0; i < n; ++i) {
    tmp_total += ((size_t)std::max(descs[i].h, 1) * dw * 3 + 255) / 256 * 256;
    s->kx = std::max(s->kx, ksize_of(std::max(descs[i].w, 1), dw, filter));
    s->ky = std::max(s->ky, ksize_of(std::max(descs[i].h, 1), dh, filter));
  }
  s->fr = c.take<FragDev>(n * sizeof(FragDev));
  pil_carve(c, n, tmp_total, dh, dw, s->kx, s->ky, &s->p);
}

}  // namespace

bool mhip_pil_filter_ok(int filter) { return filter == MHIP_PIL_LANCZOS || filter == MHIP_PIL_BILINEAR || filter == MHIP_PIL_BICUBIC; }

size_t mhip_pil_resize_scratch_bytes(int sh, int sw, int dh, int dw, int filter) {
  PilScratch s;
  return mhip_layout_bytes([&](Carver& c) { pil_carve(c, 1, (size_t)sh * dw * 3, dh, dw, ksize_of(sw, dw, filter), ksize_of(sh, dh, filter), &s); });
}

// src: u8 RGB rows of `src_stride` bytes; dst [dh][dw][3]; scratch from mhip_pil_resize_scratch_bytes
int mhip_launch_pil_resize_rgb(mhip_ctx* ctx, const uint8_t* src, int sh, int sw, size_t src_stride, uint8_t* dst, int dh,
                               int dw, int filter, void* scratch) {
  if (sh < 1 || sw < 1 || dh < 1 || dw < 1 || !mhip_pil_filter_ok(filter))
    return mhip_fail(ctx, MHIP_EINVAL, "pil_resize: bad arguments");
  const int kx = ksize_of(sw, dw, filter), ky = ksize_of(sh, dh, filter);
  Carver c(scratch);
  PilScratch s;
  pil_carve(c, 1, (size_t)sh * dw * 3, dh, dw, kx, ky, &s);
  PROF_LAUNCH(ctx, MHIP_K_IMAGE_OPS, {
    hipLaunchKernelGGL(pil_coeffs_kernel, dim3((dw + 255) / 256), dim3(256), 0, ctx->stream, sw, dw, filter, kx, s.bx, s.kx);
    hipLaunchKernelGGL(pil_coeffs_kernel, dim3((dh + 255) / 256), dim3(256), 0, ctx->stream, sh, dh, filter, ky, s.by, s.ky);
    const long long t1 = (long long)sh * dw, t2 = (long long)dh * dw;
    hipLaunchKernelGGL(pil_hpass_kernel, dim3((unsigned)std::min<long long>((t1 + 255) / 256, 1 << 20)), dim3(256), 0, ctx->stream, src, sh, src_stride, dw, kx, s.bx, s.kx, s.tmp);
    hipLaunchKernelGGL(pil_vpass_kernel, dim3((unsigned)std::min<long long>((t2 + 255) / 256, 1 << 20)), dim3(256), 0, ctx->stream, s.tmp, dw, dh, ky, s.by, s.ky, dst);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mhip_fail(ctx, MHIP_EHIP, "pil_resize launch: %s", hipGetErrorString(e));
  return 0;
}

// n fragments (3-channel u8, descs on the host) -> dst [n][dh][dw][3], through the caller's scratch of scratch_bytes
// (mhip_pil_resize_fragments_scratch)
int mhip_pil_resize_fragments(mhip_ctx* ctx, const uint8_t* base_dev, const mhip_crop_desc* descs, int n, uint8_t* dst, int dh,
                              int dw, int filter, void* scratch, size_t scratch_bytes) {
  if (n < 1) return 0;
  if (!mhip_pil_filter_ok(filter)) return mhip_fail(ctx, MHIP_EINVAL, "pil_resize: unknown filter %d", filter);
  std::vector<FragDev> fr(n);
  size_t tmp_off = 0;
  int hmax = 1;
  for (int i = 0; i < n; ++i) {
    if (descs[i].channels != 3 || descs[i].h < 1 || descs[i].w < 1) return mhip_fail(ctx, MHIP_EINVAL, "pil_resize: fragment %d must be h x w x 3", i);
    fr[i].src_off = descs[i].src_offset; fr[i].tmp_off = tmp_off;
    fr[i].h = descs[i].h; fr[i].w = descs[i].w; fr[i].row_stride = descs[i].row_stride;
    tmp_off += ((size_t)descs[i].h * dw * 3 + 255) / 256 * 256;
    hmax = std::max(hmax, descs[i].h);
  }
  Carver c(scratch);
  FragScratch s;
  frag_carve(c, descs, n, dh, dw, filter, &s);
  if (c.off > scratch_bytes) return mhip_fail(ctx, MHIP_ENOMEM, "pil_resize: scratch %zu < %zu", scratch_bytes, c.off);
  const int kx = s.kx, ky = s.ky;
  // fr is a host temporary: through pinned staging, without draining the stream (the engine encodes page batches back to back;
  // a drain here left the GPU idle while the host prepared the next batch: ~12 ms per 8 pages)
  {
    const int rc = mhip_stage_h2d(ctx, s.fr, fr.data(), n * sizeof(FragDev));
    if (rc) return rc;
  }
  PROF_LAUNCH(ctx, MHIP_K_IMAGE_OPS, {
    hipLaunchKernelGGL(pil_coeffs_batch_kernel, dim3((dw + 255) / 256, n), dim3(256), 0, ctx->stream, s.fr, 0, dw, filter, kx, s.p.bx, s.p.kx);
    hipLaunchKernelGGL(pil_coeffs_batch_kernel, dim3((dh + 255) / 256, n), dim3(256), 0, ctx->stream, s.fr, 1, dh, filter, ky, s.p.by, s.p.ky);
    hipLaunchKernelGGL(pil_hpass_batch_kernel, dim3((hmax * dw + 255) / 256, n), dim3(256), 0, ctx->stream, base_dev, s.fr, dw, kx, s.p.bx, s.p.kx, s.p.tmp);
    hipLaunchKernelGGL(pil_vpass_batch_kernel, dim3((dh * dw + 255) / 256, n), dim3(256), 0, ctx->stream, s.p.tmp, s.fr, dw, dh, ky, s.p.by, s.p.ky, dst);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mhip_fail(ctx, MHIP_EHIP, "pil_resize_fragments launch: %s", hipGetErrorString(e));
  return 0;
}

size_t mhip_pil_resize_fragments_scratch(const mhip_crop_desc* descs, int n, int dh, int dw, int filter) {
  FragScratch s;
  return mhip_layout_bytes([&](Carver& c) { frag_carve(c, descs, n, dh, dw, filter, &s); });
}

// replaces: Image.fromarray(rgb).resize((dw, dh), LANCZOS | BILINEAR | BICUBIC) on host buffers (test / standalone entry)
extern "C" int mhip_pil_resize_rgb_host(mhip_ctx* ctx, const uint8_t* src_host, int sh, int sw, uint8_t* dst_host, int dh,
                                        int dw, int filter) {
  if (!ctx || !src_host || !dst_host) return MHIP_EINVAL;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t sb = (size_t)sh * sw * 3, db = (size_t)dh * dw * 3;
  uint8_t* s = nullptr;
  uint8_t* d = nullptr;
  void* scratch = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    s = ws.take<uint8_t>(sb);
    d = ws.take<uint8_t>(db);
    scratch = ws.take(mhip_pil_resize_scratch_bytes(sh, sw, dh, dw, filter));
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(s, src_host, sb, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_launch_pil_resize_rgb(ctx, s, sh, sw, (size_t)sw * 3, d, dh, dw, filter, scratch))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dst_host, d, db, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

// replaces: [Image.fromarray(f).resize((dw, dh), filter) for f in fragments] on host buffers, through the batched kernels
// (test / standalone entry): fragments inside base_host as descs say -> dst_host [n][dh][dw][3]
extern "C" int mhip_pil_resize_fragments_host(mhip_ctx* ctx, const uint8_t* base_host, size_t base_bytes, const mhip_crop_desc* descs,
                                              int n, int dh, int dw, int filter, uint8_t* dst_host) {
  if (!ctx || !base_host || !descs || !dst_host || n < 1 || dh < 1 || dw < 1) return MHIP_EINVAL;
  for (int i = 0; i < n; ++i) {
    const mhip_crop_desc& d = descs[i];
    if (d.channels != 3 || d.h < 1 || d.w < 1 || d.row_stride < 3 * d.w ||
        d.src_offset + (size_t)(d.h - 1) * d.row_stride + (size_t)3 * d.w > base_bytes)
      return mhip_fail(ctx, MHIP_EINVAL, "pil_resize: fragment %d is not h x w x 3 inside the %zu bytes of base", i, base_bytes);
  }
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t db = (size_t)n * dh * dw * 3, sb = mhip_pil_resize_fragments_scratch(descs, n, dh, dw, filter);
  uint8_t* base = nullptr;
  uint8_t* d = nullptr;
  void* scratch = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    base = ws.take<uint8_t>(base_bytes);
    d = ws.take<uint8_t>(db);
    scratch = ws.take(sb);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(base, base_host, base_bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_pil_resize_fragments(ctx, base, descs, n, d, dh, dw, filter, scratch, sb))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(dst_host, d, db, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}
