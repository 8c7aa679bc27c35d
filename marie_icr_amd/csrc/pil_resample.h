// pil_resample.h — the arithmetic of Pillow's 8-bit Image.resize (libImaging/Resample.c: precompute_coeffs and the rounding of
// the two integer passes), written once.  pil_resize.hip builds coefficient tables from it (single-image and batched kernels),
// crop_batch.hip rebuilds the weights per thread.  IEEE double, in the order of the C code, FMA contraction off: the pragma
// below holds for the rest of the including file, so include this where the first kernel may rely on it.
#pragma once
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

constexpr int PRECISION_BITS = 32 - 8 - 2;

// the filter supports of Resample.c: lanczos 3, bilinear 1, bicubic 2
__host__ __device__ __forceinline__ double support_of(int filter) {
  return filter == MHIP_PIL_LANCZOS ? 3.0 : (filter == MHIP_PIL_BILINEAR ? 1.0 : 2.0);
}

// sinc_filter of Resample.c
__device__ __forceinline__ double sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}

// bilinear_filter, lanczos_filter (the truncated sinc) and bicubic_filter (a = -0.5); a constant `filter` leaves one of them
__device__ __forceinline__ double filt(int filter, double x) {
  if (x < 0.0) x = -x;
  if (filter == MHIP_PIL_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  if (filter == MHIP_PIL_LANCZOS) return x < 3.0 ? sinc(x) * sinc(x / 3) : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// window [xmin, xmin + n) and normaliser ww of output sample xx (precompute_coeffs)
struct PilWindow {
  int xmin, n;
  double center, ss, ww;
};
__device__ __forceinline__ PilWindow window(int filter, int in_size, int out_size, int xx) {
  const double scale = (double)in_size / (double)out_size;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = support_of(filter) * filterscale;
  const double center = ((double)xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += filt(filter, ((double)(x + xmin) - center + 0.5) * ss);
  return {xmin, xmax, center, ss, ww};
}

// tap x of the window as 22-bit fixed point
__device__ __forceinline__ int fixed_weight(int filter, const PilWindow& win, int x) {
  double w = filt(filter, ((double)(x + win.xmin) - win.center + 0.5) * win.ss);
  if (win.ww != 0.0) w /= win.ww;
  return w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
}

// an accumulator that started at 1 << (PRECISION_BITS - 1) -> uint8
__device__ __forceinline__ uint8_t clip8(int v) {
  v >>= PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// taps per output coordinate of the coefficient tables (host)
inline int ksize_of(int in_size, int out_size, int filter) {
  double scale = (double)in_size / (double)out_size;
  if (scale < 1.0) scale = 1.0;
  const double support = support_of(filter) * scale;
  return (int)ceil(support) * 2 + 1;
}
