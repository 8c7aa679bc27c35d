// row_ops.h — what the one-wave-per-row kernels share (clip_ops.hip, cliptext_ops.hip, berttext_ops.hip, layoutreader_ops.hip):
// D % 64 == 0, D <= 1024, a lane holds the float4 groups at columns (i * 64 + lane) * 4 < D.
#pragma once
#include "igemm_common.h"

// internal linkage: a file that includes this keeps its own helpers of the same names apart from another file's
constexpr int ROW_GROUPS = 4;      // float4 groups per lane: D <= 1024
static inline bool row_width_ok(int D) { return D >= 64 && D % 64 == 0 && D <= 256 * ROW_GROUPS; }

static __device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// LayerNorm of the row a wave holds, two-pass in registers; groups at columns >= D are not touched
static __device__ __forceinline__ void row_layernorm(float4v v[ROW_GROUPS], int D, int lane, const float* __restrict__ g,
                                              const float* __restrict__ b, float eps) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i)
    if ((i * 64 + lane) * 4 < D) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i)
    if ((i * 64 + lane) * 4 < D)
#pragma unroll
      for (int k = 0; k < 4; ++k) { const float d = v[i][k] - mean; q += d * d; }
  const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) {
      const float4v gg = *(const float4v*)(g + c), bb = *(const float4v*)(b + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[i][k] = (v[i][k] - mean) * rstd * gg[k] + bb[k];
    }
  }
}
