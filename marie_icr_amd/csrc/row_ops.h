// row_ops.h — what the one-wave-per-row kernels of the ViT, CLIP, BERT and LayoutReader towers do with a row: load it into
// registers, LayerNorm it there, store it.  Used by the row LayerNorm kernel itself (row_ops.hip: the stand-alone LayerNorm of
// those towers) and by the embedding / head fronts of clip_ops.hip, cliptext_ops.hip, berttext_ops.hip and layoutreader_ops.hip.
// (trocr_ops.hip and layoutlmv3_ops.hip keep their own copies: their variance rounds differently)
// D % 64 == 0, D <= 1024, a lane holds the float4 groups at columns (i * 64 + lane) * 4 < D.
#pragma once
#include "igemm_common.h"

// The loads build a group in a local and assign v[i] once: written as "v[i] = 0; if (c < D) v[i] = load" inside a helper, the
// compiler kept every group of x, g and b in flight (77 .. 102 VGPRs, 4 .. 6 waves per SIMD); this form compiles to 30 .. 66.
//
// internal linkage: a file that includes this keeps its own helpers of the same names apart from another file's
constexpr int ROW_GROUPS = 4;      // float4 groups per lane: D <= 1024
static inline bool row_width_ok(int D) { return D >= 64 && D % 64 == 0 && D <= 256 * ROW_GROUPS; }

static __device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// v <- the fp32 row; groups at columns >= D are zeros
static __device__ __forceinline__ void row_load(float4v v[ROW_GROUPS], const float* row, int D, int lane) {
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    float4v t = {0.f, 0.f, 0.f, 0.f};
    if (c < D) t = *(const float4v*)(row + c);
    v[i] = t;
  }
}
// the same from an f16 row, hi + lo with the low plane of a split stream (lo null: hi alone)
static __device__ __forceinline__ void row_load(float4v v[ROW_GROUPS], const _Float16* row, const _Float16* lo, int D, int lane) {
  typedef _Float16 half4 __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    float4v t = {0.f, 0.f, 0.f, 0.f};
    if (c < D) {
      const half4 h = *(const half4*)(row + c);
      t = (float4v){(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
      if (lo) {
        const half4 l = *(const half4*)(lo + c);
        t += (float4v){(float)l[0], (float)l[1], (float)l[2], (float)l[3]};
      }
    }
    v[i] = t;
  }
}
// v += the fp32 row (one term of an embedding sum: the caller's order of calls is the order of the additions)
static __device__ __forceinline__ void row_add(float4v v[ROW_GROUPS], const float* row, int D, int lane) {
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    float4v t = v[i];
    if (c < D) t += *(const float4v*)(row + c);
    v[i] = t;
  }
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

// the row -> the fp32 stream (h_row) and / or its copy in the element type of the next GEMM's operand (ht_row); either may be null
template <typename T>
static __device__ __forceinline__ void row_store(const float4v v[ROW_GROUPS], float* h_row, T* ht_row, int D, int lane) {
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) {
      if (h_row) *(float4v*)(h_row + c) = v[i];
      if (ht_row) {
        T o4[4] = {(T)v[i][0], (T)v[i][1], (T)v[i][2], (T)v[i][3]};
        if (sizeof(T) == 2) *(uint64_t*)(ht_row + c) = *(uint64_t*)o4;
        else *(float4v*)(ht_row + c) = *(float4v*)o4;
      }
    }
  }
}
