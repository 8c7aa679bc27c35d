// berttext_ops.hip — the kernels of the BERT sentence encoders (berttext_api.hip) the other towers do not have: bidirectional
// soft-max attention over sequences of different lengths (attn_short: up to 128 rows, keys held in LDS; attn_long: up to 8192
// rows, keys streamed in blocks of 128 under an online soft-max), the embedding + LayerNorm front, the post-LayerNorm of a layer
// at widths that are no multiple of 256, GEGLU and masked pooling.
//
// Replaces, in transformers/models/bert/modeling_bert.py: BertEmbeddings.forward, the attention of BertSelfAttention under the
// padding mask, the LayerNorms of BertSelfOutput / BertOutput; of JinaBERT the symmetric ALiBi bias and the gated MLP's
// activation; and the Pooling (mean / cls) and Normalize modules of sentence_transformers.
//
// attn_short: one workgroup = one (sequence, head), as attn_causal (cliptext_ops.hip): K and V^T of the head are staged in LDS
// once, each wave owns the 16-query tiles wave, wave + 4, the products are taken transposed (S^T = K Q^T, O^T = V^T P^T) so that
// the score registers are the B operand of the second product with no lane movement, and the whole score row stays in registers
// (at most 8 tiles x 4): the mask is applied before the row maximum and no online rescaling is needed.  What differs:
//   * a sequence has len[b] keys (1 <= len <= npad).  A query tile walks the key tiles 0 .. ceil(len / 16) - 1 in that order — a
//     function of len alone, never of npad or of the batch — keys >= len are staged as zeros and their scores are set to -inf by
//     select, so a sequence's rows do not depend on what it is batched with, bit for bit.  Query rows >= len are computed like
//     any other row: finite, and nobody reads them;
//   * with slopes, the score of (query i, key j) gets  - slope[head] * |i - j|  (ALiBi, symmetric), in the log2 units q carries
//     (q arrives scaled by head_dim^-0.5 * log2(e)); without slopes there is no bias term;
//   * the head dim HD is 64 or 32: at 32 the first product is one 16x16x32 f16 step and O^T has two 16-row tiles.
//   f16: v_mfma_f32_16x16x32_f16 for both products (two key tiles make one 32-key step of the second; a tile past the last enters
//        as zeros), probabilities rounded to f16 only as that operand; the row sum is of the fp32 probabilities.
//   f32: v_mfma_f32_16x16x4_f32, an fp32 fma chain: no f16 value anywhere.
#include <algorithm>

#include "igemm_common.h"
#include "row_ops.h"

using namespace igemm;

namespace {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));

constexpr int AS_MAXK = 128;      // keys of a sequence
constexpr int AS_THREADS = 256;

// LDS images of K [key][d] and V^T [d][key].  f16: padded rows; f32: 16-byte chunks XOR-swizzled by the row, unpadded, so that
// both images fit in 64 KiB at HD 64
template <typename T, int HD>
struct AsLay;
template <int HD>
struct AsLay<_Float16, HD> {
  static constexpr int KP = HD + 8, VP = AS_MAXK + 8;
  static constexpr int KSZ = AS_MAXK * KP, VSZ = HD * VP;
  static __device__ __forceinline__ int k(int key, int d) { return key * KP + d; }
  static __device__ __forceinline__ int v(int d, int key) { return d * VP + key; }
};
template <int HD>
struct AsLay<float, HD> {
  static constexpr int KSZ = AS_MAXK * HD, VSZ = HD * AS_MAXK;
  // d, key: multiples of 4
  static __device__ __forceinline__ int k(int key, int d) { return key * HD + ((((d >> 2) ^ key) & (HD / 4 - 1)) << 2); }
  static __device__ __forceinline__ int v(int d, int key) { return d * AS_MAXK + (((key >> 2) ^ (d & 15)) << 2); }
};

template <typename T>
struct ShortArgs {
  const T* q;      // [seqs * npad][ldq], head h at column h * HD, in head_dim^-0.5 * log2(e) units
  const T* k;      // [seqs * npad][ldk]
  const T* vt;     // [heads * HD][ldv], column = seq * npad + key
  T* out;          // [seqs * npad][ldo]
  const int* len;        // [seqs]
  const float* slope;    // [heads] in log2 units, or null
  int ldq, ldk, ldv, ldo;
  int npad, heads;
};

template <typename T>
__device__ __forceinline__ typename Tr<T>::chunk_t zero_chunk() {
  typename Tr<T>::chunk_t z;
#pragma unroll
  for (int j = 0; j < Tr<T>::E; ++j) z[j] = (T)0.f;
  return z;
}

template <typename T, int HD>
__global__ __launch_bounds__(AS_THREADS) void attn_short_kernel(ShortArgs<T> p) {
  typedef Tr<T> X;
  typedef typename X::chunk_t chunk_t;
  typedef AsLay<T, HD> L;
  constexpr int E = X::E;                 // elements of a 16-byte chunk
  constexpr int NKS = HD / (4 * E);       // MFMA steps over the head dim
  constexpr int NDT = HD / 16;            // 16-row tiles of O^T
  __shared__ __attribute__((aligned(16))) T Ks[L::KSZ];
  __shared__ __attribute__((aligned(16))) T Vs[L::VSZ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const int head = blockIdx.x % p.heads, seq = blockIdx.x / p.heads;
  const int npad = p.npad;
  const size_t row0 = (size_t)seq * npad;
  // the host entries have checked the lengths; the clamp keeps a stray value inside the LDS images
  const int len = min(max(p.len[seq], 1), npad);
  const int nkt = (len + 15) >> 4;        // key tiles of this sequence
  const int kp = ((nkt + 1) & ~1) * 16;   // keys staged: the second product steps by 32 (f16)

  {
    constexpr int KC = HD / E;
    for (int e = tid; e < kp * KC; e += AS_THREADS) {
      const int key = e / KC, c = e % KC;
      chunk_t v = zero_chunk<T>();
      if (key < len) v = *(const chunk_t*)(p.k + (row0 + key) * p.ldk + head * HD + c * E);
      *(chunk_t*)&Ks[L::k(key, c * E)] = v;
    }
    const int VC = kp / E;
    for (int e = tid; e < HD * VC; e += AS_THREADS) {
      const int d = e / VC, key = (e % VC) * E;
      chunk_t v = zero_chunk<T>();
      if (key < len) {      // len <= npad, npad % 8 == 0: the chunk lies inside the sequence's columns
        v = *(const chunk_t*)(p.vt + ((size_t)head * HD + d) * p.ldv + row0 + key);
#pragma unroll
        for (int j = 0; j < E; ++j)
          if (key + j >= len) v[j] = (T)0.f;
      }
      *(chunk_t*)&Vs[L::v(d, key)] = v;
    }
  }
  __syncthreads();

  const float slope = p.slope ? p.slope[head] : 0.f;
  const int ntiles = (npad + 15) >> 4;
  for (int qt = wave; qt < ntiles; qt += 4) {
    const int query = qt * 16 + n;
    // Q^T B operands: lane (g, n) holds Q[query n][d = 4 E ks + E g + j]
    chunk_t qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      qf[ks] = zero_chunk<T>();
      if (query < npad) qf[ks] = *(const chunk_t*)(p.q + (row0 + query) * p.ldq + head * HD + ks * 4 * E + g * E);
    }
    // S^T: s[t][r] = score of key 16 t + 4 g + r for query n
    float4v s[AS_MAXK / 16];
#pragma unroll
    for (int t = 0; t < AS_MAXK / 16; ++t) {
      s[t] = (float4v){0.f, 0.f, 0.f, 0.f};
      if (t < nkt) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const chunk_t a = *(const chunk_t*)&Ks[L::k(t * 16 + n, ks * 4 * E + g * E)];
          X::mma(a, qf[ks], s[t]);
        }
        if (p.slope) {
#pragma unroll
          for (int r = 0; r < 4; ++r) s[t][r] -= slope * fabsf((float)(query - (t * 16 + 4 * g + r)));
        }
        if (t == nkt - 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (t * 16 + 4 * g + r >= len) s[t][r] = -INFINITY;
        }
      }
    }
    float m = -INFINITY;      // key 0 is a key of every sequence: the maximum is finite
#pragma unroll
    for (int t = 0; t < AS_MAXK / 16; ++t)
      if (t < nkt) m = fmaxf(fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])), m);
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < AS_MAXK / 16; ++t)
      if (t < nkt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][r] = __builtin_amdgcn_exp2f(s[t][r] - m);
        l += (s[t][0] + s[t][1]) + (s[t][2] + s[t][3]);
      }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);

    // O^T: o[dt][r] = output d = 16 dt + 4 g + r of query n
    float4v o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] = (float4v){0.f, 0.f, 0.f, 0.f};
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int t0 = 0; t0 < AS_MAXK / 16; t0 += 2)
        if (t0 < nkt) {
          // k index of the step: element j of lane group g is key 16 (t0 + (j >> 2)) + 4 g + (j & 3), in both operands
          half8 b;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            b[r] = (_Float16)s[t0][r];
            b[4 + r] = t0 + 1 < nkt ? (_Float16)s[t0 + 1][r] : (_Float16)0.f;
          }
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const half4 lo = *(const half4*)&Vs[L::v(dt * 16 + n, t0 * 16 + 4 * g)];
            const half4 hi = *(const half4*)&Vs[L::v(dt * 16 + n, t0 * 16 + 16 + 4 * g)];
            const half8 a = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            X::mma(a, b, o[dt]);
          }
        }
    } else {
#pragma unroll
      for (int t = 0; t < AS_MAXK / 16; ++t)
        if (t < nkt) {
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const float4v a = *(const float4v*)&Vs[L::v(dt * 16 + n, t * 16 + 4 * g)];
            X::mma(a, s[t], o[dt]);
          }
        }
    }
    if (query < npad) {
      const float inv = 1.f / l;
      T* dst = p.out + (row0 + query) * p.ldo + head * HD + 4 * g;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        if constexpr (sizeof(T) == 2) {
          half4 w;
#pragma unroll
          for (int r = 0; r < 4; ++r) w[r] = (_Float16)(o[dt][r] * inv);
          *(half4*)(dst + dt * 16) = w;
        } else {
          *(float4v*)(dst + dt * 16) = o[dt] * inv;
        }
      }
    }
  }
}

// attn_long: the same attention for sequences past AS_MAXK keys.  One workgroup = one (sequence, head, block of 64 queries), a
// 16-query tile a wave; the keys arrive in blocks of AS_MAXK, 0 .. ceil(len / AS_MAXK) - 1 in that order, each staged into the
// same LDS images and walked as attn_short walks its key tiles (transposed products, ALiBi from the absolute key index, the -inf
// select in the block's last tile), then folded into the running state of the online soft-max:
//   m' = max(m, block max)   alpha = exp2(m - m')   l = l alpha + sum p   o = o alpha, then the block's second product
// and o / l at the end.  The first key of every walked block is a key of the sequence, so no block maximum is -inf; alpha of the
// first block is exp2(-inf) = 0 on o = l = 0.  The walk is a function of len alone.  A query block that starts at or past len
// writes zeros and leaves before any barrier.  m, alpha, l and o are fp32 in both modes; l is kept as the lane's partial sum (the
// four lane groups of a query share m and alpha) and reduced once at the end.  One buffer, two barriers a block.
constexpr int AL_QB = 64;         // queries of a workgroup
constexpr int AL_MAXROWS = 8192;  // rows of a sequence: jina-embeddings-v2's 8192 tokens

template <typename T, int HD>
__global__ __launch_bounds__(AS_THREADS) void attn_long_kernel(ShortArgs<T> p) {
  typedef Tr<T> X;
  typedef typename X::chunk_t chunk_t;
  typedef AsLay<T, HD> L;
  constexpr int E = X::E;
  constexpr int NKS = HD / (4 * E);
  constexpr int NDT = HD / 16;
  __shared__ __attribute__((aligned(16))) T Ks[L::KSZ];
  __shared__ __attribute__((aligned(16))) T Vs[L::VSZ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const int head = blockIdx.x % p.heads, seq = blockIdx.x / p.heads;
  const int npad = p.npad;
  const size_t row0 = (size_t)seq * npad;
  const int len = min(max(p.len[seq], 1), npad);
  const int q0 = blockIdx.y * AL_QB;
  const int query = q0 + wave * 16 + n;
  T* dst = p.out + (row0 + query) * p.ldo + head * HD + 4 * g;

  if (q0 >= len) {      // uniform over the workgroup: nobody reads these rows, they are written as zeros
    if (query < npad) {
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        if constexpr (sizeof(T) == 2) *(half4*)(dst + dt * 16) = (half4){(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
        else *(float4v*)(dst + dt * 16) = (float4v){0.f, 0.f, 0.f, 0.f};
      }
    }
    return;
  }

  // Q^T B operands: lane (g, n) holds Q[query n][d = 4 E ks + E g + j]; a tile past npad computes on zeros and stores nothing
  chunk_t qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    qf[ks] = zero_chunk<T>();
    if (query < npad) qf[ks] = *(const chunk_t*)(p.q + (row0 + query) * p.ldq + head * HD + ks * 4 * E + g * E);
  }
  const float slope = p.slope ? p.slope[head] : 0.f;
  float m = -INFINITY, l = 0.f;
  float4v o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = (float4v){0.f, 0.f, 0.f, 0.f};

  const int nkb = (len + AS_MAXK - 1) / AS_MAXK;
  for (int kb = 0; kb < nkb; ++kb) {
    const int k0 = kb * AS_MAXK;
    const int blen = min(len - k0, AS_MAXK);      // keys of this block, >= 1
    const int nkt = (blen + 15) >> 4;
    const int kp = ((nkt + 1) & ~1) * 16;
    if (kb) __syncthreads();      // the block before has been read
    {
      constexpr int KC = HD / E;
      for (int e = tid; e < kp * KC; e += AS_THREADS) {
        const int key = e / KC, c = e % KC;
        chunk_t v = zero_chunk<T>();
        if (key < blen) v = *(const chunk_t*)(p.k + (row0 + k0 + key) * p.ldk + head * HD + c * E);
        *(chunk_t*)&Ks[L::k(key, c * E)] = v;
      }
      const int VC = kp / E;
      for (int e = tid; e < HD * VC; e += AS_THREADS) {
        const int d = e / VC, key = (e % VC) * E;
        chunk_t v = zero_chunk<T>();
        if (key < blen) {      // k0 + key < len <= npad, npad % 8 == 0: the chunk lies inside the sequence's columns
          v = *(const chunk_t*)(p.vt + ((size_t)head * HD + d) * p.ldv + row0 + k0 + key);
#pragma unroll
          for (int j = 0; j < E; ++j)
            if (key + j >= blen) v[j] = (T)0.f;
        }
        *(chunk_t*)&Vs[L::v(d, key)] = v;
      }
    }
    __syncthreads();

    // S^T of the block: s[t][r] = score of key k0 + 16 t + 4 g + r for query n
    float4v s[AS_MAXK / 16];
#pragma unroll
    for (int t = 0; t < AS_MAXK / 16; ++t) {
      s[t] = (float4v){0.f, 0.f, 0.f, 0.f};
      if (t < nkt) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const chunk_t a = *(const chunk_t*)&Ks[L::k(t * 16 + n, ks * 4 * E + g * E)];
          X::mma(a, qf[ks], s[t]);
        }
        if (p.slope) {
#pragma unroll
          for (int r = 0; r < 4; ++r) s[t][r] -= slope * fabsf((float)(query - (k0 + t * 16 + 4 * g + r)));
        }
        if (t == nkt - 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (t * 16 + 4 * g + r >= blen) s[t][r] = -INFINITY;
        }
      }
    }
    float mb = -INFINITY;      // key k0 is a key of the sequence: the block's maximum is finite
#pragma unroll
    for (int t = 0; t < AS_MAXK / 16; ++t)
      if (t < nkt) mb = fmaxf(fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])), mb);
    mb = fmaxf(mb, __shfl_xor(mb, 16));
    mb = fmaxf(mb, __shfl_xor(mb, 32));
    const float mn = fmaxf(m, mb);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    float lb = 0.f;
#pragma unroll
    for (int t = 0; t < AS_MAXK / 16; ++t)
      if (t < nkt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][r] = __builtin_amdgcn_exp2f(s[t][r] - mn);
        lb += (s[t][0] + s[t][1]) + (s[t][2] + s[t][3]);
      }
    l = l * alpha + lb;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] = o[dt] * alpha;

    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int t0 = 0; t0 < AS_MAXK / 16; t0 += 2)
        if (t0 < nkt) {
          half8 b;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            b[r] = (_Float16)s[t0][r];
            b[4 + r] = t0 + 1 < nkt ? (_Float16)s[t0 + 1][r] : (_Float16)0.f;
          }
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const half4 lo = *(const half4*)&Vs[L::v(dt * 16 + n, t0 * 16 + 4 * g)];
            const half4 hi = *(const half4*)&Vs[L::v(dt * 16 + n, t0 * 16 + 16 + 4 * g)];
            const half8 a = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            X::mma(a, b, o[dt]);
          }
        }
    } else {
#pragma unroll
      for (int t = 0; t < AS_MAXK / 16; ++t)
        if (t < nkt) {
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const float4v a = *(const float4v*)&Vs[L::v(dt * 16 + n, t * 16 + 4 * g)];
            X::mma(a, s[t], o[dt]);
          }
        }
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (query < npad) {
    const float inv = 1.f / l;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      if constexpr (sizeof(T) == 2) {
        half4 w;
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = (_Float16)(o[dt][r] * inv);
        *(half4*)(dst + dt * 16) = w;
      } else {
        *(float4v*)(dst + dt * 16) = o[dt] * inv;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------- rows
// a lane's float4 groups of the row -> the fp32 stream and the operand of the next GEMM
template <typename T>
__device__ __forceinline__ void store_row(const float4v v[ROW_GROUPS], float* __restrict__ h, T* __restrict__ ht, size_t row, int D, int lane) {
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) {
      *(float4v*)(h + row * D + c) = v[i];
      if (ht) {
        T o4[4] = {(T)v[i][0], (T)v[i][1], (T)v[i][2], (T)v[i][3]};
        if (sizeof(T) == 2) *(uint64_t*)(ht + row * D + c) = *(uint64_t*)o4;
        else *(float4v*)(ht + row * D + c) = *(float4v*)o4;
      }
    }
  }
}

// h[seq][t] = LN((word[ids[seq][t]] + type0) + pos[t]) (pos null: no position table), one wave per row, 16 bytes a lane
template <typename T>
__global__ __launch_bounds__(256) void berttext_embed_kernel(const float* __restrict__ word, const float* __restrict__ type0,
                                                             const float* __restrict__ pos, const float* __restrict__ g,
                                                             const float* __restrict__ b, const int* __restrict__ ids,
                                                             float* __restrict__ h, T* __restrict__ ht, int rows, int npad, int D,
                                                             float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* src = word + (size_t)ids[row] * D;
  const float* pp = pos ? pos + (size_t)(row % npad) * D : nullptr;
  float4v v[ROW_GROUPS];
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = (float4v){0.f, 0.f, 0.f, 0.f};
    if (c < D) {
      v[i] = *(const float4v*)(src + c) + *(const float4v*)(type0 + c);
      if (pp) v[i] += *(const float4v*)(pp + c);
    }
  }
  row_layernorm(v, D, lane, g, b, eps);
  store_row<T>(v, h, ht, (size_t)row, D, lane);
}

// the post-LayerNorm of a layer: h = LN(x), ht its copy in the GEMM element type
template <typename T>
__global__ __launch_bounds__(256) void berttext_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                 const float* __restrict__ b, float* __restrict__ h,
                                                                 T* __restrict__ ht, int rows, int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float4v v[ROW_GROUPS];
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = (float4v){0.f, 0.f, 0.f, 0.f};
    if (c < D) v[i] = *(const float4v*)(x + (size_t)row * D + c);
  }
  row_layernorm(v, D, lane, g, b, eps);
  store_row<T>(v, h, ht, (size_t)row, D, lane);
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

inline int grid_for(long long total, int block) { return (int)std::min<long long>((total + block - 1) / block, 65535LL * 4); }
inline bool row_width_ok(int D) { return D >= 64 && D % 64 == 0 && D <= 256 * ROW_GROUPS; }

template <typename T, int HD>
void launch_short(mhip_ctx* ctx, const AttnShortDesc& s) {
  const AttnDesc& d = s.a;
  ShortArgs<T> a;
  a.q = (const T*)d.q; a.k = (const T*)d.k; a.vt = (const T*)d.vt; a.out = (T*)d.out;
  a.len = s.len; a.slope = s.slopes;
  a.ldq = d.ldq; a.ldk = d.ldk; a.ldv = d.ldv; a.ldo = d.ldo;
  a.npad = d.npad_k; a.heads = d.heads;
  PROF_LAUNCH(ctx, MHIP_K_ATTN_SHORT, hipLaunchKernelGGL((attn_short_kernel<T, HD>), dim3((unsigned)(d.images * d.heads)), dim3(AS_THREADS), 0, ctx->stream, a));
}

template <typename T, int HD>
void launch_long(mhip_ctx* ctx, const AttnShortDesc& s) {
  const AttnDesc& d = s.a;
  ShortArgs<T> a;
  a.q = (const T*)d.q; a.k = (const T*)d.k; a.vt = (const T*)d.vt; a.out = (T*)d.out;
  a.len = s.len; a.slope = s.slopes;
  a.ldq = d.ldq; a.ldk = d.ldk; a.ldv = d.ldv; a.ldo = d.ldo;
  a.npad = d.npad_k; a.heads = d.heads;
  const dim3 grid((unsigned)(d.images * d.heads), (unsigned)((d.npad_k + AL_QB - 1) / AL_QB));
  // no slot of its own: the profiler's list is pinned, and a call runs one of the two attentions
  PROF_LAUNCH(ctx, MHIP_K_ATTN_SHORT, hipLaunchKernelGGL((attn_long_kernel<T, HD>), grid, dim3(AS_THREADS), 0, ctx->stream, a));
}

}  // namespace

int mhip_launch_attention_short(mhip_ctx* ctx, int precision, const AttnShortDesc& s) {
  const AttnDesc& d = s.a;
  if (s.head_dim != 64 && s.head_dim != 32) return mhip_fail(ctx, MHIP_EINVAL, "attention_short: head_dim %d (64 or 32)", s.head_dim);
  if (!s.len || d.images <= 0 || d.heads <= 0 || (long long)d.images * d.heads > 0x7fffffffLL || d.npad_k < 8 || d.npad_k % 8 ||
      d.npad_k > AS_MAXK || d.npad_q != d.npad_k)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_short: bad shape (%d sequences, %d heads, %d rows of at most %d)", d.images, d.heads, d.npad_k, AS_MAXK);
  const int esz = precision == MHIP_PREC_F16 ? 2 : 4;
  if ((d.ldq * esz) % 16 || (d.ldk * esz) % 16 || (d.ldv * esz) % 16 || (d.ldo * esz) % 16 || d.ldv < d.images * d.npad_k ||
      ((uintptr_t)d.q & 15) || ((uintptr_t)d.k & 15) || ((uintptr_t)d.vt & 15) || ((uintptr_t)d.out & 15))
    return mhip_fail(ctx, MHIP_EINVAL, "attention_short: rows must keep 16-byte alignment");
  // the lengths live on the device: counted as full sequences
  if (ctx->profiling) ctx->prof[MHIP_K_ATTN_SHORT].flops += 4.0 * d.images * d.heads * (double)d.npad_k * d.npad_k * s.head_dim;
  if (precision == MHIP_PREC_F16) {
    if (s.head_dim == 64) launch_short<_Float16, 64>(ctx, s);
    else launch_short<_Float16, 32>(ctx, s);
  } else {
    if (s.head_dim == 64) launch_short<float, 64>(ctx, s);
    else launch_short<float, 32>(ctx, s);
  }
  CHECK_LAUNCH(ctx, "attention_short");
  return 0;
}

int mhip_launch_attention_long(mhip_ctx* ctx, int precision, const AttnShortDesc& s) {
  const AttnDesc& d = s.a;
  if (s.head_dim != 64 && s.head_dim != 32) return mhip_fail(ctx, MHIP_EINVAL, "attention_long: head_dim %d (64 or 32)", s.head_dim);
  if (!s.len) return mhip_fail(ctx, MHIP_EINVAL, "attention_long: len is null");
  if (d.images <= 0 || d.heads <= 0 || (long long)d.images * d.heads > 0x7fffffffLL)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_long: images %d, heads %d", d.images, d.heads);
  if (d.npad_k < 8 || d.npad_k % 8 || d.npad_k > AL_MAXROWS)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_long: npad_k %d (a multiple of 8, 8 .. %d)", d.npad_k, AL_MAXROWS);
  if (d.npad_q != d.npad_k) return mhip_fail(ctx, MHIP_EINVAL, "attention_long: npad_q %d is not npad_k %d", d.npad_q, d.npad_k);
  const int esz = precision == MHIP_PREC_F16 ? 2 : 4;
  if ((d.ldq * esz) % 16 || (d.ldk * esz) % 16 || (d.ldv * esz) % 16 || (d.ldo * esz) % 16 || (long long)d.ldv < (long long)d.images * d.npad_k ||
      ((uintptr_t)d.q & 15) || ((uintptr_t)d.k & 15) || ((uintptr_t)d.vt & 15) || ((uintptr_t)d.out & 15))
    return mhip_fail(ctx, MHIP_EINVAL, "attention_long: rows must keep 16-byte alignment (ldq, ldk, ldv, ldo, the pointers), ldv the whole batch");
  // the lengths live on the device: counted as full sequences
  if (ctx->profiling) ctx->prof[MHIP_K_ATTN_SHORT].flops += 4.0 * d.images * d.heads * (double)d.npad_k * d.npad_k * s.head_dim;
  if (precision == MHIP_PREC_F16) {
    if (s.head_dim == 64) launch_long<_Float16, 64>(ctx, s);
    else launch_long<_Float16, 32>(ctx, s);
  } else {
    if (s.head_dim == 64) launch_long<float, 64>(ctx, s);
    else launch_long<float, 32>(ctx, s);
  }
  CHECK_LAUNCH(ctx, "attention_long");
  return 0;
}

int mhip_launch_berttext_embed(mhip_ctx* ctx, int precision, const float* word, const float* type0, const float* pos, const float* g,
                               const float* b, float eps, const int* ids, float* h, void* ht, int B, int npad, int D) {
  if (B <= 0 || npad < 1 || !row_width_ok(D)) return mhip_fail(ctx, MHIP_EINVAL, "berttext_embed: B=%d npad=%d D=%d", B, npad, D);
  const int rows = B * npad;
  dim3 grid((rows + 3) / 4), block(256);
  if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_BERTTEXT_EMBED, hipLaunchKernelGGL(berttext_embed_kernel<_Float16>, grid, block, 0, ctx->stream, word, type0, pos, g, b, ids, h, (_Float16*)ht, rows, npad, D, eps));
  else
    PROF_LAUNCH(ctx, MHIP_K_BERTTEXT_EMBED, hipLaunchKernelGGL(berttext_embed_kernel<float>, grid, block, 0, ctx->stream, word, type0, pos, g, b, ids, h, (float*)ht, rows, npad, D, eps));
  CHECK_LAUNCH(ctx, "berttext_embed");
  return 0;
}

int mhip_launch_berttext_layernorm(mhip_ctx* ctx, int precision, const float* x, const float* g, const float* b, float* h, void* ht,
                                   int rows, int D, float eps) {
  if (rows <= 0 || !row_width_ok(D)) return mhip_fail(ctx, MHIP_EINVAL, "berttext_layernorm: D=%d rows=%d", D, rows);
  dim3 grid((rows + 3) / 4), block(256);
  if (precision == MHIP_PREC_F16)
    PROF_LAUNCH(ctx, MHIP_K_BERTTEXT_EMBED, hipLaunchKernelGGL(berttext_layernorm_kernel<_Float16>, grid, block, 0, ctx->stream, x, g, b, h, (_Float16*)ht, rows, D, eps));
  else
    PROF_LAUNCH(ctx, MHIP_K_BERTTEXT_EMBED, hipLaunchKernelGGL(berttext_layernorm_kernel<float>, grid, block, 0, ctx->stream, x, g, b, h, (float*)ht, rows, D, eps));
  CHECK_LAUNCH(ctx, "berttext_layernorm");
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
