// cliptext_ops.hip — the two kernels the CLIP text tower has that the vision tower (clip_ops.hip) does not: the token + position
// embedding, and causal soft-max attention at head dim 64 over sequences of at most 128 rows.
//
// Replaces, in transformers/models/clip/modeling_clip.py: CLIPTextEmbeddings.forward and the attention of CLIPEncoderLayer under
// the causal mask of CLIPTextTransformer (the same arithmetic as clip/model.py: CLIP.encode_text's token_embedding +
// positional_embedding and the attn_mask of build_attention_mask).
//
// attn_causal: one workgroup = one (sequence, head).  K and V^T of that head are staged in LDS once (keys past npad as zeros);
// each wave owns the 16-query tiles wave, wave + 4.  As in attn_flash.hip the products are taken transposed,  S^T = K Q^T  and
// O^T = V^T P^T,  so a query is a lane's column (C layout: col = lane & 15, row = 4 (lane >> 4) + reg): a lane holds, of its
// query's score row, keys 16 t + 4 g + r of every 16-key tile t, and those registers are the B operand of the second product
// with no lane movement: the A operand (V^T) is read from LDS at the same keys.  A query tile qt walks the key tiles 0 .. qt in
// that order — a function of the row's position alone, never of npad or of the batch — the whole score row stays in registers
// (at most 8 tiles x 4), the mask is applied before the row maximum, and no online rescaling is needed.  Scores are in log2
// units: q arrives scaled by ATTN_SCORE_SCALE.
//   f16: v_mfma_f32_16x16x32_f16 for both products (two key tiles make one 32-key step of the second; a tile past qt enters as
//        zeros), probabilities rounded to f16 only as that operand; the row sum is of the fp32 probabilities.
//   f32: v_mfma_f32_16x16x4_f32, an fp32 fma chain: no f16 value anywhere.
#include <algorithm>

#include "igemm_common.h"

using namespace igemm;

namespace {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));

constexpr int CA_MAXK = 128;      // keys of a sequence (mhip_cliptext: context <= 128)
constexpr int CA_THREADS = 256;

// LDS images of K [key][d] and V^T [d][key].  f16: padded rows (144 / 272 bytes); f32: 16-byte chunks XOR-swizzled by the row,
// unpadded, so that both images fit in 64 KiB
template <typename T>
struct CaLay;
template <>
struct CaLay<_Float16> {
  static constexpr int KP = 72, VP = CA_MAXK + 8;
  static constexpr int KSZ = CA_MAXK * KP, VSZ = 64 * VP;
  static __device__ __forceinline__ int k(int key, int d) { return key * KP + d; }
  static __device__ __forceinline__ int v(int d, int key) { return d * VP + key; }
};
template <>
struct CaLay<float> {
  static constexpr int KSZ = CA_MAXK * 64, VSZ = 64 * CA_MAXK;
  // d, key: multiples of 4
  static __device__ __forceinline__ int k(int key, int d) { return key * 64 + ((((d >> 2) ^ key) & 15) << 2); }
  static __device__ __forceinline__ int v(int d, int key) { return d * CA_MAXK + (((key >> 2) ^ (d & 15)) << 2); }
};

template <typename T>
struct CausalArgs {
  const T* q;      // [seqs * npad][ldq], head h at column h * 64, in ATTN_SCORE_SCALE units
  const T* k;      // [seqs * npad][ldk]
  const T* vt;     // [heads * 64][ldv], column = seq * npad + key
  T* out;          // [seqs * npad][ldo]
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

template <typename T>
__global__ __launch_bounds__(CA_THREADS) void attn_causal_kernel(CausalArgs<T> p) {
  typedef Tr<T> X;
  typedef typename X::chunk_t chunk_t;
  typedef CaLay<T> L;
  constexpr int E = X::E;                 // elements of a 16-byte chunk
  constexpr int NKS = 64 / (4 * E);       // MFMA steps over the head dim
  __shared__ __attribute__((aligned(16))) T Ks[L::KSZ];
  __shared__ __attribute__((aligned(16))) T Vs[L::VSZ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const int head = blockIdx.x % p.heads, seq = blockIdx.x / p.heads;
  const int npad = p.npad;
  const size_t row0 = (size_t)seq * npad;
  const int kp = (npad + 31) & ~31;       // keys staged: the second product steps by 32 (f16)

  {
    constexpr int KC = 64 / E;
    for (int e = tid; e < kp * KC; e += CA_THREADS) {
      const int key = e / KC, c = e % KC;
      chunk_t v = zero_chunk<T>();
      if (key < npad) v = *(const chunk_t*)(p.k + (row0 + key) * p.ldk + head * 64 + c * E);
      *(chunk_t*)&Ks[L::k(key, c * E)] = v;
    }
    const int VC = kp / E;
    for (int e = tid; e < 64 * VC; e += CA_THREADS) {
      const int d = e / VC, key = (e % VC) * E;
      chunk_t v = zero_chunk<T>();
      if (key < npad) v = *(const chunk_t*)(p.vt + ((size_t)head * 64 + d) * p.ldv + row0 + key);      // npad % 8 == 0: all in or all out
      *(chunk_t*)&Vs[L::v(d, key)] = v;
    }
  }
  __syncthreads();

  const int ntiles = (npad + 15) >> 4;
  for (int qt = wave; qt < ntiles; qt += 4) {
    const int query = qt * 16 + n;
    // Q^T B operands: lane (g, n) holds Q[query n][d = 4 E ks + E g + j]
    chunk_t qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      qf[ks] = zero_chunk<T>();
      if (query < npad) qf[ks] = *(const chunk_t*)(p.q + (row0 + query) * p.ldq + head * 64 + ks * 4 * E + g * E);
    }
    // S^T: s[t][r] = score of key 16 t + 4 g + r for query n
    float4v s[CA_MAXK / 16];
#pragma unroll
    for (int t = 0; t < CA_MAXK / 16; ++t) {
      s[t] = (float4v){0.f, 0.f, 0.f, 0.f};
      if (t <= qt) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const chunk_t a = *(const chunk_t*)&Ks[L::k(t * 16 + n, ks * 4 * E + g * E)];
          X::mma(a, qf[ks], s[t]);
        }
        if (t == qt) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (4 * g + r > n) s[t][r] = -INFINITY;
        }
      }
    }
    float m = -INFINITY;      // key 0 is visible to every row: the maximum is finite
#pragma unroll
    for (int t = 0; t < CA_MAXK / 16; ++t)
      if (t <= qt) m = fmaxf(fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])), m);
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < CA_MAXK / 16; ++t)
      if (t <= qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][r] = __builtin_amdgcn_exp2f(s[t][r] - m);
        l += (s[t][0] + s[t][1]) + (s[t][2] + s[t][3]);
      }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);

    // O^T: o[dt][r] = output d = 16 dt + 4 g + r of query n
    float4v o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (float4v){0.f, 0.f, 0.f, 0.f};
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int t0 = 0; t0 < CA_MAXK / 16; t0 += 2)
        if (t0 <= qt) {
          // k index of the step: element j of lane group g is key 16 (t0 + (j >> 2)) + 4 g + (j & 3), in both operands
          half8 b;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            b[r] = (_Float16)s[t0][r];
            b[4 + r] = t0 + 1 <= qt ? (_Float16)s[t0 + 1][r] : (_Float16)0.f;
          }
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const half4 lo = *(const half4*)&Vs[L::v(dt * 16 + n, t0 * 16 + 4 * g)];
            const half4 hi = *(const half4*)&Vs[L::v(dt * 16 + n, t0 * 16 + 16 + 4 * g)];
            const half8 a = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            X::mma(a, b, o[dt]);
          }
        }
    } else {
#pragma unroll
      for (int t = 0; t < CA_MAXK / 16; ++t)
        if (t <= qt) {
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const float4v a = *(const float4v*)&Vs[L::v(dt * 16 + n, t * 16 + 4 * g)];
            X::mma(a, s[t], o[dt]);
          }
        }
    }
    if (query < npad) {
      const float inv = 1.f / l;
      T* dst = p.out + (row0 + query) * p.ldo + head * 64 + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
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

// ------------------------------------------------------------------------------------------------------- embedding
// h[seq][t] = table[ids[seq][t]] + pos[t], fp32, one wave per row, 16 bytes a lane
constexpr int ROW_GROUPS = 4;      // float4 groups per lane: D <= 1024

__global__ __launch_bounds__(256) void cliptext_embed_kernel(const float* __restrict__ table, const float* __restrict__ pos,
                                                             const int* __restrict__ ids, float* __restrict__ h, int rows,
                                                             int npad, int D) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* src = table + (size_t)ids[row] * D;
  const float* pp = pos + (size_t)(row % npad) * D;
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) *(float4v*)(h + (size_t)row * D + c) = *(const float4v*)(src + c) + *(const float4v*)(pp + c);
  }
}

template <typename T>
int launch_causal(mhip_ctx* ctx, const AttnDesc& d) {
  CausalArgs<T> a;
  a.q = (const T*)d.q; a.k = (const T*)d.k; a.vt = (const T*)d.vt; a.out = (T*)d.out;
  a.ldq = d.ldq; a.ldk = d.ldk; a.ldv = d.ldv; a.ldo = d.ldo;
  a.npad = d.npad_k; a.heads = d.heads;
  PROF_LAUNCH(ctx, MHIP_K_ATTN_CAUSAL, hipLaunchKernelGGL(attn_causal_kernel<T>, dim3((unsigned)(d.images * d.heads)), dim3(CA_THREADS), 0, ctx->stream, a));
  return 0;
}

}  // namespace

int mhip_launch_attention_causal(mhip_ctx* ctx, int precision, const AttnDesc& d) {
  if (d.images <= 0 || d.heads <= 0 || (long long)d.images * d.heads > 0x7fffffffLL || d.npad_k < 8 || d.npad_k % 8 ||
      d.npad_k > CA_MAXK || d.npad_q != d.npad_k || d.n_queries != d.n_keys || d.n_keys < 1 || d.n_keys > d.npad_k)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_causal: bad shape (%d sequences, %d heads, %d/%d rows of at most %d)", d.images, d.heads,
                     d.n_keys, d.npad_k, CA_MAXK);
  const int esz = precision == MHIP_PREC_F16 ? 2 : 4;
  if ((d.ldq * esz) % 16 || (d.ldk * esz) % 16 || (d.ldv * esz) % 16 || (d.ldo * esz) % 16 || d.ldv < d.images * d.npad_k ||
      ((uintptr_t)d.q & 15) || ((uintptr_t)d.k & 15) || ((uintptr_t)d.vt & 15) || ((uintptr_t)d.out & 15))
    return mhip_fail(ctx, MHIP_EINVAL, "attention_causal: rows must keep 16-byte alignment");
  if (ctx->profiling) ctx->prof[MHIP_K_ATTN_CAUSAL].flops += 2.0 * d.images * d.heads * (double)d.n_keys * (d.n_keys + 1) * 64;
  if (precision == MHIP_PREC_F16) launch_causal<_Float16>(ctx, d);
  else launch_causal<float>(ctx, d);
  CHECK_LAUNCH(ctx, "attention_causal");
  return 0;
}

int mhip_launch_cliptext_embed(mhip_ctx* ctx, const float* table, const float* pos, const int* ids, float* h, int B, int npad, int D) {
  if (B <= 0 || npad < 1 || D < 64 || D % 64 || D > 256 * ROW_GROUPS) return mhip_fail(ctx, MHIP_EINVAL, "cliptext_embed: B=%d npad=%d D=%d", B, npad, D);
  const int rows = B * npad;
  PROF_LAUNCH(ctx, MHIP_K_CLIPTEXT_EMBED, hipLaunchKernelGGL(cliptext_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, ctx->stream, table, pos, ids, h, rows, npad, D));
  CHECK_LAUNCH(ctx, "cliptext_embed");
  return 0;
}
