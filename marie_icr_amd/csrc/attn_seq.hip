// attn_seq.hip — soft-max attention of the text towers, one sequence at a time with its keys in LDS: causal over at most 128 rows
// (attn_causal: the CLIP text tower, cliptext_api.hip), over sequences of their own length with optional ALiBi (attn_short: the
// BERT encoders at up to 128 rows, berttext_api.hip), and the same with the keys streamed in blocks of 128 under an online
// soft-max (attn_long: up to 8192 rows).  Every step is written once, in Seq<T, HD> below; the kernels differ in four things:
// which key tiles a query tile walks and which scores of the last walked tile become -inf (data: `nvis`, `limit`), the ALiBi
// term (a branch), the relative-distance table's term (MPNet: a template parameter, so the instances without it are the code
// they were), and whether the block's result is normalised directly or folded into a running (m, l, o).  Longformer's attention
// (berttext_api.hip with windows) is two more kernels, described where they stand: attn_window, the streamed kernel over a band
// of keys plus key 0 (the *_band steps of Seq), and attn_global_row, the global token's single query over all keys.
//
// Replaces, in transformers/models/clip/modeling_clip.py: the attention of CLIPEncoderLayer under the causal mask of
// CLIPTextTransformer (clip/model.py: the attn_mask of build_attention_mask); in transformers/models/bert/modeling_bert.py: the
// attention of BertSelfAttention under the padding mask, and of JinaBERT the symmetric ALiBi bias; in transformers/models/mpnet/
// modeling_mpnet.py: the attention of MPNetSelfAttention under MPNetEncoder.compute_position_bias.
//
// Whole-row kernel (attn_causal, attn_short): one workgroup = one (sequence, head).  K and V^T of that head are staged in LDS
// once (keys past the sequence's as zeros); each wave owns the 16-query tiles wave, wave + 4.  As in attn_flash.hip the products
// are taken transposed,  S^T = K Q^T  and  O^T = V^T P^T,  so a query is a lane's column (C layout: col = lane & 15, row =
// 4 (lane >> 4) + reg): a lane holds, of its query's score row, keys 16 t + 4 g + r of every 16-key tile t, and those registers
// are the B operand of the second product with no lane movement: the A operand (V^T) is read from LDS at the same keys.  The
// whole score row stays in registers (at most 8 tiles x 4), the mask is applied before the row maximum, and no online rescaling
// is needed.  Scores are in log2 units: q arrives scaled by head_dim^-0.5 * log2(e).
//   * causal: query tile qt walks the key tiles 0 .. qt in that order — a function of the row's position alone, never of npad or
//     of the batch — and masks key > query.  Head dim 64 only.
//   * with lengths: a sequence has len[b] keys (1 <= len <= npad).  A query tile walks the key tiles 0 .. ceil(len / 16) - 1 in
//     that order — a function of len alone, never of npad or of the batch — keys >= len are staged as zeros and their scores are
//     -inf, so a sequence's rows do not depend on what it is batched with, bit for bit.  Query rows >= len are
//     computed like any other row: finite, and nobody reads them.
//   * with slopes, the score of (query i, key j) gets  - slope[head] * |i - j|  (ALiBi, symmetric), in the log2 units q carries;
//     without slopes there is no bias term.
//   * with a table (REL instances; never with slopes, never causal), the score of (query i, key j) gets
//     table[head][clamp(i - j, -R, R) + R], fp32 in the log2 units q carries, finite: a lane reads its four values a tile through
//     the vector cache (257 floats a head at R = 128: the table stays resident), the index taken from `dist` and the tile.
//   * the head dim HD is 64 or 32: at 32 the first product is one 16x16x32 f16 step and O^T has two 16-row tiles.
//   f16: v_mfma_f32_16x16x32_f16 for both products (two key tiles make one 32-key step of the second; a tile past the last walked
//        enters as zeros), probabilities rounded to f16 only as that operand; the row sum is of the fp32 probabilities.
//   f32: v_mfma_f32_16x16x4_f32, an fp32 fma chain: no f16 value anywhere.
#include <algorithm>
#include <type_traits>

#include "igemm_common.h"

using namespace igemm;

namespace {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));

constexpr int SEQ_MAXK = 128;      // keys in LDS: a whole sequence (mhip_cliptext: context <= 128), or a block of the streamed walk
constexpr int SEQ_NT = SEQ_MAXK / 16;
constexpr int SEQ_THREADS = 256;
constexpr int SEQ_QB = 64;         // streamed: queries of a workgroup
constexpr int SEQ_MAXROWS = 8192;  // streamed: rows of a sequence (jina-embeddings-v2's 8192 tokens)

// LDS images of K [key][d] and V^T [d][key].  f16: padded rows (HD 64: 144 / 272 bytes); f32: 16-byte chunks XOR-swizzled by the
// row, unpadded, so that both images fit in 64 KiB at HD 64
template <typename T, int HD>
struct SeqLay;
template <int HD>
struct SeqLay<_Float16, HD> {
  static constexpr int KP = HD + 8, VP = SEQ_MAXK + 8;
  static constexpr int KSZ = SEQ_MAXK * KP, VSZ = HD * VP;
  static __device__ __forceinline__ int k(int key, int d) { return key * KP + d; }
  static __device__ __forceinline__ int v(int d, int key) { return d * VP + key; }
};
template <int HD>
struct SeqLay<float, HD> {
  static constexpr int KSZ = SEQ_MAXK * HD, VSZ = HD * SEQ_MAXK;
  // d, key: multiples of 4
  static __device__ __forceinline__ int k(int key, int d) { return key * HD + ((((d >> 2) ^ key) & (HD / 4 - 1)) << 2); }
  static __device__ __forceinline__ int v(int d, int key) { return d * SEQ_MAXK + (((key >> 2) ^ (d & 15)) << 2); }
};

template <typename T>
struct SeqArgs {
  const T* q;      // [seqs * npad][ldq], head h at column h * HD, in head_dim^-0.5 * log2(e) units
  const T* k;      // [seqs * npad][ldk]
  const T* vt;     // [heads * HD][ldv], column = seq * npad + key
  T* out;          // [seqs * npad][ldo]
  const int* len;        // [seqs], or null: causal
  const float* slope;    // [heads] in log2 units, or null
  int ldq, ldk, ldv, ldo;
  int npad, heads;
};
// the arguments of an instance: those above and, with REL, the relative-distance table.  Without REL the struct is SeqArgs<T>
template <typename T, bool REL>
struct SeqRelArgs : SeqArgs<T> {};
template <typename T>
struct SeqRelArgs<T, true> : SeqArgs<T> {
  const float* rel;      // [heads][2 rel_r + 1] in log2 units, finite
  int rel_r;
};

// The steps of one query tile (lane (g, n): query column n, lane group g) over one block of at most SEQ_MAXK keys in LDS.  A
// step that changes the score row builds its tile in a local and assigns it once: the steps are compiled on their own before
// they are inlined, and element-wise conditional stores through the reference cost the kernels 30 and more VGPRs
template <typename T, int HD>
struct Seq {
  typedef Tr<T> X;
  typedef typename X::chunk_t chunk_t;
  typedef SeqLay<T, HD> L;
  static constexpr int E = X::E;                 // elements of a 16-byte chunk
  static constexpr int NKS = HD / (4 * E);       // MFMA steps over the head dim
  static constexpr int NDT = HD / 16;            // 16-row tiles of O^T

  static __device__ __forceinline__ chunk_t zero_chunk() {
    chunk_t z;
#pragma unroll
    for (int j = 0; j < E; ++j) z[j] = (T)0.f;
    return z;
  }

  // keys staged for nkt key tiles: the second product steps by 32 (f16).  With nkt = ceil(npad / 16) this is (npad + 31) & ~31,
  // what the causal kernel staged before it shared this code: 16 (nkt rounded up to even) = npad rounded up to 32
  static __device__ __forceinline__ int staged(int nkt) { return ((nkt + 1) & ~1) * 16; }

  // keys k0 .. k0 + kp - 1 of the sequence at row0 -> Ks, Vs; those >= k0 + blen as zeros.  TRIM = false: blen % 8 == 0 (causal
  // stages blen = npad), no V chunk straddles it
  template <bool TRIM>
  static __device__ __forceinline__ void stage(const SeqArgs<T>& p, T* Ks, T* Vs, int head, size_t row0, int k0, int blen, int kp) {
    constexpr int KC = HD / E;
    for (int e = threadIdx.x; e < kp * KC; e += SEQ_THREADS) {
      const int key = e / KC, c = e % KC;
      chunk_t v = zero_chunk();
      if (key < blen) v = *(const chunk_t*)(p.k + (row0 + k0 + key) * p.ldk + head * HD + c * E);
      *(chunk_t*)&Ks[L::k(key, c * E)] = v;
    }
    const int VC = kp / E;
    for (int e = threadIdx.x; e < HD * VC; e += SEQ_THREADS) {
      const int d = e / VC, key = (e % VC) * E;
      chunk_t v = zero_chunk();
      if (key < blen) {      // k0 + key < len <= npad, npad % 8 == 0: the chunk lies inside the sequence's columns
        v = *(const chunk_t*)(p.vt + ((size_t)head * HD + d) * p.ldv + row0 + k0 + key);
        if constexpr (TRIM) {
#pragma unroll
          for (int j = 0; j < E; ++j)
            if (key + j >= blen) v[j] = (T)0.f;
        }
      }
      *(chunk_t*)&Vs[L::v(d, key)] = v;
    }
  }

  // Q^T B operands: lane (g, n) holds Q[query n][d = 4 E ks + E g + j]; a query past npad computes on zeros and stores nothing
  static __device__ __forceinline__ void load_q(const SeqArgs<T>& p, int head, size_t row0, int query, int g, chunk_t (&qf)[NKS]) {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      qf[ks] = zero_chunk();
      if (query < p.npad) qf[ks] = *(const chunk_t*)(p.q + (row0 + query) * p.ldq + head * HD + ks * 4 * E + g * E);
    }
  }

  // S^T of the block: s[t][r] = score of key k0 + 16 t + 4 g + r for query n, over the tiles t < nvis; in the last of them the
  // keys >= limit (counted from k0) become -inf.  alibi is uniform across the workgroup.  INIT: the mask goes on as the initial
  // value of the last tile's product (-inf + a finite product = -inf, and it stays -inf under the bias) and not as a select
  // on its result.  That is for a walk that is the same for every query tile (the whole-row kernel with lengths): the few
  // conditions are then kept across the tiles and nothing waits for the product.  It needs the masked keys' products finite,
  // which holds there because keys >= len are staged as zeros; causal masks keys the caller wrote, and keeps the select.
  // REL: rel is the head's table [2 R + 1]; key 16 t + 4 g + r of the block is at distance dist - 16 t - r from the query
  template <bool INIT, bool REL>
  static __device__ __forceinline__ void scores(const T* Ks, const chunk_t (&qf)[NKS], bool alibi, float slope, const float* rel, int R,
                                                int query, int k0, int nvis, int limit, int g, int n, float4v (&s)[SEQ_NT]) {
    // the lane's keys are 16 t + 4 g + r.  Mask and bias are written relative to one value a lane — the keys it has left in the
    // last visible tile, the distance of its first key — and not as one value a key, which would be kept across the tiles
    const int room = limit - (nvis - 1) * 16 - 4 * g, dist = query - k0 - 4 * g;
#pragma unroll
    for (int t = 0; t < SEQ_NT; ++t) {
      float4v c = {0.f, 0.f, 0.f, 0.f};
      if (t < nvis) {
        if (INIT && t == nvis - 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r >= room) c[r] = -INFINITY;
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const chunk_t a = *(const chunk_t*)&Ks[L::k(t * 16 + n, ks * 4 * E + g * E)];
          X::mma(a, qf[ks], c);
        }
        if (alibi) {
#pragma unroll
          for (int r = 0; r < 4; ++r) c[r] -= slope * fabsf((float)(dist - (t * 16 + r)));
        }
        if constexpr (REL) {
          float4v b;
#pragma unroll
          for (int r = 0; r < 4; ++r) b[r] = rel[min(max(dist - (t * 16 + r), -R), R) + R];
          c += b;
        }
        if (!INIT && t == nvis - 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r >= room) c[r] = -INFINITY;
        }
      }
      s[t] = c;
    }
  }

  // the maximum of the query's walked scores.  Key k0 is visible to every query that walks the block: the maximum is finite
  static __device__ __forceinline__ float block_max(const float4v (&s)[SEQ_NT], int nvis) {
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < SEQ_NT; ++t)
      if (t < nvis) m = fmaxf(fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])), m);
    m = fmaxf(m, __shfl_xor(m, 16));
    return fmaxf(m, __shfl_xor(m, 32));
  }

  // s -> exp2(s - m); returns the lane's partial sum (the four lane groups of a query hold a quarter of its keys each)
  static __device__ __forceinline__ float exp_sum(float4v (&s)[SEQ_NT], int nvis, float m) {
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < SEQ_NT; ++t) {
      float4v e = s[t];
      if (t < nvis) {
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r] = __builtin_amdgcn_exp2f(e[r] - m);
        l += (e[0] + e[1]) + (e[2] + e[3]);
      }
      s[t] = e;
    }
    return l;
  }

  // O^T += V^T P^T: o[dt][r] = output d = 16 dt + 4 g + r of query n
  static __device__ __forceinline__ void pv(const T* Vs, const float4v (&s)[SEQ_NT], int nvis, int g, int n, float4v (&o)[NDT]) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int t0 = 0; t0 < SEQ_NT; t0 += 2)
        if (t0 < nvis) {
          // k index of the step: element j of lane group g is key 16 (t0 + (j >> 2)) + 4 g + (j & 3), in both operands
          half8 b;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            b[r] = (_Float16)s[t0][r];
            b[4 + r] = t0 + 1 < nvis ? (_Float16)s[t0 + 1][r] : (_Float16)0.f;
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
      for (int t = 0; t < SEQ_NT; ++t)
        if (t < nvis) {
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const float4v a = *(const float4v*)&Vs[L::v(dt * 16 + n, t * 16 + 4 * g)];
            X::mma(a, s[t], o[dt]);
          }
        }
    }
  }

  // ---- the same steps over the tiles tlo <= t < thi of the block (uniform across the wave), for a band of keys (attn_window)
  // S^T of those tiles; the others are zeros and are not computed.  Key 16 t + 4 g + r of the block is the lane's to see when
  // lo <= it <= hi (the query's band, counted from the block's first key); a tile inside [ilo, ihi], the band every query of
  // the wave shares, needs no mask.  A masked score is a select on the product: the keys below the band are rows of the text
  static __device__ __forceinline__ void scores_band(const T* Ks, const chunk_t (&qf)[NKS], int tlo, int thi, int lo, int hi, int ilo,
                                                     int ihi, int g, int n, float4v (&s)[SEQ_NT]) {
    const int lo4 = lo - 4 * g, hi4 = hi - 4 * g;
#pragma unroll
    for (int t = 0; t < SEQ_NT; ++t) {
      float4v c = {0.f, 0.f, 0.f, 0.f};
      if (t >= tlo && t < thi) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const chunk_t a = *(const chunk_t*)&Ks[L::k(t * 16 + n, ks * 4 * E + g * E)];
          X::mma(a, qf[ks], c);
        }
        if (t * 16 < ilo || t * 16 + 15 > ihi) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (t * 16 + r < lo4 || t * 16 + r > hi4) c[r] = -INFINITY;
        }
      }
      s[t] = c;
    }
  }

  // the maximum of the walked scores: -inf for a query that sees none of them
  static __device__ __forceinline__ float block_max_band(const float4v (&s)[SEQ_NT], int tlo, int thi) {
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < SEQ_NT; ++t)
      if (t >= tlo && t < thi) m = fmaxf(fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])), m);
    m = fmaxf(m, __shfl_xor(m, 16));
    return fmaxf(m, __shfl_xor(m, 32));
  }

  // s -> exp2(s - m) on the walked tiles (m finite); the others stay zeros
  static __device__ __forceinline__ float exp_sum_band(float4v (&s)[SEQ_NT], int tlo, int thi, float m) {
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < SEQ_NT; ++t) {
      float4v e = s[t];
      if (t >= tlo && t < thi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r] = __builtin_amdgcn_exp2f(e[r] - m);
        l += (e[0] + e[1]) + (e[2] + e[3]);
      }
      s[t] = e;
    }
    return l;
  }

  // O^T += V^T P^T over the walked tiles; f16: a 32-key step with one walked tile takes the other's probabilities as the zeros
  // they are (both tiles are staged: staged() rounds up to the step)
  static __device__ __forceinline__ void pv_band(const T* Vs, const float4v (&s)[SEQ_NT], int tlo, int thi, int g, int n, float4v (&o)[NDT]) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int t0 = 0; t0 < SEQ_NT; t0 += 2)
        if (t0 + 1 >= tlo && t0 < thi) {
          half8 b;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            b[r] = (_Float16)s[t0][r];
            b[4 + r] = (_Float16)s[t0 + 1][r];
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
      for (int t = 0; t < SEQ_NT; ++t)
        if (t >= tlo && t < thi) {
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const float4v a = *(const float4v*)&Vs[L::v(dt * 16 + n, t * 16 + 4 * g)];
            X::mma(a, s[t], o[dt]);
          }
        }
    }
  }

  // out[query][head] = o * inv, for the queries that are rows of the sequence
  static __device__ __forceinline__ void store(const SeqArgs<T>& p, int head, size_t row0, int query, int g, const float4v (&o)[NDT], float inv) {
    if (query >= p.npad) return;
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
};

template <typename T, int HD, bool CAUSAL, bool REL>
__global__ __launch_bounds__(SEQ_THREADS) void attn_seq_rows_kernel(SeqRelArgs<T, REL> p) {
  static_assert(!(CAUSAL && REL), "the causal instances take no table");
  typedef Seq<T, HD> S;
  __shared__ __attribute__((aligned(16))) T Ks[S::L::KSZ];
  __shared__ __attribute__((aligned(16))) T Vs[S::L::VSZ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, n = lane & 15;
  const int head = blockIdx.x % p.heads, seq = blockIdx.x / p.heads;
  const int npad = p.npad;
  const size_t row0 = (size_t)seq * npad;
  // the host entries have checked the lengths; the clamp keeps a stray value inside the LDS images
  const int len = CAUSAL ? npad : min(max(p.len[seq], 1), npad);
  const int nkt = (len + 15) >> 4;        // key tiles of this sequence
  S::template stage<!CAUSAL>(p, Ks, Vs, head, row0, 0, len, S::staged(nkt));
  __syncthreads();

  const bool alibi = !CAUSAL && p.slope;
  const float slope = alibi ? p.slope[head] : 0.f;
  const float* rel = nullptr;
  int rel_r = 0;
  if constexpr (REL) {
    rel_r = p.rel_r;
    rel = p.rel + (size_t)head * (2 * rel_r + 1);
  }
  const int ntiles = (npad + 15) >> 4;
  for (int qt = wave; qt < ntiles; qt += 4) {
    const int query = qt * 16 + n;
    // causal: in tile qt, 4 g + r > n is exactly key >= query + 1
    const int nvis = CAUSAL ? qt + 1 : nkt, limit = CAUSAL ? query + 1 : len;
    typename S::chunk_t qf[S::NKS];
    S::load_q(p, head, row0, query, g, qf);
    float4v s[SEQ_NT];
    S::template scores<!CAUSAL, REL>(Ks, qf, alibi, slope, rel, rel_r, query, 0, nvis, limit, g, n, s);
    const float m = S::block_max(s, nvis);
    float l = S::exp_sum(s, nvis, m);
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    float4v o[S::NDT];
#pragma unroll
    for (int dt = 0; dt < S::NDT; ++dt) o[dt] = (float4v){0.f, 0.f, 0.f, 0.f};
    S::pv(Vs, s, nvis, g, n, o);
    S::store(p, head, row0, query, g, o, 1.f / l);
  }
}

// attn_long: the same attention for sequences past SEQ_MAXK keys.  One workgroup = one (sequence, head, block of 64 queries), a
// 16-query tile a wave; the keys arrive in blocks of SEQ_MAXK, 0 .. ceil(len / SEQ_MAXK) - 1 in that order, each staged into the
// same LDS images and walked as attn_short walks its key tiles (ALiBi from the absolute key index, the -inf select in the
// block's last tile; the table's term from the same index, so a block farther than R away adds one value), then folded into the
// running state of the online soft-max:
//   m' = max(m, block max)   alpha = exp2(m - m')   l = l alpha + sum p   o = o alpha, then the block's second product
// and o / l at the end.  The first key of every walked block is a key of the sequence, so no block maximum is -inf; alpha of the
// first block is exp2(-inf) = 0 on o = l = 0.  The walk is a function of len alone.  A query block that starts at or past len
// writes zeros and leaves before any barrier.  m, alpha, l and o are fp32 in both modes; l is kept as the lane's partial sum (the
// four lane groups of a query share m and alpha) and reduced once at the end.  One buffer, two barriers a block.
template <typename T, int HD, bool REL>
__global__ __launch_bounds__(SEQ_THREADS) void attn_seq_stream_kernel(SeqRelArgs<T, REL> p) {
  typedef Seq<T, HD> S;
  __shared__ __attribute__((aligned(16))) T Ks[S::L::KSZ];
  __shared__ __attribute__((aligned(16))) T Vs[S::L::VSZ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, n = lane & 15;
  const int head = blockIdx.x % p.heads, seq = blockIdx.x / p.heads;
  const int npad = p.npad;
  const size_t row0 = (size_t)seq * npad;
  const int len = min(max(p.len[seq], 1), npad);
  const int q0 = blockIdx.y * SEQ_QB;
  const int query = q0 + wave * 16 + n;
  float m = -INFINITY, l = 0.f;
  float4v o[S::NDT];
#pragma unroll
  for (int dt = 0; dt < S::NDT; ++dt) o[dt] = (float4v){0.f, 0.f, 0.f, 0.f};
  if (q0 >= len) {      // uniform over the workgroup: nobody reads these rows, they are written as zeros
    S::store(p, head, row0, query, g, o, 1.f);
    return;
  }
  typename S::chunk_t qf[S::NKS];
  S::load_q(p, head, row0, query, g, qf);
  const bool alibi = p.slope != nullptr;
  const float slope = alibi ? p.slope[head] : 0.f;
  const float* rel = nullptr;
  int rel_r = 0;
  if constexpr (REL) {
    rel_r = p.rel_r;
    rel = p.rel + (size_t)head * (2 * rel_r + 1);
  }

  const int nkb = (len + SEQ_MAXK - 1) / SEQ_MAXK;
  for (int kb = 0; kb < nkb; ++kb) {
    const int k0 = kb * SEQ_MAXK;
    const int blen = min(len - k0, SEQ_MAXK);      // keys of this block, >= 1
    const int nkt = (blen + 15) >> 4;
    if (kb) __syncthreads();      // the block before has been read
    S::template stage<true>(p, Ks, Vs, head, row0, k0, blen, S::staged(nkt));
    __syncthreads();
    float4v s[SEQ_NT];
    S::template scores<false, REL>(Ks, qf, alibi, slope, rel, rel_r, query, k0, nkt, blen, g, n, s);
    const float mn = fmaxf(m, S::block_max(s, nkt));
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    l = l * alpha + S::exp_sum(s, nkt, mn);
#pragma unroll
    for (int dt = 0; dt < S::NDT; ++dt) o[dt] = o[dt] * alpha;
    S::pv(Vs, s, nkt, g, n, o);
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  S::store(p, head, row0, query, g, o, 1.f / l);
}

// attn_window: Longformer's attention of the local queries.  Query i of a text of len rows sees key 0 (the one global token, with
// the local k_0, v_0, counted once) and the keys max(1, i - w) .. min(len - 1, i + w).  The workgroup and the steps are attn_long's;
// what differs is data: the walk of a block of 64 queries at q0 starts at max(1, q0 - w) rounded down to 16 (the V^T chunks stay
// 16-byte aligned) and ends at min(len, q0 + 64 + w); a wave skips the key tiles outside the union of its 16 bands, and masks, per
// lane, from below and from above, the tiles that are not inside all of them.  Key 0 is the state the walk starts from:
// m = q_i . k_0, l = 1, o = v_0 — a one-key block without a product — so m is finite for every row and a query that sees no key of
// a block folds it in with alpha = 1 and probabilities exp2(-inf) = 0.  The walk is a function of (q0, w, len) alone: a text's
// rows do not depend on npad or on the batch.  Rows >= len and row 0 are computed like the others, finite; nobody reads them (row 0
// is attn_global_row's).  Head dim 64.
template <typename T>
struct SeqWinArgs : SeqArgs<T> {
  int w;      // one-sided window, 1 .. 512
};

template <typename T, int HD>
__global__ __launch_bounds__(SEQ_THREADS) void attn_seq_window_kernel(SeqWinArgs<T> p) {
  typedef Seq<T, HD> S;
  constexpr int E = S::E;
  __shared__ __attribute__((aligned(16))) T Ks[S::L::KSZ];
  __shared__ __attribute__((aligned(16))) T Vs[S::L::VSZ];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, n = lane & 15;
  const int head = blockIdx.x % p.heads, seq = blockIdx.x / p.heads;
  const int npad = p.npad, w = p.w;
  const size_t row0 = (size_t)seq * npad;
  const int len = min(max(p.len[seq], 1), npad);
  const int q0 = blockIdx.y * SEQ_QB;
  const int qa = q0 + wave * 16, query = qa + n;
  float4v o[S::NDT];
#pragma unroll
  for (int dt = 0; dt < S::NDT; ++dt) o[dt] = (float4v){0.f, 0.f, 0.f, 0.f};
  if (q0 >= len) {      // uniform over the workgroup: nobody reads these rows, they are written as zeros
    S::store(p, head, row0, query, g, o, 1.f);
    return;
  }
  typename S::chunk_t qf[S::NKS];
  S::load_q(p, head, row0, query, g, qf);

  // key 0: the lane group's quarter of q . k_0, summed over the four groups in an order that gives each the same bits
  float m = 0.f;
#pragma unroll
  for (int ks = 0; ks < S::NKS; ++ks) {
    const typename S::chunk_t kc = *(const typename S::chunk_t*)(p.k + row0 * p.ldk + head * HD + ks * 4 * E + g * E);
#pragma unroll
    for (int j = 0; j < E; ++j) m += (float)qf[ks][j] * (float)kc[j];
  }
  m += __shfl_xor(m, 16);
  m += __shfl_xor(m, 32);
  float l = g == 0 ? 1.f : 0.f;      // the lane's partial sum, as in attn_long
#pragma unroll
  for (int dt = 0; dt < S::NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[dt][r] = (float)p.vt[((size_t)head * HD + dt * 16 + 4 * g + r) * p.ldv + row0];

  const int kend = min(len, q0 + SEQ_QB + w);            // one past the last key of the walk
  const int a0 = max(1, q0 - w) & ~15;
  const int lo = max(1, query - w), hi = min(len - 1, query + w);      // the lane's band
  // the wave's: the union of its bands (empty for a tile past the text) and what they share
  const int ulo = max(1, qa - w), uhi = qa < len ? min(len - 1, qa + 15 + w) : -1;
  const int ilo = max(1, qa + 15 - w), ihi = min(len - 1, qa + w);
  for (int k0 = a0; k0 < kend; k0 += SEQ_MAXK) {
    const int blen = min(kend - k0, SEQ_MAXK);      // keys of this block, >= 1, all rows of the text
    const int nkt = (blen + 15) >> 4;
    if (k0 != a0) __syncthreads();      // the block before has been read
    S::template stage<true>(p, Ks, Vs, head, row0, k0, blen, S::staged(nkt));
    __syncthreads();
    const int tlo = max(ulo - k0, 0) >> 4, thi = min(((uhi - k0) >> 4) + 1, nkt);
    if (tlo < thi) {
      float4v s[SEQ_NT];
      S::scores_band(Ks, qf, tlo, thi, lo - k0, hi - k0, ilo - k0, ihi - k0, g, n, s);
      const float mn = fmaxf(m, S::block_max_band(s, tlo, thi));
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      m = mn;
      l = l * alpha + S::exp_sum_band(s, tlo, thi, mn);
#pragma unroll
      for (int dt = 0; dt < S::NDT; ++dt) o[dt] = o[dt] * alpha;
      S::pv_band(Vs, s, tlo, thi, g, n, o);
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  S::store(p, head, row0, query, g, o, 1.f / l);
}

// attn_global_row: Longformer's attention of the global token, query 0 of every text, over all len keys with the global
// projections.  One workgroup = one (text, head); q_g fp32 [64] in the log2 units of the other kernels, k_g | v_g rows of the
// element type.  The keys go by in chunks of 1024 under an online soft-max whose state (m, l, the 64 outputs) is fp32: a thread
// scores a key (its row is 64 contiguous elements), the chunk's maximum and sum are reduced over the workgroup, then thread
// (key group kg, output d) adds p_j v_j[d] over the keys j = kg mod 4.  The order is a function of len alone.  `bias` (fp32, or
// null) is added to the normalised row: b_vg less the b_v that the output projection's folded bias adds to every row
constexpr int GROW_CHUNK = 1024;

template <typename T>
struct GlobalRowArgs {
  const float* qg;       // [seqs][ldq], head h at column h * 64
  const T* k;            // [seqs * npad][ldk]
  const T* v;            // [seqs * npad][ldv]
  const float* bias;     // [heads * 64] or null
  T* out;                // row seq * out_rows of [..][ldo]
  const int* len;
  int ldq, ldk, ldv, ldo, npad, heads;
  long long out_rows;    // rows between two texts' outputs
};

// the workgroup's maximum / sum of v; every thread gets the same bits.  red: [4]
template <bool MAX>
__device__ __forceinline__ float grow_reduce(float v, float* red, int lane, int wave) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const float u = __shfl_xor(v, o);
    v = MAX ? fmaxf(v, u) : v + u;
  }
  __syncthreads();      // red of the reduction before has been read
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename T>
__global__ __launch_bounds__(256) void attn_global_row_kernel(GlobalRowArgs<T> p) {
  typedef Tr<T> X;
  typedef typename X::chunk_t chunk_t;
  constexpr int E = X::E, HD = 64;
  __shared__ float qs[HD];
  __shared__ float sc[GROW_CHUNK];
  __shared__ float red[4];
  __shared__ float part[4][HD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int head = blockIdx.x % p.heads, seq = blockIdx.x / p.heads;
  const size_t row0 = (size_t)seq * p.npad;
  const int len = min(max(p.len[seq], 1), p.npad);
  if (tid < HD) qs[tid] = p.qg[(size_t)seq * p.ldq + head * HD + tid];
  __syncthreads();
  const int kg = wave, d = lane;
  float m = -INFINITY, l = 0.f, acc = 0.f;
  for (int c0 = 0; c0 < len; c0 += GROW_CHUNK) {
    const int cn = min(len - c0, GROW_CHUNK);
    float lm = -INFINITY;
    for (int j = tid; j < cn; j += 256) {
      const T* kr = p.k + (row0 + c0 + j) * p.ldk + head * HD;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < HD / E; ++c) {
        const chunk_t kc = *(const chunk_t*)(kr + c * E);
#pragma unroll
        for (int e = 0; e < E; ++e) s += qs[c * E + e] * (float)kc[e];
      }
      sc[j] = s;
      lm = fmaxf(lm, s);
    }
    const float mn = fmaxf(m, grow_reduce<true>(lm, red, lane, wave));      // finite: the chunk has a key
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    float ls = 0.f;
    for (int j = tid; j < cn; j += 256) {      // the thread's own scores
      const float e = __builtin_amdgcn_exp2f(sc[j] - mn);
      sc[j] = e;
      ls += e;
    }
    l = l * alpha + grow_reduce<false>(ls, red, lane, wave);      // its barriers publish sc
    acc *= alpha;
    for (int j = kg; j < cn; j += 4) acc += sc[j] * (float)p.v[(row0 + c0 + j) * p.ldv + head * HD + d];
    __syncthreads();      // sc is read before the next chunk's scores
  }
  part[kg][d] = acc;
  __syncthreads();
  if (tid < HD) {
    float r = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) / l;
    if (p.bias) r += p.bias[head * HD + tid];
    p.out[(size_t)seq * p.out_rows * p.ldo + head * HD + tid] = (T)r;
  }
}

enum SeqKind { SEQ_CAUSAL, SEQ_SHORT, SEQ_LONG };

// what the three entries require of an AttnDesc: counts, rows per sequence (a multiple of 8, 8 .. max_rows, the same for queries
// and keys), 16-byte rows and pointers, V^T rows that span the batch
int seq_check(mhip_ctx* ctx, const char* name, int max_rows, int precision, const AttnDesc& d) {
  if (d.images <= 0 || d.heads <= 0 || (long long)d.images * d.heads > 0x7fffffffLL || d.npad_k < 8 || d.npad_k % 8 ||
      d.npad_k > max_rows || d.npad_q != d.npad_k)
    return mhip_fail(ctx, MHIP_EINVAL, "%s: bad shape (%d sequences, %d heads, %d / %d rows: equal, a multiple of 8, 8 .. %d)", name,
                     d.images, d.heads, d.npad_q, d.npad_k, max_rows);
  const int esz = precision == MHIP_PREC_F16 ? 2 : 4;
  if ((d.ldq * esz) % 16 || (d.ldk * esz) % 16 || (d.ldv * esz) % 16 || (d.ldo * esz) % 16 || (long long)d.ldv < (long long)d.images * d.npad_k ||
      ((uintptr_t)d.q & 15) || ((uintptr_t)d.k & 15) || ((uintptr_t)d.vt & 15) || ((uintptr_t)d.out & 15))
    return mhip_fail(ctx, MHIP_EINVAL, "%s: rows must keep 16-byte alignment (ldq, ldk, ldv, ldo, the pointers), ldv the whole batch", name);
  return 0;
}

template <typename T, bool REL>
SeqRelArgs<T, REL> seq_args(const AttnDesc& d, const int* len, const float* slopes, const float* rel, int rel_r) {
  SeqRelArgs<T, REL> a;
  if constexpr (REL) {
    a.rel = rel; a.rel_r = rel_r;
  }
  a.q = (const T*)d.q; a.k = (const T*)d.k; a.vt = (const T*)d.vt; a.out = (T*)d.out;
  a.len = len; a.slope = slopes;
  a.ldq = d.ldq; a.ldk = d.ldk; a.ldv = d.ldv; a.ldo = d.ldo;
  a.npad = d.npad_k; a.heads = d.heads;
  return a;
}

template <typename T, int HD, bool REL>
void seq_launch(mhip_ctx* ctx, SeqKind kind, const AttnDesc& d, const int* len, const float* slopes, const float* rel, int rel_r) {
  const SeqRelArgs<T, REL> a = seq_args<T, REL>(d, len, slopes, rel, rel_r);
  const dim3 rows((unsigned)(d.images * d.heads)), blocks(rows.x, (unsigned)((d.npad_k + SEQ_QB - 1) / SEQ_QB)), threads(SEQ_THREADS);
  if constexpr (HD == 64 && !REL) {      // causal: head dim 64 only; its one caller dispatches with 64, so no kind is left unlaunched
    if (kind == SEQ_CAUSAL) PROF_LAUNCH(ctx, MHIP_K_ATTN_CAUSAL, hipLaunchKernelGGL((attn_seq_rows_kernel<T, 64, true, false>), rows, threads, 0, ctx->stream, a));
  }
  if (kind == SEQ_SHORT) PROF_LAUNCH(ctx, MHIP_K_ATTN_SHORT, hipLaunchKernelGGL((attn_seq_rows_kernel<T, HD, false, REL>), rows, threads, 0, ctx->stream, a));
  // no slot of its own: the profiler's list is pinned, and a call runs one of the two attentions
  if (kind == SEQ_LONG) PROF_LAUNCH(ctx, MHIP_K_ATTN_SHORT, hipLaunchKernelGGL((attn_seq_stream_kernel<T, HD, REL>), blocks, threads, 0, ctx->stream, a));
}

template <bool REL>
void seq_dispatch(mhip_ctx* ctx, int precision, int head_dim, SeqKind kind, const AttnDesc& d, const int* len, const float* slopes,
                  const float* rel = nullptr, int rel_r = 0) {
  if (precision == MHIP_PREC_F16) {
    if (head_dim == 64) seq_launch<_Float16, 64, REL>(ctx, kind, d, len, slopes, rel, rel_r);
    else seq_launch<_Float16, 32, REL>(ctx, kind, d, len, slopes, rel, rel_r);
  } else {
    if (head_dim == 64) seq_launch<float, 64, REL>(ctx, kind, d, len, slopes, rel, rel_r);
    else seq_launch<float, 32, REL>(ctx, kind, d, len, slopes, rel, rel_r);
  }
}

// attn_short and attn_long: the entry's name and row limit, and which kernel
int seq_lengths_entry(mhip_ctx* ctx, const char* name, int max_rows, SeqKind kind, int precision, const AttnShortDesc& s) {
  const AttnDesc& d = s.a;
  if (s.head_dim != 64 && s.head_dim != 32) return mhip_fail(ctx, MHIP_EINVAL, "%s: head_dim %d (64 or 32)", name, s.head_dim);
  if (!s.len) return mhip_fail(ctx, MHIP_EINVAL, "%s: len is null", name);
  if (s.rel_table && s.slopes) return mhip_fail(ctx, MHIP_EINVAL, "%s: slopes and rel_table together (one bias term a call)", name);
  if (s.rel_table && (s.rel_radius < 0 || s.rel_radius > SEQ_MAXROWS))
    return mhip_fail(ctx, MHIP_EINVAL, "%s: rel_radius %d (0 .. %d)", name, s.rel_radius, SEQ_MAXROWS);
  if (const int rc = seq_check(ctx, name, max_rows, precision, d)) return rc;
  // the lengths live on the device: counted as full sequences
  if (ctx->profiling) ctx->prof[MHIP_K_ATTN_SHORT].flops += 4.0 * d.images * d.heads * (double)d.npad_k * d.npad_k * s.head_dim;
  if (s.rel_table) seq_dispatch<true>(ctx, precision, s.head_dim, kind, d, s.len, nullptr, s.rel_table, s.rel_radius);
  else seq_dispatch<false>(ctx, precision, s.head_dim, kind, d, s.len, s.slopes);
  return 0;
}

}  // namespace

int mhip_launch_attention_causal(mhip_ctx* ctx, int precision, const AttnDesc& d) {
  if (const int rc = seq_check(ctx, "attention_causal", SEQ_MAXK, precision, d)) return rc;
  if (d.n_queries != d.n_keys || d.n_keys < 1 || d.n_keys > d.npad_k)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_causal: %d queries, %d keys in %d rows", d.n_queries, d.n_keys, d.npad_k);
  if (ctx->profiling) ctx->prof[MHIP_K_ATTN_CAUSAL].flops += 2.0 * d.images * d.heads * (double)d.n_keys * (d.n_keys + 1) * 64;
  seq_dispatch<false>(ctx, precision, 64, SEQ_CAUSAL, d, nullptr, nullptr);
  CHECK_LAUNCH(ctx, "attention_causal");
  return 0;
}

int mhip_launch_attention_short(mhip_ctx* ctx, int precision, const AttnShortDesc& s) {
  if (const int rc = seq_lengths_entry(ctx, "attention_short", SEQ_MAXK, SEQ_SHORT, precision, s)) return rc;
  CHECK_LAUNCH(ctx, "attention_short");
  return 0;
}

int mhip_launch_attention_long(mhip_ctx* ctx, int precision, const AttnShortDesc& s) {
  if (const int rc = seq_lengths_entry(ctx, "attention_long", SEQ_MAXROWS, SEQ_LONG, precision, s)) return rc;
  CHECK_LAUNCH(ctx, "attention_long");
  return 0;
}

int mhip_launch_attention_window(mhip_ctx* ctx, int precision, const AttnShortDesc& s, int w) {
  const AttnDesc& d = s.a;
  if (s.head_dim != 64) return mhip_fail(ctx, MHIP_EINVAL, "attention_window: head_dim %d (64)", s.head_dim);
  if (!s.len) return mhip_fail(ctx, MHIP_EINVAL, "attention_window: len is null");
  if (s.slopes || s.rel_table) return mhip_fail(ctx, MHIP_EINVAL, "attention_window: no bias term (slopes, rel_table)");
  if (w < 1 || w > ATTN_WINDOW_MAX) return mhip_fail(ctx, MHIP_EINVAL, "attention_window: w %d (one-sided, 1 .. %d)", w, ATTN_WINDOW_MAX);
  if (const int rc = seq_check(ctx, "attention_window", SEQ_MAXROWS, precision, d)) return rc;
  // the lengths live on the device: counted as full bands of full sequences
  if (ctx->profiling) ctx->prof[MHIP_K_ATTN_SHORT].flops += 4.0 * d.images * d.heads * (double)d.npad_k * std::min(2 * w + 2, d.npad_k) * 64;
  const dim3 blocks((unsigned)(d.images * d.heads), (unsigned)((d.npad_k + SEQ_QB - 1) / SEQ_QB)), threads(SEQ_THREADS);
  // counted with the other per-sequence attentions: the profiler's list is pinned, and a call runs one of them
  if (precision == MHIP_PREC_F16) {
    SeqWinArgs<_Float16> a;
    (SeqArgs<_Float16>&)a = seq_args<_Float16, false>(d, s.len, nullptr, nullptr, 0);
    a.w = w;
    PROF_LAUNCH(ctx, MHIP_K_ATTN_SHORT, hipLaunchKernelGGL((attn_seq_window_kernel<_Float16, 64>), blocks, threads, 0, ctx->stream, a));
  } else {
    SeqWinArgs<float> a;
    (SeqArgs<float>&)a = seq_args<float, false>(d, s.len, nullptr, nullptr, 0);
    a.w = w;
    PROF_LAUNCH(ctx, MHIP_K_ATTN_SHORT, hipLaunchKernelGGL((attn_seq_window_kernel<float, 64>), blocks, threads, 0, ctx->stream, a));
  }
  CHECK_LAUNCH(ctx, "attention_window");
  return 0;
}

int mhip_launch_attention_global_row(mhip_ctx* ctx, int precision, const AttnGlobalRowDesc& d) {
  if (!d.qg || !d.k || !d.v || !d.out || !d.len) return mhip_fail(ctx, MHIP_EINVAL, "attention_global_row: null operand");
  if (d.seqs <= 0 || d.heads <= 0 || (long long)d.seqs * d.heads > 0x7fffffffLL || d.npad < 8 || d.npad % 8 || d.npad > SEQ_MAXROWS || d.out_rows < 1)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_global_row: bad shape (%d sequences, %d heads, %d rows: a multiple of 8, 8 .. %d)", d.seqs, d.heads,
                     d.npad, SEQ_MAXROWS);
  const int esz = precision == MHIP_PREC_F16 ? 2 : 4;
  if ((d.ldk * esz) % 16 || ((uintptr_t)d.k & 15) || d.ldk < d.heads * 64 || d.ldv < d.heads * 64 || d.ldq < d.heads * 64 || d.ldo < d.heads * 64)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_global_row: key rows must keep 16-byte alignment, every pitch hold heads * 64 columns");
  if (ctx->profiling) ctx->prof[MHIP_K_ATTN_SHORT].flops += 4.0 * d.seqs * d.heads * (double)d.npad * 64;
  const dim3 blocks((unsigned)(d.seqs * d.heads)), threads(256);
  auto args = [&](auto* t) {
    typedef std::remove_pointer_t<decltype(t)> T;
    GlobalRowArgs<T> a;
    a.qg = d.qg; a.k = (const T*)d.k; a.v = (const T*)d.v; a.bias = d.bias; a.out = (T*)d.out; a.len = d.len;
    a.ldq = d.ldq; a.ldk = d.ldk; a.ldv = d.ldv; a.ldo = d.ldo; a.npad = d.npad; a.heads = d.heads; a.out_rows = d.out_rows;
    return a;
  };
  if (precision == MHIP_PREC_F16) PROF_LAUNCH(ctx, MHIP_K_ATTN_SHORT, hipLaunchKernelGGL(attn_global_row_kernel<_Float16>, blocks, threads, 0, ctx->stream, args((_Float16*)nullptr)));
  else PROF_LAUNCH(ctx, MHIP_K_ATTN_SHORT, hipLaunchKernelGGL(attn_global_row_kernel<float>, blocks, threads, 0, ctx->stream, args((float*)nullptr)));
  CHECK_LAUNCH(ctx, "attention_global_row");
  return 0;
}
