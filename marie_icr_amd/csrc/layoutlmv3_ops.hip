// layoutlmv3_ops.hip — the pieces of LayoutLMv3 the ViT / TrOCR paths do not have: attention with a learned relative-position
// bias and a padding mask, the text + layout embedding gather, and the classification head.
//
// Replaces, in transformers/models/layoutlmv3/modeling_layoutlmv3.py: LayoutLMv3SelfAttention.forward's scores + (rel_pos +
// rel_2d_pos) / sqrt(d) + mask -> softmax -> @ v, LayoutLMv3Encoder._cal_1d_pos_emb / _cal_2d_pos_emb (never materialised: see
// below), LayoutLMv3TextEmbeddings.forward, the LayerNorms of LayoutLMv3Model.forward / forward_image, and
// LayoutLMv3ClassificationHead.forward.
//
// The bias of a score depends on (i, j) only through three integer differences, p_j - p_i, x0_j - x0_i, y1_j - y1_i, so
// per head three difference-indexed tables replace the [heads][n][n] tensors the library builds (3 x 24 MB a page): they are
// folded with the head weights and the score scale once (mhip_attn_bias_fold), live in LDS beside the K / V^T tiles
// (22.0 KB at 512 text rows and a 1024 grid), and each score takes three ds_read_b32 from per-token codes.
//
// attn_bias_f16_kernel is attn_flash_f16_kernel (vit_ops.hip) — same 128-query block, 64-key tile, transposed MFMA 16x16x32
// products, stale-reference soft-max in base 2 — with the look-ups between S^T and the tile maximum.  It is a kernel of its own
// so that the ViT path keeps the code it had.
#include <algorithm>

#include "igemm_common.h"

using namespace igemm;

namespace {

constexpr int HD = 64;

struct AttnArgs {
  const char* q;
  const char* k;
  const char* vt;
  char* out;
  int ldq, ldk, ldv, ldo;
  int npad_q, npad_k;
  int n_keys;
  int heads, nqb;
};
struct BiasArgs {
  const uint32_t* qcode;
  const uint32_t* kcode;
  const float* tab;
  int dp, dx, tab_len;
};

constexpr int AT_THREADS = 256, AT_QB = 128, AT_KT = 64;
constexpr int AT_TILE = AT_KT * 128;
constexpr int AT_STAGE = 2 * AT_TILE, AT_NSTAGE = 2;
constexpr int AT_TAB = AT_NSTAGE * AT_STAGE;      // byte offset of the bias tables in LDS

__global__ __launch_bounds__(AT_THREADS) void attn_bias_f16_kernel(AttnArgs p, BiasArgs bp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  int qb, hb;
  {
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
    const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    qb = L % p.nqb;
    hb = L / p.nqb;
  }
  const int h = hb % p.heads, img = hb / p.heads;
  const size_t qrow0 = (size_t)img * p.npad_q + (size_t)qb * AT_QB + wave * 32;
  const size_t krow0 = (size_t)img * p.npad_k;

  // this head's tables -> LDS (visible after the first barrier of the tile loop)
  {
    const float* src = bp.tab + (size_t)h * bp.tab_len;
    float* dst = (float*)(smem + AT_TAB);
    for (int e = tid; e < bp.tab_len; e += AT_THREADS) dst[e] = src[e];
  }
  // byte offsets into the tables that the key fields are added to: (table start + range - own field) * 4
  int b1[2], bx[2], by[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const uint32_t c = bp.qcode[qrow0 + qt * 16 + n];
    const int off_x = 3 * bp.dp + 2, off_y = off_x + 2 * bp.dx + 1;
    b1[qt] = AT_TAB + (bp.dp - (int)(c & 0xfff)) * 4;
    bx[qt] = AT_TAB + (off_x + bp.dx - (int)((c >> 12) & 0x3ff)) * 4;
    by[qt] = AT_TAB + (off_y + bp.dx - (int)(c >> 22)) * 4;
  }
  const uint32_t* kc = bp.kcode + krow0 + 8 * g;

  half8 qreg[2][2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      qreg[qt][ks] = *(const half8*)(p.q + ((qrow0 + qt * 16 + n) * p.ldq + h * HD + ks * 32 + g * 8) * 2);

  const char* ksrc[2];
  const char* vsrc[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int R = (q * 4 + wave) * 8 + (lane >> 3);
    const int lc = (lane & 7) ^ ((R >> 1) & 7);
    const int kt = R >> 4, i = R & 15;
    const int key = 32 * (kt >> 1) + 8 * (i >> 2) + 4 * (kt & 1) + (i & 3);
    ksrc[q] = p.k + ((krow0 + key) * p.ldk + h * HD + lc * 8) * 2;
    vsrc[q] = p.vt + (((size_t)h * HD + R) * p.ldv + krow0 + lc * 8) * 2;
  }
  const size_t kstep = (size_t)AT_KT * p.ldk * 2;
  auto stage = [&](int slot) {
    char* la = smem + slot * AT_STAGE + wave * 1024;
#pragma unroll
    for (int q = 0; q < 2; ++q) { glds16(ksrc[q], la + q * 4096); ksrc[q] += kstep; }
#pragma unroll
    for (int q = 0; q < 2; ++q) { glds16(vsrc[q], la + AT_TILE + q * 4096); vsrc[q] += AT_KT * 2; }
  };

  float4v acc_o[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc_o[i][j] = (float4v){0.f, 0.f, 0.f, 0.f};
  constexpr float RESCALE_AT = 8.f;
  float4v negm[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const half8 ones = n == 0 ? (half8){1, 1, 1, 1, 1, 1, 1, 1} : (half8){0, 0, 0, 0, 0, 0, 0, 0};
  float4v acc_l[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};

  int foff[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int R = t * 16 + n;
    foff[t] = R * 128 + ((g ^ ((R >> 1) & 7)) << 4);
  }

  const int ntiles = (p.n_keys + AT_KT - 1) / AT_KT;
  stage(0);
  int slot = 0, fill = 1;
  for (int t = 0; t < ntiles; ++t) {
    // codes of this lane's 16 keys of the tile: kt -> keys 32 (kt >> 1) + 8 g + 4 (kt & 1) + r, r = 0..3 in one 16-byte load
    uint4v kcode[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) kcode[kt] = *(const uint4v*)(kc + t * AT_KT + 32 * (kt >> 1) + 4 * (kt & 1));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 1 < ntiles) stage(fill);
    const char* sk = smem + slot * AT_STAGE;
    const char* sv = sk + AT_TILE;

    float4v s[4][2];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt][0] = negm[0];
      s[kt][1] = negm[1];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const half8 a = *(const half8*)(sk + (foff[kt] ^ (ks << 6)));
        s[kt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qreg[0][ks], s[kt][0], 0, 0, 0);
        s[kt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qreg[1][ks], s[kt][1], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    // ---- relative-position bias and key mask: three LDS look-ups per score -------------------------------------
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t c = kcode[kt][r];
        const int kp = (int)(c & 0xfff) << 2, kx = (int)((c >> 10) & 0xffc), ky = (int)((c >> 20) & 0xffc);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
          s[kt][qt][r] += (*(const float*)(smem + kp + b1[qt]) + *(const float*)(smem + kx + bx[qt])) +
                          *(const float*)(smem + ky + by[qt]);
      }
    if ((t + 1) * AT_KT > p.n_keys) {
      const int kbase = t * AT_KT;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kbase + 32 * (kt >> 1) + 8 * g + 4 * (kt & 1) + r;
          if (key >= p.n_keys) { s[kt][0][r] = -INFINITY; s[kt][1][r] = -INFINITY; }
        }
    }
    half8 pb[2][2];
    float tmax[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][qt][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      tmax[qt] = mx;
    }
    const bool move = t == 0 || tmax[0] > RESCALE_AT || tmax[1] > RESCALE_AT;
    if (__builtin_amdgcn_ballot_w64(move) != 0) {
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const float d = t == 0 ? tmax[qt] : (tmax[qt] > RESCALE_AT ? tmax[qt] : 0.f);
        const float alpha = t == 0 ? 0.f : __builtin_amdgcn_exp2f(-d);
        negm[qt] -= (float4v){d, d, d, d};
        acc_l[qt] *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) acc_o[dt][qt] *= alpha;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) s[kt][qt] -= (float4v){d, d, d, d};
      }
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) pb[qt][kt >> 1][(kt & 1) * 4 + r] = (_Float16)__builtin_amdgcn_exp2f(s[kt][qt][r]);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const half8 a = *(const half8*)(sv + (foff[dt] ^ (c << 6)));
        acc_o[dt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pb[0][c], acc_o[dt][0], 0, 0, 0);
        acc_o[dt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pb[1][c], acc_o[dt][1], 0, 0, 0);
      }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      acc_l[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pb[0][c], acc_l[0], 0, 0, 0);
      acc_l[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pb[1][c], acc_l[1], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    slot = slot == AT_NSTAGE - 1 ? 0 : slot + 1;
    fill = fill == AT_NSTAGE - 1 ? 0 : fill + 1;
  }
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const float inv = 1.f / __shfl(acc_l[qt][0], n);
    if (qb * AT_QB + wave * 32 + qt * 16 + n >= p.npad_q) continue;
    char* orow = p.out + ((qrow0 + qt * 16 + n) * p.ldo + h * HD) * 2;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      _Float16 o4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) o4[r] = (_Float16)(acc_o[dt][qt][r] * inv);
      *(uint64_t*)(orow + (dt * 16 + g * 4) * 2) = *(uint64_t*)o4;
    }
  }
}

// fp32 parity mode: one wave per query, lane = key stripe, tables read from HBM (L2-resident); a masked key is skipped, so
// its probability is exactly 0 as the library's finfo.min mask makes it.
__global__ __launch_bounds__(256) void attn_bias_simple_f32_kernel(AttnArgs p, BiasArgs bp, int n_queries) {
  const int lane = threadIdx.x & 63;
  const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int h = blockIdx.y, img = blockIdx.z;
  if (qi >= n_queries) return;
  const float* Q = (const float*)p.q + ((size_t)img * p.npad_q + qi) * p.ldq + h * HD;
  const float* K = (const float*)p.k + (size_t)img * p.npad_k * p.ldk + h * HD;
  const float* VT = (const float*)p.vt + (size_t)h * HD * p.ldv + (size_t)img * p.npad_k;
  const uint32_t qc = bp.qcode[(size_t)img * p.npad_q + qi];
  const uint32_t* KC = bp.kcode + (size_t)img * p.npad_k;
  const int off_x = 3 * bp.dp + 2, off_y = off_x + 2 * bp.dx + 1;
  const float* T1 = bp.tab + (size_t)h * bp.tab_len + bp.dp - (int)(qc & 0xfff);
  const float* TX = bp.tab + (size_t)h * bp.tab_len + off_x + bp.dx - (int)((qc >> 12) & 0x3ff);
  const float* TY = bp.tab + (size_t)h * bp.tab_len + off_y + bp.dx - (int)(qc >> 22);
  float q[HD], o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) { q[d] = Q[d]; o[d] = 0.f; }
  float m = -INFINITY, l = 0.f;
  for (int key = lane; key < p.n_keys; key += 64) {
    const uint32_t c = KC[key];
    const int kp = (int)(c & 0xfff);
    if (kp > 2 * bp.dp) continue;
    const float* kr = K + (size_t)key * p.ldk;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) s += q[d] * kr[d];
    s += (T1[kp] + TX[(c >> 12) & 0x3ff]) + TY[c >> 22];
    const float mx = fmaxf(m, s);
    const float alpha = exp2f(m - mx), e = exp2f(s - mx);
    l = l * alpha + e;
#pragma unroll
    for (int d = 0; d < HD; ++d) o[d] = o[d] * alpha + e * VT[(size_t)d * p.ldv + key];
    m = mx;
  }
  float M = m;
#pragma unroll
  for (int off = 32; off; off >>= 1) M = fmaxf(M, __shfl_xor(M, off));
  const float f = (m == -INFINITY) ? 0.f : exp2f(m - M);
  l *= f;
#pragma unroll
  for (int off = 32; off; off >>= 1) l += __shfl_xor(l, off);
  float* out = (float*)p.out + ((size_t)img * p.npad_q + qi) * p.ldo + h * HD;
#pragma unroll
  for (int d = 0; d < HD; ++d) {
    float v = o[d] * f;
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    if (lane == (d & 63)) out[d] = v / l;
  }
}

// ------------------------------------------------------------------------------------------------------- embeddings
// LayerNorm of the row a wave holds (nv float4 groups per lane), two-pass in registers
__device__ __forceinline__ void wave_layernorm(float4v v[4], int nv, int D, int lane, const float* __restrict__ g,
                                               const float* __restrict__ b, float eps) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
#pragma unroll
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv)
#pragma unroll
      for (int k = 0; k < 4; ++k) { const float d = v[i][k] - mean; q += d * d; }
#pragma unroll
  for (int o = 32; o; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = 1.f / sqrtf(q / (float)D + eps);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv) {
      const int c = (i * 64 + lane) * 4;
      const float4v gg = *(const float4v*)(g + c), bb = *(const float4v*)(b + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[i][k] = (v[i][k] - mean) * rstd * gg[k] + bb[k];
    }
}

struct EmbedArgs {
  const int* tok;
  const void* word;
  const float *type0, *pos, *xe, *ye, *he, *we, *g_text, *b_text, *patches, *cls, *g_vis, *b_vis, *g_all, *b_all;
  float* h;
  void* ht;
  int rows, max_text, n_vis, npad, D, coord, shape;
  float eps, eps_vis;
};

// one wave per row of the sequence: text rows gather word + token type + position + the six layout embeddings and take the
// embeddings' LayerNorm, visual rows take the patch projection (or the cls row) and `norm`; both then take the model's
// LayerNorm over the concatenated sequence.  Rows past the sequence (npad) are zeros.
template <typename T>
__global__ __launch_bounds__(256) void lmv3_embed_kernel(EmbedArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  const int page = row / a.npad, t = row % a.npad;
  const int D = a.D, nv = D >> 8;
  float4v v[4];
  if (t < a.max_text) {
    const int* tk = a.tok + ((size_t)page * a.max_text + t) * 8;
    const int id = tk[0], pid = tk[1];
    const int c4 = 4 * a.coord;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nv) {
        const int c = (i * 64 + lane) * 4;
        float4v w;
        if (sizeof(T) == 2) {
          typedef _Float16 half4 __attribute__((ext_vector_type(4)));
          const half4 hw = *(const half4*)((const _Float16*)a.word + (size_t)id * D + c);
          w = (float4v){(float)hw[0], (float)hw[1], (float)hw[2], (float)hw[3]};
        } else {
          w = *(const float4v*)((const float*)a.word + (size_t)id * D + c);
        }
        // segment of the concatenated layout embedding this group of four columns lies in
        const float* sp;
        if (c < c4) {
          const int seg = c / a.coord, cc = c - seg * a.coord;
          sp = ((seg & 1) ? a.ye : a.xe) + (size_t)tk[2 + seg] * a.coord + cc;
        } else {
          const int seg = (c - c4) / a.shape, cc = c - c4 - seg * a.shape;
          sp = (seg ? a.we : a.he) + (size_t)tk[6 + seg] * a.shape + cc;
        }
        v[i] = ((w + *(const float4v*)(a.type0 + c)) + *(const float4v*)(a.pos + (size_t)pid * D + c)) + *(const float4v*)sp;
      }
    wave_layernorm(v, nv, D, lane, a.g_text, a.b_text, a.eps);
  } else if (t < a.max_text + a.n_vis) {
    const int vi = t - a.max_text;
    const float* src = vi == 0 ? a.cls : a.patches + ((size_t)page * (a.n_vis - 1) + vi - 1) * D;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nv) v[i] = *(const float4v*)(src + (i * 64 + lane) * 4);
    wave_layernorm(v, nv, D, lane, a.g_vis, a.b_vis, a.eps_vis);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float4v){0.f, 0.f, 0.f, 0.f};
  }
  if (t < a.max_text + a.n_vis) wave_layernorm(v, nv, D, lane, a.g_all, a.b_all, a.eps);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv) {
      const size_t o = (size_t)row * D + (i * 64 + lane) * 4;
      *(float4v*)(a.h + o) = v[i];
      T o4[4] = {(T)v[i][0], (T)v[i][1], (T)v[i][2], (T)v[i][3]};
      if (sizeof(T) == 2) *(uint64_t*)((T*)a.ht + o) = *(uint64_t*)o4;
      else *(float4v*)((T*)a.ht + o) = *(float4v*)o4;
    }
}

// ------------------------------------------------------------------------------------------------------- head
// one workgroup per page: y = tanh(W_d x + b_d) (x = row 0 of the page), logits = W_o y + b_o.  A wave per output, lanes along k.
__global__ __launch_bounds__(256) void lmv3_head_kernel(const float* __restrict__ h, int npad, int D, const float* __restrict__ dw,
                                                        const float* __restrict__ db, const float* __restrict__ ow,
                                                        const float* __restrict__ ob, int labels, float* __restrict__ logits) {
  __shared__ float xs[1024], ys[1024];
  const int page = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = h + (size_t)page * npad * D;
  for (int d = threadIdx.x; d < D; d += 256) xs[d] = x[d];
  __syncthreads();
  for (int j = wave; j < D; j += 4) {
    float acc = 0.f;
    for (int k = lane; k < D; k += 64) acc += dw[(size_t)j * D + k] * xs[k];
#pragma unroll
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) ys[j] = tanhf(acc + db[j]);
  }
  __syncthreads();
  for (int j = wave; j < labels; j += 4) {
    float acc = 0.f;
    for (int k = lane; k < D; k += 64) acc += ow[(size_t)j * D + k] * ys[k];
#pragma unroll
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) logits[(size_t)page * labels + j] = acc + ob[j];
  }
}

}  // namespace

#define CHECK_LAUNCH(ctx, what)                                                                              \
  do {                                                                                                       \
    hipError_t _e = hipGetLastError();                                                                       \
    if (_e != hipSuccess) return mhip_fail((ctx), MHIP_EHIP, what " launch: %s", hipGetErrorString(_e));    \
  } while (0)

// LayoutLMv3Encoder.relative_position_bucket(bidirectional=True) of one difference.  The logarithmic half is evaluated in
// float32, operation by operation as the library's tensor expression is: its truncation decides the bucket borders.
int mhip_relative_position_bucket(int relative_position, int num_buckets, int max_distance) {
  int ret = 0;
  num_buckets /= 2;
  if (relative_position > 0) ret += num_buckets;
  const int n = relative_position < 0 ? -relative_position : relative_position;
  const int max_exact = num_buckets / 2;
  if (n < max_exact) return ret + n;
  volatile float v = logf((float)n / (float)max_exact);
  v = v / (float)log((double)max_distance / (double)max_exact);
  v = v * (float)(num_buckets - max_exact);
  int large = max_exact + (int)v;
  if (large > num_buckets - 1) large = num_buckets - 1;
  return ret + large;
}

void mhip_attn_bias_fold(const float* w1, const float* wx, const float* wy, int heads, int bins_1d, int max_1d, int bins_2d,
                         int max_2d, int dp, int dx, float scale, float* tab) {
  const int len = mhip_attn_bias_table_len(dp, dx), off_x = 3 * dp + 2, off_y = off_x + 2 * dx + 1;
  std::vector<int> b1(2 * dp + 1), b2(2 * dx + 1);
  for (int i = 0; i <= 2 * dp; ++i) b1[i] = mhip_relative_position_bucket(i - dp, bins_1d, max_1d);
  for (int i = 0; i <= 2 * dx; ++i) b2[i] = mhip_relative_position_bucket(i - dx, bins_2d, max_2d);
  for (int h = 0; h < heads; ++h) {
    float* t = tab + (size_t)h * len;
    for (int i = 0; i <= 2 * dp; ++i) t[i] = w1[h * bins_1d + b1[i]] * scale;
    for (int i = 2 * dp + 1; i < off_x; ++i) t[i] = MHIP_ATTN_MASKED;
    for (int i = 0; i <= 2 * dx; ++i) {
      t[off_x + i] = wx[h * bins_2d + b2[i]] * scale;
      t[off_y + i] = wy[h * bins_2d + b2[i]] * scale;
    }
  }
}

int mhip_launch_attention_bias(mhip_ctx* ctx, int precision, const AttnBiasDesc& bd) {
  const AttnDesc& d = bd.a;
  if (d.images <= 0 || d.heads <= 0 || d.n_keys <= 0 || d.n_queries <= 0 || d.npad_k % 8 || d.n_queries > d.npad_q ||
      d.n_keys > d.npad_k)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_bias: bad shape (q %d/%d, k %d/%d)", d.n_queries, d.npad_q, d.n_keys, d.npad_k);
  if (!bd.qcode || !bd.kcode || !bd.tab || bd.dp < 0 || bd.dp > 1023 || bd.dx < 0 || bd.dx > 1023 || ((uintptr_t)bd.kcode & 15))
    return mhip_fail(ctx, MHIP_EINVAL, "attention_bias: bad tables (dp %d, dx %d)", bd.dp, bd.dx);
  const int esz = precision == MHIP_PREC_F16 ? 2 : 4;
  if ((d.ldq * esz) % 16 || (d.ldk * esz) % 16 || (d.ldv * esz) % 16 || (d.ldo * esz) % 8)
    return mhip_fail(ctx, MHIP_EINVAL, "attention_bias: row pitches must keep 16-byte alignment");
  AttnArgs a;
  a.q = (const char*)d.q; a.k = (const char*)d.k; a.vt = (const char*)d.vt; a.out = (char*)d.out;
  a.ldq = d.ldq; a.ldk = d.ldk; a.ldv = d.ldv; a.ldo = d.ldo;
  a.npad_q = d.npad_q; a.npad_k = d.npad_k; a.n_keys = d.n_keys; a.heads = d.heads;
  a.nqb = (d.n_queries + AT_QB - 1) / AT_QB;
  BiasArgs b;
  b.qcode = bd.qcode; b.kcode = bd.kcode; b.tab = bd.tab; b.dp = bd.dp; b.dx = bd.dx;
  b.tab_len = mhip_attn_bias_table_len(bd.dp, bd.dx);
  if (ctx->profiling) ctx->prof[MHIP_K_ATTN_BIAS].flops += mhip_attention_flops(d);
  if (precision == MHIP_PREC_F16) {
    const int lds = AT_TAB + b.tab_len * 4;      // <= 32768 + 28668 bytes
    static std::once_flag attr;
    std::call_once(attr, [&] {
      (void)hipFuncSetAttribute((const void*)attn_bias_f16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    });
    dim3 grid((unsigned)(a.nqb * d.heads * d.images)), block(AT_THREADS);
    PROF_LAUNCH(ctx, MHIP_K_ATTN_BIAS, hipLaunchKernelGGL(attn_bias_f16_kernel, grid, block, lds, ctx->stream, a, b));
  } else {
    dim3 grid((d.n_queries + 3) / 4, d.heads, d.images), block(256);
    PROF_LAUNCH(ctx, MHIP_K_ATTN_BIAS, hipLaunchKernelGGL(attn_bias_simple_f32_kernel, grid, block, 0, ctx->stream, a, b, d.n_queries));
  }
  CHECK_LAUNCH(ctx, "attention_bias");
  return 0;
}

int mhip_launch_lmv3_embed(mhip_ctx* ctx, int precision, const Lmv3EmbedDesc& d) {
  if (d.D % 256 != 0 || d.D > 1024 || d.pages <= 0 || d.coord % 4 || d.shape % 4 || 4 * d.coord + 2 * d.shape != d.D ||
      d.npad < d.max_text + d.n_vis)
    return mhip_fail(ctx, MHIP_EINVAL, "lmv3_embed: D=%d coord=%d shape=%d", d.D, d.coord, d.shape);
  EmbedArgs a;
  a.tok = d.tok; a.word = d.word; a.type0 = d.type0; a.pos = d.pos; a.xe = d.xe; a.ye = d.ye; a.he = d.he; a.we = d.we;
  a.g_text = d.g_text; a.b_text = d.b_text; a.patches = d.patches; a.cls = d.cls; a.g_vis = d.g_vis; a.b_vis = d.b_vis;
  a.g_all = d.g_all; a.b_all = d.b_all; a.h = d.h; a.ht = d.ht;
  a.rows = d.pages * d.npad; a.max_text = d.max_text; a.n_vis = d.n_vis; a.npad = d.npad; a.D = d.D; a.coord = d.coord;
  a.shape = d.shape; a.eps = d.eps; a.eps_vis = d.eps_vis;
  dim3 grid((a.rows + 3) / 4), block(256);
  if (precision == MHIP_PREC_F16) PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(lmv3_embed_kernel<_Float16>, grid, block, 0, ctx->stream, a));
  else PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(lmv3_embed_kernel<float>, grid, block, 0, ctx->stream, a));
  CHECK_LAUNCH(ctx, "lmv3_embed");
  return 0;
}

int mhip_launch_lmv3_head(mhip_ctx* ctx, const float* h, int pages, int npad, int D, const float* dw, const float* db,
                          const float* ow, const float* ob, int labels, float* logits) {
  if (pages <= 0 || D > 1024 || labels < 1) return mhip_fail(ctx, MHIP_EINVAL, "lmv3_head: pages=%d D=%d labels=%d", pages, D, labels);
  PROF_LAUNCH(ctx, MHIP_K_VIT_OPS, hipLaunchKernelGGL(lmv3_head_kernel, dim3(pages), dim3(256), 0, ctx->stream, h, npad, D, dw, db, ow, ob, labels, logits));
  CHECK_LAUNCH(ctx, "lmv3_head");
  return 0;
}
