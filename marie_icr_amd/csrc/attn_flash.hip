// attn_flash.hip — fused softmax attention at head dim 64, plain (the ViT encoders of the DiT detector and of TrOCR) and with
// LayoutLMv3's relative-position bias and key mask.  Both forms are ONE kernel body per precision; the bias is a compile-time
// switch (BIAS) over exactly three passages of it.  A kernel takes the bias as an optional argument (the parameter pack
// `Bias...` is empty, or one BiasArgs): the unbiased instance has no such argument at all.
//
// Replaces, in marie/boxes/dit/ditod/beit.py: Attention.forward's q@k^T -> softmax -> @v (:175-260); in
// transformers/models/layoutlmv3/modeling_layoutlmv3.py: LayoutLMv3SelfAttention.forward's scores + (rel_pos + rel_2d_pos) /
// sqrt(d) + mask -> softmax -> @ v.
//
// attention (f16): one workgroup = 128 queries of one (image, head): 4 waves x 32 queries.  It is computed TRANSPOSED
// so that no operand ever needs a lane shuffle:  S^T = K Q^T  puts a query in a lane's column (C layout col = lane&15),
// so the online-softmax max/sum are per-lane loops plus two cross-lane steps, and the probabilities a lane holds after
// exp2 ARE the B operand of  O^T = V^T P^T  (k index = key) once the K rows of a tile are staged in the order
// key(kt, i) = 32(kt>>1) + 8(i>>2) + 4(kt&1) + (i&3).  V arrives pre-transposed ([d][token], written by its projection
// GEMM), so both K and V^T tiles go HBM -> LDS by LDS-DMA with 128-byte rows and the conflict-free XOR slot swizzle.
//
// bias (BIAS = true): the bias of a score depends on (i, j) only through three integer differences, so per head three
// difference-indexed tables (mhip_attn_bias_fold, layoutlmv3_ops.hip) live in LDS behind the K / V^T ring (22.0 KB at 512 text
// rows and a 1024 grid), and each score takes three ds_read_b32 addressed from per-token codes, between S^T and the padding test.
#include "igemm_common.h"

using namespace igemm;

namespace {

constexpr int HD = 64;            // head dim of every model on this path (768/12, 1024/16)

struct AttnArgs {
  const char* q;     // row pitch ldq elements; head h at column h*64 (pre-scaled by head_dim^-0.5 * log2 e)
  const char* k;     // row pitch ldk; head h at column h*64
  const char* vt;    // [heads*64][ldv]: V^T, column = image*npad_k + key
  char* out;         // [rows][ldo], head h at column h*64
  int ldq, ldk, ldv, ldo;
  int npad_q, npad_k;   // rows per image on the query / key side
  int n_keys;           // valid keys per image
  int heads, nqb;       // nqb = npad_q / 128
};
struct BiasArgs {      // AttnBiasDesc (common.h) says what the codes and the tables hold
  const uint32_t* qcode;
  const uint32_t* kcode;
  const float* tab;
  int dp, dx, tab_len;
};

constexpr int AT_THREADS = 256, AT_QB = 128, AT_KT = 64;
constexpr int AT_TILE = AT_KT * 128;                 // bytes of a K tile (64 keys x 64 f16) == of a V^T tile (64 d x 64 keys)
constexpr int AT_STAGE = 2 * AT_TILE, AT_NSTAGE = 2;
constexpr int AT_TAB = AT_NSTAGE * AT_STAGE;         // byte offset of the bias tables in LDS: behind the ring

template <typename... Bias>      // nothing, or BiasArgs
__global__ __launch_bounds__(AT_THREADS) void attn_flash_f16_kernel(AttnArgs p, Bias... bias) {
  constexpr bool BIAS = sizeof...(Bias) == 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  // consecutive logical ids on one XCD: the query blocks of an (image, head) share its K / V^T through that XCD's L2
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

  // byte offsets into the tables that the key fields are added to: (table start + range - own field) * 4
  [[maybe_unused]] int b1[2], bx[2], by[2];
  [[maybe_unused]] const uint32_t* kc = nullptr;
  if constexpr (BIAS) {
    const BiasArgs& bp = (bias, ...);
    // this head's tables -> LDS (visible after the first barrier of the tile loop)
    const float* src = bp.tab + (size_t)h * bp.tab_len;
    float* dst = (float*)(smem + AT_TAB);
    for (int e = tid; e < bp.tab_len; e += AT_THREADS) dst[e] = src[e];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const uint32_t c = bp.qcode[qrow0 + qt * 16 + n];
      const int off_x = 3 * bp.dp + 2, off_y = off_x + 2 * bp.dx + 1;
      b1[qt] = AT_TAB + (bp.dp - (int)(c & 0xfff)) * 4;
      bx[qt] = AT_TAB + (off_x + bp.dx - (int)((c >> 12) & 0x3ff)) * 4;
      by[qt] = AT_TAB + (off_y + bp.dx - (int)(c >> 22)) * 4;
    }
    kc = bp.kcode + krow0 + 8 * g;
  }

  // Q^T B-operands: lane (g, n) holds Q[query n of tile qt][d = 32 ks + 8 g + j]
  half8 qreg[2][2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      qreg[qt][ks] = *(const half8*)(p.q + ((qrow0 + qt * 16 + n) * p.ldq + h * HD + ks * 32 + g * 8) * 2);

  // staging: thread moves chunks (wave-instruction q covers 8 LDS rows): rows (q*4 + wave)*8 + (lane>>3), slot lane&7
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
  // tiles are staged in order: the source pointers run along (a multiply-add per tile and pointer cost ~30 VALU instructions of
  // a loop that is VALU-bound)
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
  // Online soft-max with a STALE reference: scores come out of the MFMA already minus the row's reference m (it is the
  // accumulator's initial value), and m only moves when a tile's maximum exceeds it by more than RESCALE_AT (2^8 in
  // probability) — then, and on the first tile, O^T and l are rescaled.  On every other tile the per-element subtraction,
  // the alpha exponentials and the 32 accumulator multiplies disappear from a loop whose VALU work (~800 cycles per tile
  // and wave) exceeds its MFMA work (512).  O / l at the end is independent of the reference.
  constexpr float RESCALE_AT = 8.f;
  float4v negm[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // -m of this lane's query, broadcast: the MFMA's C operand
  // The soft-max denominators come from the matrix cores as well: a 17th "value row" of ones, i.e. an A operand whose row 0 is
  // all ones (a constant fragment, no LDS), gives l[query] = sum of the SAME f16-rounded probabilities the numerator uses in
  // row 0 of acc_l (lanes g = 0, element 0).  That takes the 32 adds per tile (hipcc packs them into v_pk_add_f32, which
  // costs more than two plain adds beside MFMAs) out of the VALU stream for 4 more MFMAs per tile.
  const half8 ones = n == 0 ? (half8){1, 1, 1, 1, 1, 1, 1, 1} : (half8){0, 0, 0, 0, 0, 0, 0, 0};
  float4v acc_l[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};

  // fragment read offsets (row = n within a 16-row tile, logical slot = g (+4 for the second k step))
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
    [[maybe_unused]] uint4v kcode[4];
    if constexpr (BIAS) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) kcode[kt] = *(const uint4v*)(kc + t * AT_KT + 32 * (kt >> 1) + 4 * (kt & 1));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 1 < ntiles) stage(fill);
    const char* sk = smem + slot * AT_STAGE;
    const char* sv = sk + AT_TILE;

    // ---- S^T = K Q^T ------------------------------------------------------------------------------------
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
    if constexpr (BIAS) {
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
    }
    if ((t + 1) * AT_KT > p.n_keys) {   // keys past the end of the image (padding rows)
      const int kbase = t * AT_KT;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kbase + 32 * (kt >> 1) + 8 * g + 4 * (kt & 1) + r;
          if (key >= p.n_keys) { s[kt][0][r] = -INFINITY; s[kt][1][r] = -INFINITY; }
        }
    }
    // ---- online softmax (base 2; the log2 e factor lives in the query scale) -------------------------------
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
      tmax[qt] = mx;                       // the tile's maximum relative to the reference
    }
    const bool move = t == 0 || tmax[0] > RESCALE_AT || tmax[1] > RESCALE_AT;
    if (__builtin_amdgcn_ballot_w64(move) != 0) {      // wave-uniform: some query of this wave moves its reference
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        // first tile: the reference becomes the tile maximum whatever it is; later: a query moves only on ITS OWN excess
        // (d = 0 leaves it bit-for-bit alone: alpha = 1, s - 0), so its arithmetic never depends on its wave's neighbours
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
    // ---- O^T += V^T P^T ----------------------------------------------------------------------------------------
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
  // ---- normalise and store: lane holds O^T[d = 16 dt + 4 g + r][query n] -> 4 consecutive d of one output row ------
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const float inv = 1.f / __shfl(acc_l[qt][0], n);          // row 0 of the ones tile lives in lanes g = 0

    if (qb * AT_QB + wave * 32 + qt * 16 + n >= p.npad_q) continue;   // the last block may reach into the next image
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

// fp32 parity mode: one wave per query, lane = key stripe; plain online softmax with fp32 FMAs (no matrix cores).  BIAS: the
// tables are read from HBM (L2-resident), and a masked key is skipped, so its probability is exactly 0 as the library's
// finfo.min mask makes it.
template <typename... Bias>      // nothing, or BiasArgs
__global__ __launch_bounds__(256) void attn_simple_f32_kernel(AttnArgs p, Bias... bias, int n_queries) {
  constexpr bool BIAS = sizeof...(Bias) == 1;
  const int lane = threadIdx.x & 63;
  const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int h = blockIdx.y, img = blockIdx.z;
  if (qi >= n_queries) return;
  const float* Q = (const float*)p.q + ((size_t)img * p.npad_q + qi) * p.ldq + h * HD;
  const float* K = (const float*)p.k + (size_t)img * p.npad_k * p.ldk + h * HD;
  const float* VT = (const float*)p.vt + (size_t)h * HD * p.ldv + (size_t)img * p.npad_k;
  [[maybe_unused]] const uint32_t* KC = nullptr;
  [[maybe_unused]] const float *T1 = nullptr, *TX = nullptr, *TY = nullptr;      // the tables, offset by this query's fields
  if constexpr (BIAS) {
    const BiasArgs& bp = (bias, ...);
    const uint32_t qc = bp.qcode[(size_t)img * p.npad_q + qi];
    KC = bp.kcode + (size_t)img * p.npad_k;
    const int off_x = 3 * bp.dp + 2, off_y = off_x + 2 * bp.dx + 1;
    T1 = bp.tab + (size_t)h * bp.tab_len + bp.dp - (int)(qc & 0xfff);
    TX = bp.tab + (size_t)h * bp.tab_len + off_x + bp.dx - (int)((qc >> 12) & 0x3ff);
    TY = bp.tab + (size_t)h * bp.tab_len + off_y + bp.dx - (int)(qc >> 22);
  }
  float q[HD], o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) { q[d] = Q[d]; o[d] = 0.f; }
  float m = -INFINITY, l = 0.f;
  for (int key = lane; key < p.n_keys; key += 64) {
    [[maybe_unused]] const uint32_t c = BIAS ? KC[key] : 0;      // the key's code
    [[maybe_unused]] const int kp = (int)(c & 0xfff);
    if constexpr (BIAS)
      if (kp > 2 * (bias, ...).dp) continue;                     // a masked key
    const float* kr = K + (size_t)key * p.ldk;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) s += q[d] * kr[d];
    if constexpr (BIAS) s += (T1[kp] + TX[(c >> 12) & 0x3ff]) + TY[c >> 22];
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

// bd: the bias of the launch, or null.  `who` prefixes the error texts.
int launch_attention(mhip_ctx* ctx, int precision, const AttnDesc& d, const AttnBiasDesc* bd, const char* who) {
  if (d.images <= 0 || d.heads <= 0 || d.n_keys <= 0 || d.n_queries <= 0 || d.npad_k % 8 || d.n_queries > d.npad_q ||
      d.n_keys > d.npad_k)
    return mhip_fail(ctx, MHIP_EINVAL, "%s: bad shape (q %d/%d, k %d/%d)", who, d.n_queries, d.npad_q, d.n_keys, d.npad_k);
  if (bd && (!bd->qcode || !bd->kcode || !bd->tab || bd->dp < 0 || bd->dp > 1023 || bd->dx < 0 || bd->dx > 1023 ||
             ((uintptr_t)bd->kcode & 15)))
    return mhip_fail(ctx, MHIP_EINVAL, "%s: bad tables (dp %d, dx %d)", who, bd->dp, bd->dx);
  const int esz = precision == MHIP_PREC_F16 ? 2 : 4;
  if ((d.ldq * esz) % 16 || (d.ldk * esz) % 16 || (d.ldv * esz) % 16 || (d.ldo * esz) % 8)
    return mhip_fail(ctx, MHIP_EINVAL, "%s: row pitches must keep 16-byte alignment", who);
  AttnArgs a;
  a.q = (const char*)d.q; a.k = (const char*)d.k; a.vt = (const char*)d.vt; a.out = (char*)d.out;
  a.ldq = d.ldq; a.ldk = d.ldk; a.ldv = d.ldv; a.ldo = d.ldo;
  a.npad_q = d.npad_q; a.npad_k = d.npad_k; a.n_keys = d.n_keys; a.heads = d.heads;
  a.nqb = (d.n_queries + AT_QB - 1) / AT_QB;
  BiasArgs b = {};
  if (bd) {
    b.qcode = bd->qcode; b.kcode = bd->kcode; b.tab = bd->tab; b.dp = bd->dp; b.dx = bd->dx;
    b.tab_len = mhip_attn_bias_table_len(bd->dp, bd->dx);
  }
  const int kid = bd ? MHIP_K_ATTN_BIAS : MHIP_K_ATTN_FLASH;
  if (ctx->profiling) ctx->prof[kid].flops += mhip_attention_flops(d);
  if (precision == MHIP_PREC_F16) {
    const int lds = AT_TAB + b.tab_len * 4;      // the ring, + the tables: <= 32768 + 28668 bytes
    static std::once_flag attr;
    std::call_once(attr, [] {
      (void)hipFuncSetAttribute((const void*)attn_flash_f16_kernel<>, hipFuncAttributeMaxDynamicSharedMemorySize, AT_TAB);
      (void)hipFuncSetAttribute((const void*)attn_flash_f16_kernel<BiasArgs>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    });
    dim3 grid((unsigned)(a.nqb * d.heads * d.images)), block(AT_THREADS);
    if (bd) PROF_LAUNCH(ctx, kid, hipLaunchKernelGGL(attn_flash_f16_kernel<BiasArgs>, grid, block, lds, ctx->stream, a, b));
    else PROF_LAUNCH(ctx, kid, hipLaunchKernelGGL(attn_flash_f16_kernel<>, grid, block, lds, ctx->stream, a));
  } else {
    dim3 grid((d.n_queries + 3) / 4, d.heads, d.images), block(256);
    if (bd) PROF_LAUNCH(ctx, kid, hipLaunchKernelGGL(attn_simple_f32_kernel<BiasArgs>, grid, block, 0, ctx->stream, a, b, d.n_queries));
    else PROF_LAUNCH(ctx, kid, hipLaunchKernelGGL(attn_simple_f32_kernel<>, grid, block, 0, ctx->stream, a, d.n_queries));
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mhip_fail(ctx, MHIP_EHIP, "%s launch: %s", who, hipGetErrorString(e));
  return 0;
}

}  // namespace

int mhip_launch_attention(mhip_ctx* ctx, int precision, const AttnDesc& d) {
  return launch_attention(ctx, precision, d, nullptr, "attention");
}

int mhip_launch_attention_bias(mhip_ctx* ctx, int precision, const AttnBiasDesc& bd) {
  return launch_attention(ctx, precision, bd.a, &bd, "attention_bias");
}

double mhip_attention_flops(const AttnDesc& d) {
  return 4.0 * d.images * d.heads * (double)d.n_queries * d.n_keys * HD;
}
