// lev_ngrams.hip — unit-cost edit distance of every (template text, page n-gram) pair of a page: the hot loop of
// MetaTemplateMatcher (marie/components/template_matching/meta_template_matching.py:152-187, Levenshtein.distance of
// " ".join(words[i:i+n]).strip().upper() against the template text for n = g - 1, g, g + 1).
//
// Layout (built by the caller, template_matching.text_layout): the page is ONE string S = the upper-cased words joined by
// blanks, as dense alphabet ids (1 .. A: the code points of the template texts; 0: any other code point, which matches
// nothing), and a candidate (i, n) is the substring S[a:b] with a = min(fs[i], we[i+n-1]), b = max(le[i+n-1], a)  (fs / le:
// the strip() of a string that starts at word i / ends at word j, precomputed per word).  Nothing is copied per candidate.
//
// Kernel: one lane per candidate, a workgroup = one template x LEV_TILE consecutive (k, i).  The template is the PATTERN of
// Myers' bit-vector algorithm in Hyyro's blocked form: Peq[w][id] (64 pattern positions a word, W = ceil(m / 64) words a
// character) sits in LDS, a lane streams its candidate's ids and carries the vertical deltas Pv[W], Mv[W] and the score in
// registers.  W is a template parameter (1, 2, 4, 8, 16): with W = 1 — template texts of up to 64 code points, the usual
// case — the state is two 64-bit registers.  Templates are grouped by instance; one launch per instance present.
//   * Peq is stored word-major, [w][id], not [id][w]: in step (character j, word w) every lane reads word w of ITS character's
//     row.  ds_read_b64 banks by (address / 4) mod 64, i.e. 32 distinct 8-byte slots; word-major puts the A + 1 slots a wave
//     can touch in one instruction next to each other, so two lanes collide only when their ids differ by a multiple of 32
//     (equal ids broadcast).  Row-major would put them W slots apart: W = 16 leaves 2 usable slots.
//   * The ids of S are read from global memory, two bytes a lane a step.  Neighbouring lanes read overlapping spans of S (lane
//     i + 1 starts one word later), a page is a few tens of KB, so after the first touch the reads are L1 / L2 hits; staging a
//     tile's span in LDS would need a bound on the words' lengths that the input does not give.
#include <algorithm>

#include "common.h"

constexpr int LEV_TILE = 256;             // candidates (lanes) per workgroup
constexpr int LEV_MAX_M = 1024;           // longest pattern, code points
constexpr size_t LEV_LDS_BYTES = 65536;   // Peq budget of a workgroup: (A + 1) * W * 8 bytes; two workgroups fit a CU's 160 KiB

struct LevTmpl {
  int32_t index;      // row of the outputs
  int32_t m;          // pattern length
  int32_t g;          // words of the template text: the n-gram sizes are g - 1, g, g + 1
  int32_t W;          // ceil(m / 64)
  uint32_t peq_off;   // first 64-bit word of this template's Peq [W][rows]
};

// the distance of the pattern behind s_peq to txt[0:len]; __host__ as well, so that a plain program can check it against the DP
template <int WC>
__host__ __device__ __forceinline__ int lev_myers(const uint64_t* __restrict__ s_peq, int rows, int W, int m,
                                         const uint16_t* __restrict__ txt, int len) {
  uint64_t Pv[WC], Mv[WC];
#pragma unroll
  for (int w = 0; w < WC; ++w) { Pv[w] = ~0ull; Mv[w] = 0ull; }
  int score = m;
  const int wl = (m - 1) >> 6;
  const uint64_t top = 1ull << ((m - 1) & 63);
  for (int j = 0; j < len; ++j) {
    const int c = txt[j];
    uint64_t pin = 1ull, min_ = 0ull;      // the horizontal delta entering word 0 is +1: D[0][j] = j
#pragma unroll
    for (int w = 0; w < WC; ++w) {
      if (w < W) {
        uint64_t Eq = s_peq[w * rows + c];
        const uint64_t pv = Pv[w], mv = Mv[w];
        const uint64_t Xv = Eq | mv;
        Eq |= min_;
        const uint64_t Xh = (((Eq & pv) + pv) ^ pv) | Eq;
        uint64_t Ph = mv | ~(Xh | pv);
        uint64_t Mh = pv & Xh;
        if (w == wl) score += (Ph & top) ? 1 : ((Mh & top) ? -1 : 0);
        const uint64_t pout = Ph >> 63, mout = Mh >> 63;
        Ph = (Ph << 1) | pin;
        Mh = (Mh << 1) | min_;
        Pv[w] = Mh | ~(Xv | Ph);
        Mv[w] = Ph & Xv;
        pin = pout; min_ = mout;
      }
    }
  }
  return score;
}

// run_end (or null): the last word index j >= i with line[i] == ... == line[j]; dist / len [T][3][N], -1 where no candidate
template <int WC>
__global__ __launch_bounds__(LEV_TILE) void lev_ngrams_kernel(const uint16_t* __restrict__ page, const int32_t* __restrict__ we,
                                                              const int32_t* __restrict__ fs, const int32_t* __restrict__ le,
                                                              const int32_t* __restrict__ run_end, int N,
                                                              const LevTmpl* __restrict__ tab, const uint64_t* __restrict__ peq,
                                                              int rows, int32_t* __restrict__ dist, int32_t* __restrict__ len) {
  extern __shared__ uint64_t s_peq[];
  const LevTmpl t = tab[blockIdx.y];
  for (int idx = threadIdx.x; idx < rows * t.W; idx += LEV_TILE) s_peq[idx] = peq[t.peq_off + idx];
  __syncthreads();
  const long long c = (long long)blockIdx.x * LEV_TILE + threadIdx.x;
  if (c >= 3ll * N) return;
  const int k = (int)(c / N), i = (int)(c - (long long)k * N);
  const int n = t.g - 1 + k;
  int d = -1, l = -1;
  if (n >= 1 && n <= N && i <= N - n && (!run_end || i + n - 1 <= run_end[i])) {
    const int last = i + n - 1;
    const int a = min(fs[i], we[last]);
    const int b = max(le[last], a);
    l = b - a;
    d = t.m == 0 ? l : lev_myers<WC>(s_peq, rows, t.W, t.m, page + a, l);
  }
  const size_t o = ((size_t)t.index * 3 + k) * N + i;
  dist[o] = d;
  len[o] = l;
}

template <int WC>
static void lev_launch(mhip_ctx* ctx, dim3 grid, size_t lds, const uint16_t* page, const int32_t* we, const int32_t* fs,
                       const int32_t* le, const int32_t* run_end, int N, const LevTmpl* tab, const uint64_t* peq, int rows,
                       int32_t* dist, int32_t* len) {
  PROF_LAUNCH(ctx, MHIP_K_LEV_NGRAMS, hipLaunchKernelGGL(lev_ngrams_kernel<WC>, grid, dim3(LEV_TILE), lds, ctx->stream, page, we,
                                                         fs, le, run_end, N, tab, peq, rows, dist, len));
}

static int lev_instance(int W) { return W <= 1 ? 1 : W <= 2 ? 2 : W <= 4 ? 4 : W <= 8 ? 8 : 16; }

extern "C" int mhip_lev_ngrams_host(mhip_ctx* ctx, const uint16_t* page_ids, int L, const int32_t* ws, const int32_t* we,
                                    const int32_t* fs, const int32_t* le, const int32_t* line_ids, int N,
                                    const uint16_t* tmpl_ids, const int32_t* tmpl_off, const int32_t* g, int T, int alphabet,
                                    int32_t* dist_out, int32_t* len_out) {
  if (!ctx) return MHIP_EINVAL;
  if (!ws || !we || !fs || !le || !tmpl_off || !g || !dist_out || !len_out || L < 0 || (L > 0 && !page_ids))
    return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: null argument");
  if (N < 1 || N > (1 << 24) || T < 1 || T > 65535 || alphabet < 0 || alphabet > 65535)
    return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: %d words, %d templates, an alphabet of %d", N, T, alphabet);
  if ((size_t)T * 3 * N > ((size_t)1 << 30)) return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: %d x 3 x %d results", T, N);
  for (int i = 0; i < N; ++i)
    if (ws[i] < 0 || we[i] < ws[i] || we[i] > L || fs[i] < 0 || fs[i] > L || le[i] < 0 || le[i] > L)
      return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: word %d lies outside the %d ids of the page", i, L);
  for (int p = 0; p < L; ++p)
    if (page_ids[p] > alphabet) return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: page id %d of an alphabet of %d", (int)page_ids[p], alphabet);
  const int rows = alphabet + 1;
  if (tmpl_off[0] != 0) return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: the template offsets start at %d", tmpl_off[0]);
  std::vector<LevTmpl> tab[5];     // by instance 1, 2, 4, 8, 16
  size_t peq_words = 0;
  for (int t = 0; t < T; ++t) {
    const int m = tmpl_off[t + 1] - tmpl_off[t];
    if (m < 0 || m > LEV_MAX_M) return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: template %d has %d code points, 0..%d are built", t, m, LEV_MAX_M);
    if (m > 0 && !tmpl_ids) return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: null argument");
    if (g[t] < 1 || g[t] > (1 << 30)) return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: template %d of %d words", t, g[t]);
    const int W = (m + 63) / 64;
    if ((size_t)rows * W * sizeof(uint64_t) > LEV_LDS_BYTES)
      return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: template %d: %d code points over an alphabet of %d need %zu bytes of LDS, %zu are budgeted",
                       t, m, alphabet, (size_t)rows * W * sizeof(uint64_t), LEV_LDS_BYTES);
    for (int j = 0; j < m; ++j) {
      const int id = tmpl_ids[tmpl_off[t] + j];
      if (id < 1 || id > alphabet) return mhip_fail(ctx, MHIP_EINVAL, "lev_ngrams: template %d holds id %d of an alphabet of %d", t, id, alphabet);
    }
    const int inst = lev_instance(W);
    tab[inst == 1 ? 0 : inst == 2 ? 1 : inst == 4 ? 2 : inst == 8 ? 3 : 4].push_back(LevTmpl{t, m, g[t], W, (uint32_t)peq_words});
    peq_words += (size_t)rows * W;
  }
  std::vector<uint64_t> peq(std::max<size_t>(peq_words, 1), 0ull);
  std::vector<LevTmpl> all;
  for (auto& cls : tab)
    for (const LevTmpl& e : cls) {
      for (int j = 0; j < e.m; ++j) peq[e.peq_off + (size_t)(j >> 6) * rows + tmpl_ids[tmpl_off[e.index] + j]] |= 1ull << (j & 63);
      all.push_back(e);
    }
  std::vector<int32_t> run_end;
  if (line_ids) {
    run_end.resize(N);
    run_end[N - 1] = N - 1;
    for (int i = N - 2; i >= 0; --i) run_end[i] = line_ids[i] == line_ids[i + 1] ? run_end[i + 1] : i;
  }

  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t cells = (size_t)T * 3 * N;
  uint16_t* page_d = nullptr;
  int32_t *we_d = nullptr, *fs_d = nullptr, *le_d = nullptr, *run_d = nullptr, *dist_d = nullptr, *len_d = nullptr;
  LevTmpl* tab_d = nullptr;
  uint64_t* peq_d = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& c) {
    page_d = c.take<uint16_t>(sizeof(uint16_t) * std::max(L, 1));
    we_d = c.take<int32_t>(sizeof(int32_t) * N); fs_d = c.take<int32_t>(sizeof(int32_t) * N); le_d = c.take<int32_t>(sizeof(int32_t) * N);
    run_d = c.take<int32_t>(sizeof(int32_t) * N);
    tab_d = c.take<LevTmpl>(sizeof(LevTmpl) * T);
    peq_d = c.take<uint64_t>(sizeof(uint64_t) * peq.size());
    dist_d = c.take<int32_t>(sizeof(int32_t) * cells); len_d = c.take<int32_t>(sizeof(int32_t) * cells);
  });
  if (rc) return rc;
  auto run = [&]() -> int {
    if (L > 0) MHIP_HIP(ctx, hipMemcpyAsync(page_d, page_ids, sizeof(uint16_t) * L, hipMemcpyHostToDevice, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(we_d, we, sizeof(int32_t) * N, hipMemcpyHostToDevice, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(fs_d, fs, sizeof(int32_t) * N, hipMemcpyHostToDevice, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(le_d, le, sizeof(int32_t) * N, hipMemcpyHostToDevice, ctx->stream));
    if (line_ids) MHIP_HIP(ctx, hipMemcpyAsync(run_d, run_end.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(tab_d, all.data(), sizeof(LevTmpl) * T, hipMemcpyHostToDevice, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(peq_d, peq.data(), sizeof(uint64_t) * peq.size(), hipMemcpyHostToDevice, ctx->stream));
    const unsigned tiles = (unsigned)((3ll * N + LEV_TILE - 1) / LEV_TILE);
    const int32_t* rd = line_ids ? run_d : nullptr;
    size_t at = 0;
    for (int cls = 0; cls < 5; ++cls) {
      const size_t n = tab[cls].size();
      if (!n) continue;
      int wmax = 0;
      for (const LevTmpl& e : tab[cls]) wmax = std::max(wmax, e.W);
      const size_t lds = std::max<size_t>((size_t)rows * wmax * sizeof(uint64_t), sizeof(uint64_t));
      const dim3 grid(tiles, (unsigned)n);
      switch (cls) {
        case 0: lev_launch<1>(ctx, grid, lds, page_d, we_d, fs_d, le_d, rd, N, tab_d + at, peq_d, rows, dist_d, len_d); break;
        case 1: lev_launch<2>(ctx, grid, lds, page_d, we_d, fs_d, le_d, rd, N, tab_d + at, peq_d, rows, dist_d, len_d); break;
        case 2: lev_launch<4>(ctx, grid, lds, page_d, we_d, fs_d, le_d, rd, N, tab_d + at, peq_d, rows, dist_d, len_d); break;
        case 3: lev_launch<8>(ctx, grid, lds, page_d, we_d, fs_d, le_d, rd, N, tab_d + at, peq_d, rows, dist_d, len_d); break;
        default: lev_launch<16>(ctx, grid, lds, page_d, we_d, fs_d, le_d, rd, N, tab_d + at, peq_d, rows, dist_d, len_d); break;
      }
      CHECK_LAUNCH(ctx, "lev_ngrams");
      at += n;
    }
    MHIP_HIP(ctx, hipMemcpyAsync(dist_out, dist_d, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
    MHIP_HIP(ctx, hipMemcpyAsync(len_out, len_d, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->stream));
    MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MHIP_OK;
  };
  rc = run();
  if (rc) (void)hipStreamSynchronize(ctx->stream);    // the host temporaries above outlive every copy that reads them
  return rc;
}
