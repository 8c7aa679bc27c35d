// vqnnf.hip — VQ-NNF template matching (arXiv 2306.15010) on the colour features of a page, gfx950.
//
// replaces: marie/components/template_matching/vqnnf/matching/{template_matching,kmeans,gauss_haar_filters}.py with the
// num_features == 27 path of feature_extraction.py, and the peak loop of vqnnf_template_matching.py:184-202,307.
//
//   vq_assign        a pixel's 27 features (its RGB and its eight neighbours, wrapping around its own window) are formed in
//                    registers; the nearest code is by the direct sum of squared differences in feature order, in fp64 with
//                    every operation rounded, first minimum.
//   vq_kmeans_update one workgroup per cluster: exact integer sums of the members' bytes, mean = sum / (255 n) in fp64.
//   vq_filter        a workgroup owns a 16 x 64 tile of filter positions of one (window, template).  Per code it builds the
//                    double prefix sum of the code's one-hot over the tile and its footprint in LDS as uint16 — the filters'
//                    taps sum to zero along every row and column, so the origin of the prefix sum cancels and a local one
//                    gives the same response as the whole window's — and adds |response - template response| / K into fp64
//                    registers.  A code absent from the footprint has response 0 and skips the prefix sum.  Nothing of
//                    K x H x W is ever in HBM: what leaves the kernel is one fp64 plane per distinct filter.
//   vq_combine       each filter's minimum over its valid region, then the sum of the centred, minimum-padded filters.
//   vq_peaks         row-major first maximum per map, then the reference's suppression rectangle (Python slice rules).
//   clip_cosine      the features of two clips are nine permutations of the same pixels, applied to both alike, so their
//                    cosine is the cosine of the pixels: three exact integer sums per pair.
#include "common.h"

#include <algorithm>

namespace {

constexpr int VQ_F = MHIP_VQ_FEATURES;
constexpr int VQ_MAXK = MHIP_VQ_MAX_CODES;
constexpr int VQ_NF = MHIP_VQ_MAX_FILTERS;
constexpr int VQ_TH = 16, VQ_TW = 64;          // filter positions per workgroup (256 threads, 4 rows each)
constexpr int VQ_MAX_ITER = 25;                // VQNNFMatcher: KMeans(max_iter=25)
constexpr double VQ_TOL = 1e-4;                // KMeans.tol
constexpr float VQ_SUPPRESSED = -0.82f;        // vqnnf_template_matching.py:307
constexpr size_t VQ_LDS_MAX = 160 * 1024;

// per-template table entry the match kernels read
struct VqTmplDev {
  const float* codebook;      // [K][27]
  const float* resp;          // [VQ_NF][VQ_MAXK]
  int K, bw, bh, nf, nd;
  int dil[VQ_NF][2];
  int slot[VQ_NF];            // plane of distinct filter responses filter f reads
  int dfilt[VQ_NF];           // the filter that plane d is computed from
  float taps[VQ_NF][16];
  double weight[VQ_NF];
};

// torch.roll(x, shifts=(sr, sc)): out[r][c] = x[r - sr][c - sc]; order of feature_extraction.py:53-66
__device__ __constant__ int kShiftR[9] = {0, 0, 0, 1, -1, 1, -1, 1, -1};
__device__ __constant__ int kShiftC[9] = {0, 1, -1, 0, 0, 1, -1, -1, 1};

__device__ __forceinline__ void vq_bytes(const uint8_t* win, size_t pitch, int H, int W, int r, int c, unsigned v[VQ_F]) {
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    int rr = r - kShiftR[s], cc = c - kShiftC[s];
    rr += rr < 0 ? H : 0; rr -= rr >= H ? H : 0;
    cc += cc < 0 ? W : 0; cc -= cc >= W ? W : 0;
    const uint8_t* p = win + (size_t)rr * pitch + (size_t)cc * 3;
    v[3 * s] = p[0]; v[3 * s + 1] = p[1]; v[3 * s + 2] = p[2];
  }
}

// Squared distances in fp64, the squared differences added one by one in feature order with every product and sum rounded
// (no fused multiply-add): bit-equal centroids give bit-equal distances, mirrored ones too where the sums allow, and the
// fp64 restatement the tests compare against (tests/vqnnf_ref.py) can follow the same order and agree on every tie.
__device__ __forceinline__ int vq_nearest(const unsigned v[VQ_F], const float* lut, const double* cb, int K) {
#pragma clang fp contract(off)
  double f[VQ_F];
#pragma unroll
  for (int j = 0; j < VQ_F; ++j) f[j] = (double)lut[v[j]];
  double best = INFINITY;
  int arg = 0;
  for (int k = 0; k < K; ++k) {
    double d = 0.0;
#pragma unroll
    for (int j = 0; j < VQ_F; ++j) {
      const double e = f[j] - cb[k * VQ_F + j];
      d = d + e * e;
    }
    if (d < best) { best = d; arg = k; }
  }
  return arg;
}

// codes[pair][rh*rw] for pair = window * n_tmpl + template; the window's origin is win_xy[window] (or the image's)
__global__ __launch_bounds__(256) void vq_assign_kernel(const uint8_t* img, size_t pitch, const int32_t* win_xy, int H, int W,
                                                        int rx, int ry, int rw, int rh, const VqTmplDev* __restrict__ tab,
                                                        int n_tmpl, uint8_t* codes) {
  __shared__ double s_cb[VQ_MAXK * VQ_F];
  __shared__ float s_lut[256];
  const int tid = threadIdx.x, pair = blockIdx.y, wi = pair / n_tmpl;
  const VqTmplDev& t = tab[pair % n_tmpl];
  const int K = t.K;
  for (int i = tid; i < K * VQ_F; i += 256) s_cb[i] = (double)t.codebook[i];
  s_lut[tid] = (float)tid / 255.0f;
  __syncthreads();
  const int p = blockIdx.x * 256 + tid;
  if (p >= rw * rh) return;
  const uint8_t* win = img + (win_xy ? (size_t)win_xy[2 * wi + 1] * pitch + (size_t)win_xy[2 * wi] * 3 : 0);
  unsigned v[VQ_F];
  vq_bytes(win, pitch, H, W, ry + p / rw, rx + p % rw, v);
  codes[(size_t)pair * rw * rh + p] = (uint8_t)vq_nearest(v, s_lut, s_cb, K);
}

// cent[k] = features of pixel idx[k] of the rectangle (init_methods._kpoints)
__global__ void vq_gather_kernel(const uint8_t* img, size_t pitch, int H, int W, int rx, int ry, int rw, const int32_t* idx,
                                 int K, float* cent) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  unsigned v[VQ_F];
  vq_bytes(img, pitch, H, W, ry + idx[k] / rw, rx + idx[k] % rw, v);
#pragma unroll
  for (int j = 0; j < VQ_F; ++j) cent[k * VQ_F + j] = (float)v[j] / 255.0f;
}

// one workgroup per cluster: new centroid, members, and the cluster's share of the error
__global__ __launch_bounds__(256) void vq_kmeans_update_kernel(const uint8_t* img, size_t pitch, int H, int W, int rx, int ry,
                                                               int rw, int rh, const uint8_t* labels, const float* cent_old,
                                                               float* cent_new, int32_t* counts, float* err_part) {
  __shared__ unsigned s_sum[256][VQ_F + 1];
  __shared__ float s_d[VQ_F];
  const int tid = threadIdx.x, k = blockIdx.x, n = rw * rh;
  unsigned acc[VQ_F + 1];
#pragma unroll
  for (int j = 0; j <= VQ_F; ++j) acc[j] = 0;
  for (int p = tid; p < n; p += 256) {
    if (labels[p] != k) continue;
    unsigned v[VQ_F];
    vq_bytes(img, pitch, H, W, ry + p / rw, rx + p % rw, v);
#pragma unroll
    for (int j = 0; j < VQ_F; ++j) acc[j] += v[j];
    acc[VQ_F] += 1;
  }
#pragma unroll
  for (int j = 0; j <= VQ_F; ++j) s_sum[tid][j] = acc[j];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
      for (int j = 0; j <= VQ_F; ++j) s_sum[tid][j] += s_sum[tid + s][j];
    __syncthreads();
  }
  const unsigned cnt = s_sum[0][VQ_F];
  if (tid < VQ_F) {
    const float c = cnt ? (float)((double)s_sum[0][tid] / (255.0 * (double)cnt)) : 0.f;   // empty cluster: the zero vector
    cent_new[k * VQ_F + tid] = c;
    const float d = c - cent_old[k * VQ_F + tid];
    s_d[tid] = d * d;
  }
  __syncthreads();
  if (tid == 0) {
    float e = 0.f;
    for (int j = 0; j < VQ_F; ++j) e += s_d[j];
    err_part[k] = e;
    counts[k] = (int32_t)cnt;
  }
}

// S[pair][d][i][j] = sum_c |y_d[c][i][j] - resp[c]| / K for the distinct filters d of the pair's template, (i, j) the top-left
// corner of the filter's footprint in the window
__global__ __launch_bounds__(256) void vq_filter_kernel(const uint8_t* __restrict__ codes, int H, int W,
                                                        const VqTmplDev* __restrict__ tab, int n_tmpl, double* __restrict__ S,
                                                        int planes) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.z;
  const VqTmplDev& t = tab[pair % n_tmpl];
  const int nd = t.nd, K = t.K;
  int dxm = 0, dym = 0, ni = 0, nj = 0;
  for (int d = 0; d < nd; ++d) {
    const int dx = t.dil[t.dfilt[d]][0], dy = t.dil[t.dfilt[d]][1];
    dxm = max(dxm, dx); dym = max(dym, dy);
    ni = max(ni, H - 3 * dx); nj = max(nj, W - 3 * dy);
  }
  const int i0 = blockIdx.y * VQ_TH, j0 = blockIdx.x * VQ_TW;
  if (i0 >= ni || j0 >= nj) return;                       // the whole workgroup
  const int RH = min(VQ_TH + 3 * dxm, H - i0), RW = min(VQ_TW + 3 * dym, W - j0);
  uint16_t* L = (uint16_t*)smem;                          // [RH][RW] prefix sums of one code's one-hot
  uint8_t* sc = (uint8_t*)(L + (size_t)RH * RW);          // [RH][RW] the codes of the footprint
  const uint8_t* cmap = codes + (size_t)pair * H * W;
  for (int e = tid; e < RH * RW; e += 256) sc[e] = cmap[(size_t)(i0 + e / RW) * W + j0 + e % RW];
  __syncthreads();

  const int ty = tid >> 6, tx = tid & 63;
  const double cw = 1.0 / (double)K;
  double acc[4][VQ_NF];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int d = 0; d < VQ_NF; ++d) acc[q][d] = 0.0;

  for (int c = 0; c < K; ++c) {
    // rows: inclusive prefix count along each row, one wave per row, 64 columns per ballot
    int any = 0;
    for (int r = wave; r < RH; r += 4) {
      int carry = 0;
      for (int cb = 0; cb < RW; cb += 64) {
        const int col = cb + lane;
        const bool bit = col < RW && sc[r * RW + col] == c;
        const unsigned long long m = __ballot(bit);
        if (col < RW) L[r * RW + col] = (uint16_t)(carry + __popcll(m & ((2ull << lane) - 1ull)));
        carry += __popcll(m);
      }
      any |= carry;
    }
    if (!__syncthreads_or(any)) {                         // the code is absent here: every response is 0
#pragma unroll
      for (int d = 0; d < VQ_NF; ++d)
        if (d < nd) {
          const double a = fabs(0.0 - (double)t.resp[t.dfilt[d] * VQ_MAXK + c]) * cw;
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q][d] += a;
        }
      continue;
    }
    for (int col = tid; col < RW; col += 256) {           // columns: running sum down each column
      unsigned run = 0;
      for (int r = 0; r < RH; ++r) {
        run += L[r * RW + col];
        L[r * RW + col] = (uint16_t)run;
      }
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < VQ_NF; ++d) {
      if (d >= nd) continue;
      const int f = t.dfilt[d], dx = t.dil[f][0], dy = t.dil[f][1];
      const double tr = (double)t.resp[f * VQ_MAXK + c];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int li = ty + 4 * q;
        if (i0 + li >= H - 3 * dx || j0 + tx >= W - 3 * dy) continue;
        double y = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            y = fma((double)t.taps[f][a * 4 + b], (double)L[(li + a * dx) * RW + tx + b * dy], y);
        acc[q][d] += fabs(y - tr) * cw;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int d = 0; d < VQ_NF; ++d) {
    if (d >= nd) continue;
    const int f = t.dfilt[d], dx = t.dil[f][0], dy = t.dil[f][1];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + ty + 4 * q, j = j0 + tx;
      if (i < H - 3 * dx && j < W - 3 * dy) S[(((size_t)pair * planes + d) * H + i) * W + j] = acc[q][d];
    }
  }
}

__device__ __forceinline__ double vq_block_min(double v, double* s_red) {
  const int tid = threadIdx.x;
  s_red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] = fmin(s_red[tid], s_red[tid + s]);
    __syncthreads();
  }
  const double r = s_red[0];
  __syncthreads();
  return r;
}

// heat[pair] = sum over the filters, in their order, of the centred valid region padded with the filter's own minimum
__global__ __launch_bounds__(256) void vq_combine_kernel(const double* __restrict__ S, int H, int W,
                                                         const VqTmplDev* __restrict__ tab, int n_tmpl, int planes,
                                                         float* heat, double* minima) {
  __shared__ double s_red[256];
  __shared__ double s_min[VQ_NF];
  const int tid = threadIdx.x, pair = blockIdx.x;
  const VqTmplDev& t = tab[pair % n_tmpl];
  for (int f = 0; f < t.nf; ++f) {
    const int hv = H - 3 * t.dil[f][0], wv = W - 3 * t.dil[f][1];
    const double* Sp = S + ((size_t)pair * planes + t.slot[f]) * H * W;
    double m = INFINITY;
    for (int e = tid; e < hv * wv; e += 256) m = fmin(m, -Sp[(size_t)(e / wv) * W + e % wv] * t.weight[f]);
    m = vq_block_min(m, s_red);
    if (tid == 0) {
      s_min[f] = m;
      if (minima) minima[pair * VQ_NF + f] = m;
    }
  }
  __syncthreads();
  for (int e = tid; e < H * W; e += 256) {
    const int r = e / W, c = e % W;
    double h = 0.0;
    for (int f = 0; f < t.nf; ++f) {
      const int hv = H - 3 * t.dil[f][0], wv = W - 3 * t.dil[f][1];
      const int i = r - (H - hv) / 2, j = c - (W - wv) / 2;
      const double* Sp = S + ((size_t)pair * planes + t.slot[f]) * H * W;
      h += (i >= 0 && i < hv && j >= 0 && j < wv) ? -Sp[(size_t)i * W + j] * t.weight[f] : s_min[f];
    }
    heat[(size_t)pair * H * W + e] = (float)h;
  }
}

// Python's slice(start, start + len).indices(size)
__device__ __forceinline__ void vq_py_slice(int start, int len, int size, int* lo, int* hi) {
  int a = start, b = start + len;
  a = a < 0 ? max(a + size, 0) : min(a, size);
  b = b < 0 ? max(b + size, 0) : min(b, size);
  *lo = a; *hi = max(a, b);
}

// round k of vqnnf_template_matching.py:186-307 for every map: first maximum in row-major order, then the rectangle of the
// box centred on it (odd() arithmetic, w and h swapped as there) is set to -0.82
__global__ __launch_bounds__(256) void vq_peaks_kernel(float* heat, int H, int W, const VqTmplDev* __restrict__ tab, int n_tmpl,
                                                       int k, int max_objects, float* peaks) {
  __shared__ float s_v[256];
  __shared__ int s_i[256];
  const int tid = threadIdx.x, pair = blockIdx.x, n = H * W;
  float* hm = heat + (size_t)pair * n;
  float best = -INFINITY;
  int arg = 0x7fffffff;
  for (int e = tid; e < n; e += 256) {
    const float v = hm[e];
    if (v > best) { best = v; arg = e; }
  }
  s_v[tid] = best; s_i[tid] = arg;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const float v = s_v[tid + s];
      const int i = s_i[tid + s];
      if (v > s_v[tid] || (v == s_v[tid] && i < s_i[tid])) { s_v[tid] = v; s_i[tid] = i; }
    }
    __syncthreads();
  }
  arg = s_i[0] == 0x7fffffff ? 0 : s_i[0];
  const int row = arg / W, col = arg % W;
  if (tid == 0) {
    float* o = peaks + ((size_t)pair * max_objects + k) * 3;
    o[0] = (float)row; o[1] = (float)col; o[2] = s_v[0];
  }
  const VqTmplDev& t = tab[pair % n_tmpl];
  const int qh = t.bh, qw = t.bw;                                     // rows, cols of the rectangle
  int r0, r1, c0, c1;
  vq_py_slice(row + 1 - (qh / 2 * 2 + 1 - 1) / 2, qh, H, &r0, &r1);   // odd(h) = h // 2 * 2 + 1
  vq_py_slice(col + 1 - (qw / 2 * 2 + 1 - 1) / 2, qw, W, &c0, &c1);
  const int rw = c1 - c0, cells = (r1 - r0) * rw;
  for (int e = tid; e < cells; e += 256) hm[(size_t)(r0 + e / rw) * W + c0 + e % rw] = VQ_SUPPRESSED;
}

// out[pair] = <a, b> / (|a| |b|) over `bytes` uint8 values, 0 when either is all zero
__global__ __launch_bounds__(256) void clip_cosine_kernel(const uint8_t* a, const uint8_t* b, int bytes, float* out) {
  __shared__ unsigned long long s_r[256][3];
  const int tid = threadIdx.x;
  const uint8_t* pa = a + (size_t)blockIdx.x * bytes;
  const uint8_t* pb = b + (size_t)blockIdx.x * bytes;
  unsigned long long ab = 0, aa = 0, bb = 0;
  for (int e = tid; e < bytes; e += 256) {
    const unsigned x = pa[e], y = pb[e];
    ab += x * y; aa += x * x; bb += y * y;
  }
  s_r[tid][0] = ab; s_r[tid][1] = aa; s_r[tid][2] = bb;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
      for (int j = 0; j < 3; ++j) s_r[tid][j] += s_r[tid + s][j];
    __syncthreads();
  }
  if (tid == 0) {
    const double na = sqrt((double)s_r[0][1]), nb = sqrt((double)s_r[0][2]);
    out[blockIdx.x] = (s_r[0][1] == 0 || s_r[0][2] == 0) ? 0.f : (float)((double)s_r[0][0] / (na * nb));
  }
}

// ------------------------------------------------------------------------------------------------------------ host side
bool vq_rect_ok(const int32_t* r, int H, int W) {
  return r && r[0] >= 0 && r[1] >= 0 && r[2] > 0 && r[3] > 0 && r[0] + r[2] <= W && r[1] + r[3] <= H;
}

// fills the filter part of a table entry; distinct filters (same taps, dilation and responses) share a plane
int vq_fill_filters(mhip_ctx* ctx, VqTmplDev* e, const mhip_vq_filters* fb, const float* resp, int K) {
  if (!fb || fb->n < 1 || fb->n > VQ_NF) return mhip_fail(ctx, MHIP_EINVAL, "vqnnf: 1..%d filters", VQ_NF);
  e->nf = fb->n;
  e->nd = 0;
  for (int f = 0; f < fb->n; ++f) {
    if (fb->dil[f][0] < 1 || fb->dil[f][1] < 1) return mhip_fail(ctx, MHIP_EINVAL, "vqnnf: filter %d has a dilation below 1", f);
    e->dil[f][0] = fb->dil[f][0]; e->dil[f][1] = fb->dil[f][1];
    e->weight[f] = fb->weight[f];
    memcpy(e->taps[f], fb->taps[f], sizeof(float) * 16);
    int same = -1;
    for (int g = 0; g < f && same < 0; ++g)
      if (!memcmp(fb->taps[g], fb->taps[f], sizeof(float) * 16) && !memcmp(fb->dil[g], fb->dil[f], sizeof(int32_t) * 2) &&
          !memcmp(resp + g * K, resp + f * K, sizeof(float) * K))
        same = g;
    if (same >= 0) {
      e->slot[f] = e->slot[same];
    } else {
      e->slot[f] = e->nd;
      e->dfilt[e->nd++] = f;
    }
  }
  return MHIP_OK;
}

struct VqPlan {
  int planes = 1;        // fp64 planes per pair
  int ni = 0, nj = 0;    // filter positions the grid covers
  size_t lds = 0;        // dynamic LDS of vq_filter_kernel
};

// what a set of templates needs of vq_filter_kernel on H x W windows
int vq_plan(mhip_ctx* ctx, const VqTmplDev* tab, int n, int H, int W, VqPlan* p) {
  for (int k = 0; k < n; ++k) {
    const VqTmplDev& t = tab[k];
    int dxm = 0, dym = 0;
    for (int f = 0; f < t.nf; ++f) {
      if (H - 3 * t.dil[f][0] < 1 || W - 3 * t.dil[f][1] < 1)
        return mhip_fail(ctx, MHIP_EINVAL, "vqnnf: a filter of %d x %d exceeds the %d x %d window", 3 * t.dil[f][0] + 1,
                         3 * t.dil[f][1] + 1, H, W);
      dxm = std::max(dxm, t.dil[f][0]); dym = std::max(dym, t.dil[f][1]);
      p->ni = std::max(p->ni, H - 3 * t.dil[f][0]); p->nj = std::max(p->nj, W - 3 * t.dil[f][1]);
    }
    const size_t cells = (size_t)std::min(VQ_TH + 3 * dxm, H) * std::min(VQ_TW + 3 * dym, W);
    if (cells > 65535 || cells * 3 > VQ_LDS_MAX)    // a uint16 count per cell, and 3 bytes of LDS
      return mhip_fail(ctx, MHIP_EINVAL, "vqnnf: a filter footprint of %zu cells does not fit LDS", cells);
    p->lds = std::max(p->lds, cells * 3);
    p->planes = std::max(p->planes, t.nd);
  }
  return MHIP_OK;
}

int vq_launch_assign(mhip_ctx* ctx, const uint8_t* img, size_t pitch, const int32_t* win_xy, int H, int W, const int32_t* rect,
                     const VqTmplDev* tab_dev, int n_tmpl, int pairs, uint8_t* codes) {
  dim3 grid((unsigned)((rect[2] * rect[3] + 255) / 256), (unsigned)pairs);
  PROF_LAUNCH(ctx, MHIP_K_VQ_ASSIGN, hipLaunchKernelGGL(vq_assign_kernel, grid, dim3(256), 0, ctx->stream, img, pitch, win_xy, H,
                                                        W, rect[0], rect[1], rect[2], rect[3], tab_dev, n_tmpl, codes));
  CHECK_LAUNCH(ctx, "vq_assign");
  return MHIP_OK;
}

int vq_launch_heatmap(mhip_ctx* ctx, const uint8_t* codes, int H, int W, const VqTmplDev* tab_dev, int n_tmpl, int pairs,
                      const VqPlan& p, double* S, float* heat, double* minima) {
  if (p.lds > 64 * 1024)
    MHIP_HIP(ctx, hipFuncSetAttribute((const void*)vq_filter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
  dim3 grid((unsigned)((p.nj + VQ_TW - 1) / VQ_TW), (unsigned)((p.ni + VQ_TH - 1) / VQ_TH), (unsigned)pairs);
  hipEvent_t e0 = nullptr;
  if (ctx->profiling) mhip_prof_begin(ctx, MHIP_K_VQ_HEATMAP, &e0);
  hipLaunchKernelGGL(vq_filter_kernel, grid, dim3(256), p.lds, ctx->stream, codes, H, W, tab_dev, n_tmpl, S, p.planes);
  hipLaunchKernelGGL(vq_combine_kernel, dim3((unsigned)pairs), dim3(256), 0, ctx->stream, (const double*)S, H, W, tab_dev, n_tmpl,
                     p.planes, heat, minima);
  if (ctx->profiling) mhip_prof_end(ctx, MHIP_K_VQ_HEATMAP, e0);
  CHECK_LAUNCH(ctx, "vq_heatmap");
  return MHIP_OK;
}

int vq_launch_peaks(mhip_ctx* ctx, float* heat, int H, int W, const VqTmplDev* tab_dev, int n_tmpl, int pairs, int max_objects,
                    float* peaks) {
  for (int k = 0; k < max_objects; ++k)
    PROF_LAUNCH(ctx, MHIP_K_VQ_PEAKS, hipLaunchKernelGGL(vq_peaks_kernel, dim3((unsigned)pairs), dim3(256), 0, ctx->stream, heat, H,
                                                         W, tab_dev, n_tmpl, k, max_objects, peaks));
  CHECK_LAUNCH(ctx, "vq_peaks");
  return MHIP_OK;
}

// one iteration on device buffers: labels <- assignment against cent_old, cent_new / counts / err_part <- update
int vq_kmeans_step(mhip_ctx* ctx, const uint8_t* img, size_t pitch, int H, int W, const int32_t* rect, const VqTmplDev* tab_dev,
                   int K, const float* cent_old, float* cent_new, uint8_t* labels, int32_t* counts, float* err_part) {
  int rc = vq_launch_assign(ctx, img, pitch, nullptr, H, W, rect, tab_dev, 1, 1, labels);
  if (rc) return rc;
  PROF_LAUNCH(ctx, MHIP_K_VQ_KMEANS, hipLaunchKernelGGL(vq_kmeans_update_kernel, dim3((unsigned)K), dim3(256), 0, ctx->stream, img,
                                                        pitch, H, W, rect[0], rect[1], rect[2], rect[3], (const uint8_t*)labels,
                                                        cent_old, cent_new, counts, err_part));
  CHECK_LAUNCH(ctx, "vq_kmeans_update");
  return MHIP_OK;
}

// error = sum over the clusters, in their order
double vq_error(const float* err_part, int K) {
  double e = 0.0;
  for (int k = 0; k < K; ++k) e += (double)err_part[k];
  return e;
}

}  // namespace

struct mhip_vq_template {
  mhip_ctx* ctx = nullptr;
  int K = 0, bw = 0, bh = 0, iters = 0;
  float* dev = nullptr;             // codebook [VQ_MAXK][27], then responses [VQ_NF][VQ_MAXK]
  std::vector<uint8_t> labels;
  std::vector<float> codebook;
  VqTmplDev entry{};
  bool filters_set = false;
};

extern "C" int mhip_vq_template_create(mhip_ctx* ctx, const uint8_t* frame, int on_device, int H, int W, const int32_t* box,
                                       const int32_t* init_idx, int n_init, mhip_vq_template** out) {
  if (!ctx) return MHIP_EINVAL;
  if (!frame || !init_idx || !out || H <= 0 || W <= 0) return mhip_fail(ctx, MHIP_EINVAL, "vq_template_create: null argument");
  if (!vq_rect_ok(box, H, W)) return mhip_fail(ctx, MHIP_EINVAL, "vq_template_create: the box is outside the %d x %d frame", H, W);
  const int n = box[2] * box[3], K = n > VQ_MAXK ? VQ_MAXK : n;
  if (n_init != K) return mhip_fail(ctx, MHIP_EINVAL, "vq_template_create: %d initial centroids for %d codes", n_init, K);
  for (int k = 0; k < K; ++k)
    if (init_idx[k] < 0 || init_idx[k] >= n) return mhip_fail(ctx, MHIP_EINVAL, "vq_template_create: initial index outside the box");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t fb = (size_t)H * W * 3;
  uint8_t *img = nullptr, *labels = nullptr;
  float* cent[2] = {nullptr, nullptr};
  float* err = nullptr;
  int32_t *counts = nullptr, *idx = nullptr;
  VqTmplDev* tab = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    img = ws.take<uint8_t>(on_device ? 0 : fb);
    labels = ws.take<uint8_t>(n);
    cent[0] = ws.take<float>(sizeof(float) * VQ_MAXK * VQ_F);
    cent[1] = ws.take<float>(sizeof(float) * VQ_MAXK * VQ_F);
    err = ws.take<float>(sizeof(float) * VQ_MAXK);
    counts = ws.take<int32_t>(sizeof(int32_t) * VQ_MAXK);
    idx = ws.take<int32_t>(sizeof(int32_t) * VQ_MAXK);
    tab = ws.take<VqTmplDev>(sizeof(VqTmplDev) * 2);
  });
  if (rc) return rc;
  const uint8_t* src = frame;
  if (!on_device) {
    MHIP_HIP(ctx, hipMemcpyAsync(img, frame, fb, hipMemcpyHostToDevice, ctx->stream));
    src = img;
  }
  const size_t pitch = (size_t)W * 3;
  if ((rc = mhip_stage_h2d(ctx, idx, init_idx, sizeof(int32_t) * K))) return rc;
  VqTmplDev host_tab[2] = {};
  for (int b = 0; b < 2; ++b) { host_tab[b].codebook = cent[b]; host_tab[b].K = K; }
  if ((rc = mhip_stage_h2d(ctx, tab, host_tab, sizeof(host_tab)))) return rc;
  PROF_LAUNCH(ctx, MHIP_K_VQ_KMEANS, hipLaunchKernelGGL(vq_gather_kernel, dim3(1), dim3(VQ_MAXK), 0, ctx->stream, src, pitch, H, W,
                                                        box[0], box[1], box[2], (const int32_t*)idx, K, cent[0]));
  CHECK_LAUNCH(ctx, "vq_gather");
  std::vector<float> err_host(K);
  int cur = 0, iters = 0;
  for (int it = 0; it < VQ_MAX_ITER; ++it) {
    if ((rc = vq_kmeans_step(ctx, src, pitch, H, W, box, tab + cur, K, cent[cur], cent[cur ^ 1], labels, counts, err))) return rc;
    MHIP_HIP(ctx, hipMemcpyAsync(err_host.data(), err, sizeof(float) * K, hipMemcpyDeviceToHost, ctx->stream));
    MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    cur ^= 1;
    iters = it + 1;
    if (vq_error(err_host.data(), K) <= VQ_TOL) break;
  }
  mhip_vq_template* t = new mhip_vq_template();
  t->ctx = ctx; t->K = K; t->bw = box[2]; t->bh = box[3]; t->iters = iters;
  t->labels.resize(n);
  t->codebook.resize((size_t)K * VQ_F);
  if (hipMalloc(&t->dev, sizeof(float) * (VQ_MAXK * VQ_F + VQ_NF * VQ_MAXK)) != hipSuccess) {
    (void)hipGetLastError();
    delete t;
    return mhip_fail(ctx, MHIP_ENOMEM, "vq_template_create: device allocation failed");
  }
  hipError_t e = hipMemcpyAsync(t->dev, cent[cur], sizeof(float) * K * VQ_F, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t->codebook.data(), cent[cur], sizeof(float) * K * VQ_F, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t->labels.data(), labels, n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(t->dev);
    delete t;
    return mhip_fail(ctx, MHIP_EHIP, "vq_template_create: %s", hipGetErrorString(e));
  }
  t->entry.codebook = t->dev;
  t->entry.resp = t->dev + VQ_MAXK * VQ_F;
  t->entry.K = K; t->entry.bw = t->bw; t->entry.bh = t->bh;
  *out = t;
  return MHIP_OK;
}

extern "C" int mhip_vq_template_destroy(mhip_vq_template* t) {
  if (!t) return MHIP_OK;
  mhip_quiesce(t->ctx);
  if (t->dev) (void)hipFree(t->dev);
  delete t;
  return MHIP_OK;
}

extern "C" int mhip_vq_template_state(mhip_vq_template* t, int* n_codes, int* iterations, uint8_t* labels_out,
                                      float* codebook_out) {
  if (!t) return MHIP_EINVAL;
  if (n_codes) *n_codes = t->K;
  if (iterations) *iterations = t->iters;
  if (labels_out) memcpy(labels_out, t->labels.data(), t->labels.size());
  if (codebook_out) memcpy(codebook_out, t->codebook.data(), sizeof(float) * t->codebook.size());
  return MHIP_OK;
}

extern "C" int mhip_vq_template_set_filters(mhip_vq_template* t, const float* responses, const mhip_vq_filters* filters) {
  if (!t) return MHIP_EINVAL;
  mhip_ctx* ctx = t->ctx;
  if (!responses || !filters) return mhip_fail(ctx, MHIP_EINVAL, "vq_template_set_filters: null argument");
  int rc = vq_fill_filters(ctx, &t->entry, filters, responses, t->K);
  if (rc) return rc;
  std::vector<float> resp((size_t)VQ_NF * VQ_MAXK, 0.f);
  for (int f = 0; f < filters->n; ++f) memcpy(&resp[(size_t)f * VQ_MAXK], responses + (size_t)f * t->K, sizeof(float) * t->K);
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  MHIP_HIP(ctx, hipMemcpyAsync(t->dev + VQ_MAXK * VQ_F, resp.data(), sizeof(float) * resp.size(), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  t->filters_set = true;
  return MHIP_OK;
}

extern "C" int mhip_vq_match(mhip_ctx* ctx, const uint8_t* page_dev, int page_h, int page_w, size_t page_pitch,
                             const int32_t* win_xy, int n_win, int win_h, int win_w, mhip_vq_template* const* templates,
                             int n_templates, int max_objects, float* peaks_out) {
  if (!ctx) return MHIP_EINVAL;
  if (!page_dev || !win_xy || !templates || !peaks_out) return mhip_fail(ctx, MHIP_EINVAL, "vq_match: null argument");
  if (n_win < 1 || n_templates < 1 || max_objects < 1 || win_h < 1 || win_w < 1 || page_pitch < (size_t)page_w * 3)
    return mhip_fail(ctx, MHIP_EINVAL, "vq_match: bad shape");
  for (int i = 0; i < n_win; ++i)
    if (win_xy[2 * i] < 0 || win_xy[2 * i + 1] < 0 || win_xy[2 * i] + win_w > page_w || win_xy[2 * i + 1] + win_h > page_h)
      return mhip_fail(ctx, MHIP_EINVAL, "vq_match: window %d is outside the %d x %d page", i, page_h, page_w);
  std::vector<VqTmplDev> tab(n_templates);
  for (int k = 0; k < n_templates; ++k) {
    if (!templates[k] || templates[k]->ctx != ctx || !templates[k]->filters_set)
      return mhip_fail(ctx, MHIP_ESTATE, "vq_match: template %d has no filters, or lives on another context", k);
    tab[k] = templates[k]->entry;
  }
  VqPlan plan;
  int rc = vq_plan(ctx, tab.data(), n_templates, win_h, win_w, &plan);
  if (rc) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  // windows per round: the fp64 planes of a round stay under 512 MiB, and a grid dimension under 65536
  const size_t cells = (size_t)win_h * win_w;
  const size_t per_win = (size_t)n_templates * cells * (1 + sizeof(float) + sizeof(double) * plan.planes);
  const int by_mem = (int)std::max<size_t>(1, ((size_t)512 << 20) / per_win);
  if (n_templates > 65535) return mhip_fail(ctx, MHIP_EINVAL, "vq_match: too many templates");
  const int chunk = std::max(1, std::min({n_win, by_mem, 65535 / n_templates}));
  VqTmplDev* tab_dev = nullptr;
  int32_t* xy_dev = nullptr;
  uint8_t* codes = nullptr;
  double* S = nullptr;
  float *heat = nullptr, *peaks = nullptr;
  const size_t peak_floats = (size_t)n_win * n_templates * max_objects * 3;
  rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    tab_dev = ws.take<VqTmplDev>(sizeof(VqTmplDev) * n_templates);
    xy_dev = ws.take<int32_t>(sizeof(int32_t) * 2 * n_win);
    peaks = ws.take<float>(sizeof(float) * peak_floats);
    codes = ws.take<uint8_t>((size_t)chunk * n_templates * cells);
    heat = ws.take<float>(sizeof(float) * chunk * n_templates * cells);
    S = ws.take<double>(sizeof(double) * chunk * n_templates * plan.planes * cells);
  });
  if (rc) return rc;
  if ((rc = mhip_stage_h2d(ctx, tab_dev, tab.data(), sizeof(VqTmplDev) * n_templates))) return rc;
  if ((rc = mhip_stage_h2d(ctx, xy_dev, win_xy, sizeof(int32_t) * 2 * n_win))) return rc;
  const int32_t rect[4] = {0, 0, win_w, win_h};
  for (int w0 = 0; w0 < n_win; w0 += chunk) {
    const int pairs = std::min(chunk, n_win - w0) * n_templates;
    if ((rc = vq_launch_assign(ctx, page_dev, page_pitch, xy_dev + 2 * w0, win_h, win_w, rect, tab_dev, n_templates, pairs, codes)))
      return rc;
    if ((rc = vq_launch_heatmap(ctx, codes, win_h, win_w, tab_dev, n_templates, pairs, plan, S, heat, nullptr))) return rc;
    if ((rc = vq_launch_peaks(ctx, heat, win_h, win_w, tab_dev, n_templates, pairs, max_objects,
                              peaks + (size_t)w0 * n_templates * max_objects * 3)))
      return rc;
  }
  MHIP_HIP(ctx, hipMemcpyAsync(peaks_out, peaks, sizeof(float) * peak_floats, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

// ------------------------------------------------------------------------------------------------------------ host entries
extern "C" int mhip_vq_assign_host(mhip_ctx* ctx, const uint8_t* image, int H, int W, const int32_t* rect, const float* codebook,
                                   int n_codes, uint8_t* codes_out) {
  if (!ctx) return MHIP_EINVAL;
  if (!image || !codebook || !codes_out || H <= 0 || W <= 0) return mhip_fail(ctx, MHIP_EINVAL, "vq_assign: null argument");
  if (!vq_rect_ok(rect, H, W) || n_codes < 1 || n_codes > VQ_MAXK) return mhip_fail(ctx, MHIP_EINVAL, "vq_assign: bad rectangle or code count");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t fb = (size_t)H * W * 3, n = (size_t)rect[2] * rect[3];
  uint8_t *img = nullptr, *codes = nullptr;
  float* cb = nullptr;
  VqTmplDev* tab = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    img = ws.take<uint8_t>(fb); codes = ws.take<uint8_t>(n);
    cb = ws.take<float>(sizeof(float) * VQ_MAXK * VQ_F); tab = ws.take<VqTmplDev>(sizeof(VqTmplDev));
  });
  if (rc) return rc;
  VqTmplDev e{};
  e.codebook = cb; e.K = n_codes;
  MHIP_HIP(ctx, hipMemcpyAsync(img, image, fb, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(cb, codebook, sizeof(float) * n_codes * VQ_F, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_stage_h2d(ctx, tab, &e, sizeof(e)))) return rc;
  if ((rc = vq_launch_assign(ctx, img, (size_t)W * 3, nullptr, H, W, rect, tab, 1, 1, codes))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(codes_out, codes, n, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_vq_kmeans_step_host(mhip_ctx* ctx, const uint8_t* image, int H, int W, const int32_t* rect,
                                        const float* centroids_in, int n_codes, uint8_t* labels_out, float* centroids_out,
                                        int32_t* counts_out, double* error_out) {
  if (!ctx) return MHIP_EINVAL;
  if (!image || !centroids_in || !labels_out || !centroids_out || !counts_out || !error_out || H <= 0 || W <= 0)
    return mhip_fail(ctx, MHIP_EINVAL, "vq_kmeans_step: null argument");
  if (!vq_rect_ok(rect, H, W) || n_codes < 1 || n_codes > VQ_MAXK) return mhip_fail(ctx, MHIP_EINVAL, "vq_kmeans_step: bad rectangle or code count");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t fb = (size_t)H * W * 3, n = (size_t)rect[2] * rect[3];
  uint8_t *img = nullptr, *labels = nullptr;
  float *c0 = nullptr, *c1 = nullptr, *err = nullptr;
  int32_t* counts = nullptr;
  VqTmplDev* tab = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    img = ws.take<uint8_t>(fb); labels = ws.take<uint8_t>(n);
    c0 = ws.take<float>(sizeof(float) * VQ_MAXK * VQ_F); c1 = ws.take<float>(sizeof(float) * VQ_MAXK * VQ_F);
    err = ws.take<float>(sizeof(float) * VQ_MAXK); counts = ws.take<int32_t>(sizeof(int32_t) * VQ_MAXK);
    tab = ws.take<VqTmplDev>(sizeof(VqTmplDev));
  });
  if (rc) return rc;
  VqTmplDev e{};
  e.codebook = c0; e.K = n_codes;
  MHIP_HIP(ctx, hipMemcpyAsync(img, image, fb, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(c0, centroids_in, sizeof(float) * n_codes * VQ_F, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_stage_h2d(ctx, tab, &e, sizeof(e)))) return rc;
  if ((rc = vq_kmeans_step(ctx, img, (size_t)W * 3, H, W, rect, tab, n_codes, c0, c1, labels, counts, err))) return rc;
  std::vector<float> err_host(n_codes);
  MHIP_HIP(ctx, hipMemcpyAsync(labels_out, labels, n, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(centroids_out, c1, sizeof(float) * n_codes * VQ_F, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(counts_out, counts, sizeof(int32_t) * n_codes, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(err_host.data(), err, sizeof(float) * n_codes, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *error_out = vq_error(err_host.data(), n_codes);
  return MHIP_OK;
}

extern "C" int mhip_vq_heatmap_host(mhip_ctx* ctx, const uint8_t* codes, int H, int W, int n_codes, const float* responses,
                                    const mhip_vq_filters* filters, float* heat_out, double* minima_out) {
  if (!ctx) return MHIP_EINVAL;
  if (!codes || !responses || !filters || !heat_out || H <= 0 || W <= 0) return mhip_fail(ctx, MHIP_EINVAL, "vq_heatmap: null argument");
  if (n_codes < 1 || n_codes > VQ_MAXK) return mhip_fail(ctx, MHIP_EINVAL, "vq_heatmap: 1..%d codes", VQ_MAXK);
  const size_t cells = (size_t)H * W;
  for (size_t i = 0; i < cells; ++i)
    if (codes[i] >= n_codes) return mhip_fail(ctx, MHIP_EINVAL, "vq_heatmap: code %d of %d", (int)codes[i], n_codes);
  VqTmplDev e{};
  e.K = n_codes;
  int rc = vq_fill_filters(ctx, &e, filters, responses, n_codes);
  if (rc) return rc;
  VqPlan plan;
  if ((rc = vq_plan(ctx, &e, 1, H, W, &plan))) return rc;
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  uint8_t* cd = nullptr;
  float *resp = nullptr, *heat = nullptr;
  double *S = nullptr, *mins = nullptr;
  VqTmplDev* tab = nullptr;
  rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    cd = ws.take<uint8_t>(cells); resp = ws.take<float>(sizeof(float) * VQ_NF * VQ_MAXK);
    heat = ws.take<float>(sizeof(float) * cells); S = ws.take<double>(sizeof(double) * plan.planes * cells);
    mins = ws.take<double>(sizeof(double) * VQ_NF); tab = ws.take<VqTmplDev>(sizeof(VqTmplDev));
  });
  if (rc) return rc;
  std::vector<float> rh((size_t)VQ_NF * VQ_MAXK, 0.f);
  for (int f = 0; f < filters->n; ++f) memcpy(&rh[(size_t)f * VQ_MAXK], responses + (size_t)f * n_codes, sizeof(float) * n_codes);
  e.resp = resp;
  MHIP_HIP(ctx, hipMemcpyAsync(cd, codes, cells, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_stage_h2d(ctx, resp, rh.data(), sizeof(float) * rh.size()))) return rc;
  if ((rc = mhip_stage_h2d(ctx, tab, &e, sizeof(e)))) return rc;
  if ((rc = vq_launch_heatmap(ctx, cd, H, W, tab, 1, 1, plan, S, heat, mins))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(heat_out, heat, sizeof(float) * cells, hipMemcpyDeviceToHost, ctx->stream));
  if (minima_out) MHIP_HIP(ctx, hipMemcpyAsync(minima_out, mins, sizeof(double) * filters->n, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_vq_peaks_host(mhip_ctx* ctx, float* heat, int n, int H, int W, const int32_t* box_wh, int max_objects,
                                  float* peaks_out) {
  if (!ctx) return MHIP_EINVAL;
  if (!heat || !box_wh || !peaks_out || n < 1 || n > 65535 || H <= 0 || W <= 0 || max_objects < 1)
    return mhip_fail(ctx, MHIP_EINVAL, "vq_peaks: bad argument");
  std::vector<VqTmplDev> tab(n);
  for (int i = 0; i < n; ++i) {
    if (box_wh[2 * i] < 1 || box_wh[2 * i + 1] < 1) return mhip_fail(ctx, MHIP_EINVAL, "vq_peaks: empty box");
    tab[i] = VqTmplDev{};
    tab[i].bw = box_wh[2 * i]; tab[i].bh = box_wh[2 * i + 1];
  }
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t cells = (size_t)n * H * W, pf = (size_t)n * max_objects * 3;
  float *hd = nullptr, *pk = nullptr;
  VqTmplDev* tab_dev = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    hd = ws.take<float>(sizeof(float) * cells); pk = ws.take<float>(sizeof(float) * pf);
    tab_dev = ws.take<VqTmplDev>(sizeof(VqTmplDev) * n);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(hd, heat, sizeof(float) * cells, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mhip_stage_h2d(ctx, tab_dev, tab.data(), sizeof(VqTmplDev) * n))) return rc;
  if ((rc = vq_launch_peaks(ctx, hd, H, W, tab_dev, n, n, max_objects, pk))) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(heat, hd, sizeof(float) * cells, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(peaks_out, pk, sizeof(float) * pf, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_clip_cosine_host(mhip_ctx* ctx, const uint8_t* a, const uint8_t* b, int n, int h, int w, float* out) {
  if (!ctx) return MHIP_EINVAL;
  if (!a || !b || !out || n < 1 || h < 1 || w < 1 || (long long)h * w * 3 > (1ll << 26))   // the sums stay inside 64 bits
    return mhip_fail(ctx, MHIP_EINVAL, "clip_cosine: bad argument");
  MHIP_HIP(ctx, hipSetDevice(ctx->device));
  const int bytes = h * w * 3;
  const size_t total = (size_t)n * bytes;
  uint8_t *ad = nullptr, *bd = nullptr;
  float* od = nullptr;
  int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
    ad = ws.take<uint8_t>(total); bd = ws.take<uint8_t>(total); od = ws.take<float>(sizeof(float) * n);
  });
  if (rc) return rc;
  MHIP_HIP(ctx, hipMemcpyAsync(ad, a, total, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipMemcpyAsync(bd, b, total, hipMemcpyHostToDevice, ctx->stream));
  PROF_LAUNCH(ctx, MHIP_K_CLIP_COSINE, hipLaunchKernelGGL(clip_cosine_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream,
                                                          (const uint8_t*)ad, (const uint8_t*)bd, bytes, od));
  CHECK_LAUNCH(ctx, "clip_cosine");
  MHIP_HIP(ctx, hipMemcpyAsync(out, od, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}
