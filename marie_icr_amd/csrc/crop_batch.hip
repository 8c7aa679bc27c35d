// crop_batch.hip — the recognizer's line/word crop batcher on the GPU, bit-exact with Pillow.
//
// Replaces, per fragment: cv2 BGR->RGB + Image.fromarray(...).convert("L")
// (marie/models/icr/memory_dataset.py:40-55), the aspect-preserving
// image.resize((w', 32), Image.BICUBIC) and NormalizePAD's right-edge replication
// (marie/models/icr/dataset.py:275-324).  The /255, -0.5, /0.5 normalisation is fused into the recognizer's
// first conv kernel (conv_first.hip), so this stage writes uint8.
//
// Pillow's 8-bit resampling is integer work: per output pixel a short filter window whose weights are
// bicubic(a = -0.5) values normalised in double precision and rounded to 22-bit fixed point, a horizontal pass
// rounded to uint8, then a vertical pass (libImaging/Resample.c).  Each thread owns one output pixel and rebuilds
// its (<= 2*ceil(2*scale)+1) weights itself in IEEE double with FMA contraction off — identical to the C code
// Pillow runs — so no coefficient tables cross PCIe and the kernels are pure gather + integer MAC:
//   pass 1: BGR (or gray) fragment  -> tmp  [h][w']   (gray conversion fused: (R*19595+G*38470+B*7471+0x8000)>>16)
//   pass 2: tmp                     -> out  [32][imgW] with the last column replicated to imgW.
#include "pil_resample.h"   // the arithmetic, and #pragma clang fp contract(off) for everything below

namespace {

struct CropDev {
  unsigned long long src_off;  // byte offset of the fragment's first pixel in `base`
  unsigned long long tmp_off;  // byte offset of its [h][rw] intermediate in `tmp`
  int h, w, row_stride, channels, rw;
};

// pass 1: horizontal resample (+ gray conversion).  grid = (ceil(maxrw*maxh / 256), n)
__global__ __launch_bounds__(256) void crop_hpass_kernel(const uint8_t* __restrict__ base,
                                                         const CropDev* __restrict__ descs,
                                                         uint8_t* __restrict__ tmp) {
  const CropDev d = descs[blockIdx.y];
  const int total = d.h * d.rw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int yy = i / d.rw, xx = i - yy * d.rw;
    const uint8_t* row = base + d.src_off + (size_t)yy * d.row_stride;
    const PilWindow win = window(MHIP_PIL_BICUBIC, d.w, d.rw, xx);
    int acc = 1 << (PRECISION_BITS - 1);
    for (int x = 0; x < win.n; ++x) {
      const int k = fixed_weight(MHIP_PIL_BICUBIC, win, x);
      int g;
      if (d.channels == 3) {
        const uint8_t* p = row + (size_t)(x + win.xmin) * 3;   // B, G, R
        g = (int)(((unsigned)p[2] * 19595u + (unsigned)p[1] * 38470u + (unsigned)p[0] * 7471u + 0x8000u) >> 16);
      } else {
        g = row[x + win.xmin];
      }
      acc += g * k;
    }
    tmp[d.tmp_off + (size_t)yy * d.rw + xx] = clip8(acc);
  }
}

// pass 2: vertical resample to out_h rows + replicate the last column up to img_w.  grid = (ceil(out_h*img_w/256), n)
__global__ __launch_bounds__(256) void crop_vpass_kernel(const uint8_t* __restrict__ tmp,
                                                         const CropDev* __restrict__ descs, uint8_t* __restrict__ out,
                                                         int out_h, int img_w) {
  const CropDev d = descs[blockIdx.y];
  const int total = out_h * img_w;
  uint8_t* o = out + (size_t)blockIdx.y * total;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int yy = i / img_w, xo = i - yy * img_w;
    const int xx = xo < d.rw ? xo : d.rw - 1;   // NormalizePAD: columns beyond the resized width repeat the last one
    const PilWindow win = window(MHIP_PIL_BICUBIC, d.h, out_h, yy);
    int acc = 1 << (PRECISION_BITS - 1);
    const uint8_t* col = tmp + d.tmp_off + xx;
    for (int y = 0; y < win.n; ++y) acc += (int)col[(size_t)(y + win.xmin) * d.rw] * fixed_weight(MHIP_PIL_BICUBIC, win, y);
    o[i] = clip8(acc);
  }
}

}  // namespace

// Host: AlignCollate's width rule (marie/models/icr/dataset.py:313-318), same double arithmetic as CPython.
int mhip_crop_resized_width(int w, int h, int img_h, int img_w) {
  const double ratio = (double)w / (double)h;
  const double c = ceil((double)img_h * ratio);
  int rw = (c > (double)img_w) ? img_w : (int)c;
  return rw < 1 ? 1 : rw;
}

namespace {

// the scratch of mhip_launch_crop_batch: the CropDev table the kernels read and the [h][rw] intermediates behind it.  Sized with
// a null base, placed on the caller's scratch otherwise; `host` is the table's content either way.
struct CropScratch {
  CropDev* table;
  uint8_t* tmp;
  std::vector<CropDev> host;
  int max_hrw = 1;
};
void crop_carve(Carver& c, const mhip_crop_desc* descs, int n, int img_h, int img_w, CropScratch* s) {
  s->host.resize((size_t)n);
  size_t tmp_bytes = 0;
  for (int i = 0; i < n; ++i) {
    CropDev& d = s->host[i];
    d.src_off = descs[i].src_offset;
    d.h = descs[i].h; d.w = descs[i].w; d.row_stride = descs[i].row_stride; d.channels = descs[i].channels;
    d.rw = mhip_crop_resized_width(d.w, d.h, img_h, img_w);
    d.tmp_off = tmp_bytes;
    tmp_bytes += ((size_t)d.h * d.rw + 15) / 16 * 16;
    s->max_hrw = std::max(s->max_hrw, d.h * d.rw);
  }
  s->table = c.take<CropDev>((size_t)n * sizeof(CropDev));
  s->tmp = c.take<uint8_t>(tmp_bytes);
}

}  // namespace

size_t mhip_crop_scratch_bytes(const mhip_crop_desc* descs, int n, int img_h, int img_w) {
  CropScratch s;
  return mhip_layout_bytes([&](Carver& c) { crop_carve(c, descs, n, img_h, img_w, &s); });
}

// descs: n x {src_off, h, w, row_stride, channels} on the host.  scratch_dev must hold mhip_crop_scratch_bytes().
int mhip_launch_crop_batch(mhip_ctx* ctx, const uint8_t* base_dev, const mhip_crop_desc* descs, int n, int img_h,
                           int img_w, void* scratch_dev, uint8_t* out_dev) {
  if (n < 1 || img_h < 1 || img_w < 1 || !descs || !base_dev || !scratch_dev || !out_dev)
    return mhip_fail(ctx, MHIP_EINVAL, "crop_batch: bad arguments");
  for (int i = 0; i < n; ++i) {
    const mhip_crop_desc& s = descs[i];
    if (s.h < 1 || s.w < 1 || (s.channels != 1 && s.channels != 3) || s.row_stride < s.w * s.channels)
      return mhip_fail(ctx, MHIP_EINVAL, "crop_batch: bad fragment %d (%dx%d, %d ch, stride %d)", i, s.h, s.w,
                       s.channels, s.row_stride);
  }
  Carver c(scratch_dev);
  CropScratch s;
  crop_carve(c, descs, n, img_h, img_w, &s);
  // the table is a host temporary: a plain copy and a drain of the stream (not the pinned staging ring of mhip_stage_h2d)
  MHIP_HIP(ctx, hipMemcpyAsync(s.table, s.host.data(), (size_t)n * sizeof(CropDev), hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // s.host dies with this scope
  hipEvent_t e0 = nullptr;
  if (ctx->profiling) mhip_prof_begin(ctx, MHIP_K_CROP_BATCH, &e0);
  const unsigned gx1 = (unsigned)std::min((s.max_hrw + 255) / 256, 64);
  hipLaunchKernelGGL(crop_hpass_kernel, dim3(gx1, n), dim3(256), 0, ctx->stream, base_dev, s.table, s.tmp);
  const unsigned gx2 = (unsigned)std::min((img_h * img_w + 255) / 256, 64);
  hipLaunchKernelGGL(crop_vpass_kernel, dim3(gx2, n), dim3(256), 0, ctx->stream, s.tmp, s.table, out_dev, img_h, img_w);
  if (ctx->profiling) mhip_prof_end(ctx, MHIP_K_CROP_BATCH, e0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mhip_fail(ctx, MHIP_EHIP, "crop_batch launch: %s", hipGetErrorString(e));
  return 0;
}
