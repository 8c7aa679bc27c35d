// context.hip — the context behind the C ABI of include/marie_hip.h: errors, init / destroy, stream, pinned staging, the
// grow-only workspace (every call lays itself out in it through mhip_carve_workspace, common.h), profiling, device info.
#include <stdarg.h>

#include <algorithm>

#include "common.h"

int mhip_fail(mhip_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

static const char* kKernelNames[MHIP_K_COUNT] = {"conv_first", "conv_igemm", "lstm_rec",   "ctc_decode",
                                                 "image_ops",  "ccl",        "crop_batch", "attn",
                                                 "attn_flash", "vit_ops",    "det_ops",    "dec_ops",
                                                 "conv_igemm<64>", "conv_igemm<128>", "conv_igemm<256>", "conv_igemm<1128>",
                                                 "conv3x3_patch", "cross_attn", "attn_bias",
                                                 "vq_assign", "vq_kmeans", "vq_heatmap", "vq_peaks", "clip_cosine",
                                                 "clipvis_patchify", "clipvis_embed", "quick_gelu", "clipvis_head", "pair_cosine",
                                                 "cliptext_embed", "attn_causal", "lev_ngrams",
                                                 "attn_short", "berttext_embed", "geglu", "berttext_pool"};

extern "C" int mhip_kernel_count(void) { return MHIP_K_COUNT; }
extern "C" const char* mhip_kernel_name(int k) { return (k >= 0 && k < MHIP_K_COUNT) ? kKernelNames[k] : ""; }

extern "C" int mhip_init(int device_id, mhip_ctx** out) {
  if (!out) return MHIP_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MHIP_EHIP;
  if (device_id < 0 || device_id >= ndev) return MHIP_EINVAL;
  if (hipSetDevice(device_id) != hipSuccess) return MHIP_EHIP;
  mhip_ctx* ctx = new mhip_ctx();
  ctx->device = device_id;
  for (int k = MHIP_K_IGEMM_T64; k <= MHIP_K_IGEMM_PATCH; ++k) ctx->prof[k].parent = MHIP_K_CONV_IGEMM;
  if (hipMalloc(&ctx->zeros, MHIP_ZERO_BYTES) != hipSuccess || hipMemset(ctx->zeros, 0, MHIP_ZERO_BYTES) != hipSuccess) {
    delete ctx;
    return MHIP_ENOMEM;
  }
  *out = ctx;
  return MHIP_OK;
}

extern "C" int mhip_destroy(mhip_ctx* ctx) {
  if (!ctx) return MHIP_OK;
  (void)hipSetDevice(ctx->device);
  mhip_quiesce(ctx);
  for (auto& s : ctx->prof)
    for (auto& p : s.pending) {
      (void)hipEventDestroy(p.first);
      (void)hipEventDestroy(p.second);
    }
  for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
  for (int i = 0; i < mhip_ctx::PinnedRing::N; ++i) {
    if (ctx->stage.ev[i]) (void)hipEventDestroy(ctx->stage.ev[i]);
    if (ctx->stage.buf[i]) (void)hipHostFree(ctx->stage.buf[i]);
  }
  if (ctx->ws) (void)hipFree(ctx->ws);
  if (ctx->zeros) (void)hipFree(ctx->zeros);
  delete ctx;
  return MHIP_OK;
}

int mhip_stage_h2d(mhip_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
  if (!bytes) return MHIP_OK;
  mhip_ctx::PinnedRing& r = ctx->stage;
  const int i = r.next;
  r.next = (i + 1) % mhip_ctx::PinnedRing::N;
  if (r.ev[i]) MHIP_HIP(ctx, hipEventSynchronize(r.ev[i]));          // the copy that last read this buffer (four calls ago) is done
  else MHIP_HIP(ctx, hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming));
  if (bytes > r.cap[i]) {
    if (r.buf[i]) (void)hipHostFree(r.buf[i]);
    r.buf[i] = nullptr; r.cap[i] = 0;
    const size_t cap = std::max<size_t>(bytes, 64 * 1024);
    MHIP_HIP(ctx, hipHostMalloc(&r.buf[i], cap, hipHostMallocDefault));
    r.cap[i] = cap;
  }
  memcpy(r.buf[i], src_host, bytes);
  MHIP_HIP(ctx, hipMemcpyAsync(dst_dev, r.buf[i], bytes, hipMemcpyHostToDevice, ctx->stream));
  MHIP_HIP(ctx, hipEventRecord(r.ev[i], ctx->stream));
  return MHIP_OK;
}

extern "C" const char* mhip_last_error(mhip_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

extern "C" int mhip_set_stream(mhip_ctx* ctx, void* s) {
  if (!ctx) return MHIP_EINVAL;
  ctx->stream = (hipStream_t)s;
  return MHIP_OK;
}

extern "C" int mhip_synchronize(mhip_ctx* ctx) {
  if (!ctx) return MHIP_EINVAL;
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MHIP_OK;
}

extern "C" int mhip_device_info(mhip_ctx* ctx, char* arch, size_t arch_len, int* cu_count, size_t* hbm_bytes) {
  if (!ctx) return MHIP_EINVAL;
  hipDeviceProp_t p;
  MHIP_HIP(ctx, hipGetDeviceProperties(&p, ctx->device));
  if (arch && arch_len) {
    strncpy(arch, p.gcnArchName, arch_len - 1);
    arch[arch_len - 1] = 0;
  }
  if (cu_count) *cu_count = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = p.totalGlobalMem;
  return MHIP_OK;
}

extern "C" int mhip_memcpy_dev(mhip_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return MHIP_EINVAL;
  MHIP_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return MHIP_OK;
}

int mhip_ensure_workspace(mhip_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->ws_bytes) return MHIP_OK;
  MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->ws) MHIP_HIP(ctx, hipFree(ctx->ws));
  ctx->ws = nullptr;
  ctx->ws_bytes = 0;
  size_t want = bytes + bytes / 8;
  if (hipMalloc(&ctx->ws, want) != hipSuccess) {
    (void)hipGetLastError();
    return mhip_fail(ctx, MHIP_ENOMEM, "workspace allocation of %zu bytes failed", want);
  }
  ctx->ws_bytes = want;
  return MHIP_OK;
}

// ------------------------------------------------------------------ profiling
static hipEvent_t get_event(mhip_ctx* ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
void mhip_prof_begin(mhip_ctx* ctx, int kid, hipEvent_t* e0) {
  (void)kid;
  *e0 = get_event(ctx);
  (void)hipEventRecord(*e0, ctx->stream);
}
void mhip_prof_end(mhip_ctx* ctx, int kid, hipEvent_t e0) {
  hipEvent_t e1 = get_event(ctx);
  (void)hipEventRecord(e1, ctx->stream);
  ctx->prof[kid].pending.emplace_back(e0, e1);
}
static void prof_drain(mhip_ctx* ctx) {
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& s : ctx->prof) {
    for (auto& p : s.pending) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
        s.total_ms += ms;
        s.launches += 1;
        if (s.parent >= 0) {
          ctx->prof[s.parent].total_ms += ms;
          ctx->prof[s.parent].launches += 1;
        }
      }
      ctx->event_pool.push_back(p.first);
      ctx->event_pool.push_back(p.second);
    }
    s.pending.clear();
  }
}
extern "C" int mhip_profile_enable(mhip_ctx* ctx, int enable) {
  if (!ctx) return MHIP_EINVAL;
  if (!enable) prof_drain(ctx);
  ctx->profiling = enable != 0;
  return MHIP_OK;
}
extern "C" int mhip_profile_reset(mhip_ctx* ctx) {
  if (!ctx) return MHIP_EINVAL;
  prof_drain(ctx);
  for (auto& s : ctx->prof) {
    s.total_ms = 0;
    s.launches = 0;
    s.flops = 0;
  }
  return MHIP_OK;
}
extern "C" int mhip_profile_flops(mhip_ctx* ctx, int kid, double* flops) {
  if (!ctx || kid < 0 || kid >= MHIP_K_COUNT || !flops) return MHIP_EINVAL;
  *flops = ctx->prof[kid].flops;
  return MHIP_OK;
}
extern "C" int mhip_profile_read(mhip_ctx* ctx, int kid, double* total_ms, int64_t* launches) {
  if (!ctx || kid < 0 || kid >= MHIP_K_COUNT) return MHIP_EINVAL;
  prof_drain(ctx);
  if (total_ms) *total_ms = ctx->prof[kid].total_ms;
  if (launches) *launches = ctx->prof[kid].launches;
  return MHIP_OK;
}
