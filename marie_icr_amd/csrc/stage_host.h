// stage_host.h — the plumbing of the per-kernel stage entries (mhip_*_host in icr_ops.hip and image_ops.hip): host buffers
// up, one launcher call, guarded outputs back.  Test surface only; the models never come through here.
//
//   act   an activation: fp32 on the host, the mode's element type on the device (narrowed on the way in, widened on the way
//         out; the kernel-level tests hand over f16-representable values, so the narrowing is exact)
//   raw   bytes as they are (u8 images, int32 indices, fp32 weights / scores)
// Every output is carved with MHIP_STAGE_GUARD elements behind it, filled with 0xff bytes before the launch and read back
// whole: a cell never written, or a write past the end, reaches the caller (f16 0xffff widens to the fp32 NaN 0xffffe000).
#pragma once
#include <functional>

#include "common.h"

struct StageIO {
  struct Slot {
    const void* src;   // host source (inputs, in/out), or nullptr
    void* dst;         // host destination of n + MHIP_STAGE_GUARD elements (outputs, in/out), or nullptr
    size_t n, es;      // elements the launch owns, host element size
    bool act;
    char* dev = nullptr;
    std::vector<char> tmp;
  };
  mhip_ctx* ctx;
  int precision;
  std::vector<Slot> slots;

  StageIO(mhip_ctx* c, int prec) : ctx(c), precision(prec) { slots.reserve(16); }
  size_t dev_es(const Slot& s) const { return s.act ? (precision == MHIP_PREC_F16 ? 2 : 4) : s.es; }
  size_t dev_el(const Slot& s) const { return s.n + (s.dst ? MHIP_STAGE_GUARD : 0); }

  int add(const void* src, void* dst, size_t n, size_t es, bool act) {
    slots.push_back(Slot{src, dst, n, es, act});
    return (int)slots.size() - 1;
  }
  int in_act(const float* h, size_t n) { return add(h, nullptr, n, 4, true); }
  int in_raw(const void* h, size_t n, size_t es) { return add(h, nullptr, n, es, false); }
  int out_act(float* h, size_t n) { return add(nullptr, h, n, 4, true); }
  int out_raw(void* h, size_t n, size_t es) { return add(nullptr, h, n, es, false); }
  int inout_raw(void* h, size_t n, size_t es) { return add(h, h, n, es, false); }
  template <typename P = void>
  P* dev(int i) const { return (P*)slots[i].dev; }

  // carve, upload, fill the outputs, launch(), read back after a synchronise
  int run(const std::function<int()>& launch) {
    MHIP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = mhip_carve_workspace(ctx, [&](Carver& ws) {
      for (Slot& s : slots) s.dev = ws.take(dev_el(s) * dev_es(s));
    });
    if (rc) return rc;
    for (Slot& s : slots) {
      const size_t es = dev_es(s);
      if (s.dst) MHIP_HIP(ctx, hipMemsetAsync(s.dev, 0xff, dev_el(s) * es, ctx->stream));
      if (!s.src || !s.n) continue;
      const void* from = s.src;
      if (s.act && es == 2) {
        s.tmp.resize(s.n * 2);
        for (size_t i = 0; i < s.n; ++i) ((_Float16*)s.tmp.data())[i] = (_Float16)((const float*)s.src)[i];
        from = s.tmp.data();
      }
      MHIP_HIP(ctx, hipMemcpyAsync(s.dev, from, s.n * es, hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = launch())) {
      (void)hipStreamSynchronize(ctx->stream);      // the uploads still read this call's host memory
      return rc;
    }
    for (Slot& s : slots) {
      if (!s.dst) continue;
      const size_t es = dev_es(s), bytes = dev_el(s) * es;
      void* to = s.dst;
      if (s.act && es == 2) {
        s.tmp.resize(bytes);
        to = s.tmp.data();
      }
      MHIP_HIP(ctx, hipMemcpyAsync(to, s.dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    MHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (Slot& s : slots)
      if (s.dst && s.act && dev_es(s) == 2)
        for (size_t i = 0; i < dev_el(s); ++i) ((float*)s.dst)[i] = (float)((const _Float16*)s.tmp.data())[i];
    return MHIP_OK;
  }
};

inline int mhip_stage_precision(mhip_ctx* ctx, int precision) {
  if (precision != MHIP_PREC_F16 && precision != MHIP_PREC_F32) return mhip_fail(ctx, MHIP_EINVAL, "unknown precision %d", precision);
  return MHIP_OK;
}
