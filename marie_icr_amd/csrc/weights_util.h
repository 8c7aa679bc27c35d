// weights_util.h — host-side weight staging shared by every model file (CRAFT, CRNN, ICR, ViT, DiT, TrOCR, overlay): a
// state_dict-like tensor store, an arena builder that lays named blocks out once (256-byte aligned) and fills them in the
// kernels' layouts, and the conv packers the conv models have in common.
#pragma once
#include <math.h>

#include <algorithm>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "common.h"

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  size_t numel() const { return data.size(); }
};

struct TensorStore {
  std::map<std::string, HostTensor> t;
  int set(mhip_ctx* ctx, const std::string& key, const float* data, const int64_t* shape, int ndim) {
    if (!data || ndim < 0 || ndim > 5 || (ndim > 0 && !shape)) return mhip_fail(ctx, MHIP_EINVAL, "bad tensor %s", key.c_str());
    HostTensor h;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
      if (shape[i] <= 0) return mhip_fail(ctx, MHIP_EINVAL, "bad shape for %s", key.c_str());
      h.shape.push_back(shape[i]);
      n *= (size_t)shape[i];
    }
    h.data.assign(data, data + n);
    t[key] = std::move(h);
    return MHIP_OK;
  }
  const HostTensor* find(mhip_ctx* ctx, const std::string& k, const std::vector<int64_t>& shape) const {
    auto it = t.find(k);
    if (it == t.end()) {
      mhip_fail(ctx, MHIP_ESTATE, "missing tensor %s", k.c_str());
      return nullptr;
    }
    if (it->second.shape != shape) {
      mhip_fail(ctx, MHIP_EINVAL, "tensor %s has the wrong shape", k.c_str());
      return nullptr;
    }
    return &it->second;
  }
  bool has(const std::string& k) const { return t.count(k) != 0; }
};

// set_tensor of the conv models (CRAFT, CRNN, ICR): a DataParallel `module.` prefix is stripped, BatchNorm's
// num_batches_tracked is dropped, a key under none of `prefixes` is refused, and tensors are at most 4-d
inline int set_conv_model_tensor(mhip_ctx* ctx, TensorStore& st, bool& ready, const char* key,
                                 std::initializer_list<const char*> prefixes, const float* data, const int64_t* shape,
                                 int ndim) {
  std::string k(key);
  if (k.rfind("module.", 0) == 0) k = k.substr(7);
  if (k.size() > 19 && k.compare(k.size() - 19, 19, "num_batches_tracked") == 0) return MHIP_OK;
  if (std::none_of(prefixes.begin(), prefixes.end(), [&](const char* p) { return k.rfind(p, 0) == 0; }))
    return mhip_fail(ctx, MHIP_EINVAL, "unknown state_dict key %s", key);
  if (ndim > 4) return mhip_fail(ctx, MHIP_EINVAL, "bad tensor %s", key);
  int rc = st.set(ctx, k, data, shape, ndim);
  if (!rc) ready = false;
  return rc;
}

struct Arena {
  std::map<std::string, size_t> off;
  size_t bytes = 0;
  char* dev = nullptr;
  std::vector<char> host;
  size_t take(const std::string& name, size_t n) {
    size_t at = bytes;
    off[name] = at;
    bytes = (bytes + n + 255) / 256 * 256;
    return at;
  }
  bool known(const std::string& name) const { return off.count(name) != 0; }
  char* h(const std::string& name) { return host.data() + off.at(name); }
  template <typename P = char>
  P* d(const std::string& name) const { return (P*)(dev + off.at(name)); }
  void begin_fill() { host.assign(bytes, 0); }
  // fp32 source -> element type of `precision`
  static void put(int precision, char* dst, const float* src, size_t n) {
    if (precision == MHIP_PREC_F16) {
      _Float16* o = (_Float16*)dst;
      for (size_t i = 0; i < n; ++i) o[i] = (_Float16)src[i];
    } else {
      memcpy(dst, src, n * 4);
    }
  }
  int alloc(mhip_ctx* ctx) {
    if (!dev && hipMalloc((void**)&dev, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return mhip_fail(ctx, MHIP_ENOMEM, "arena allocation of %zu bytes failed", bytes);
    }
    return MHIP_OK;
  }
  int upload(mhip_ctx* ctx) {
    int rc = alloc(ctx);
    if (rc) return rc;
    MHIP_HIP(ctx, hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice));
    host.clear();
    host.shrink_to_fit();
    return MHIP_OK;
  }
  void release() {
    if (dev) (void)hipFree(dev);
    dev = nullptr;
  }
};

// conv weight [Co][Ci][k][k] -> [Cop][taps][Cip] at `precision`, zero padded to the channel counts the kernels see
inline void pack_conv_weight(int precision, char* dst, const HostTensor& w, int co, int ci, int taps, int cop, int cip) {
  std::vector<float> tmp((size_t)cop * taps * cip, 0.f);
  for (int o = 0; o < co; ++o)
    for (int c = 0; c < ci; ++c)
      for (int t = 0; t < taps; ++t) tmp[((size_t)o * taps + t) * cip + c] = w.data[((size_t)o * ci + c) * taps + t];
  Arena::put(precision, dst, tmp.data(), tmp.size());
}

// first-layer conv weight [Co][Cin][k][k] -> [tap*Cin + c][Co] fp32 for the VALU first-layer kernels
inline void pack_first_conv_weight(float* dst, const HostTensor& w, int co, int cin, int taps) {
  for (int o = 0; o < co; ++o)
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < taps; ++t) dst[(t * cin + c) * co + o] = w.data[((size_t)o * cin + c) * taps + t];
}

// fp32 per-channel epilogue of a conv: the conv's bias (none: 0) with an eval-mode BatchNorm (`bn` prefix, or nullptr)
// folded in, scale = gamma / sqrt(var + 1e-5), shift = beta + (bias - mean) * scale.  Both arrays hold max(cop, 64)
// channels; padded output channels get 1 / 0 (0 * x + 0 -> ReLU -> 0).
inline int fold_conv_bn(mhip_ctx* ctx, const TensorStore& st, const std::string& conv, bool has_bias, const char* bn,
                        int co, int cop, float* scale, float* shift) {
  const int np = std::max(cop, 64);
  std::fill(scale, scale + np, 1.f);
  std::fill(shift, shift + np, 0.f);
  if (has_bias) {
    const HostTensor* b = st.find(ctx, conv + ".bias", {co});
    if (!b) return MHIP_ESTATE;
    std::copy(b->data.begin(), b->data.end(), shift);
  }
  if (!bn) return MHIP_OK;
  const std::string p(bn);
  const HostTensor* g = st.find(ctx, p + ".weight", {co});
  const HostTensor* be = st.find(ctx, p + ".bias", {co});
  const HostTensor* mu = st.find(ctx, p + ".running_mean", {co});
  const HostTensor* va = st.find(ctx, p + ".running_var", {co});
  if (!g || !be || !mu || !va) return MHIP_ESTATE;
  for (int o = 0; o < co; ++o) {
    const float s = g->data[o] / sqrtf(va->data[o] + 1e-5f);   // nn.BatchNorm2d eps
    scale[o] = s;
    shift[o] = be->data[o] + (shift[o] - mu->data[o]) * s;
  }
  return MHIP_OK;
}
