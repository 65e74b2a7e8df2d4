// What the handles of the C ABI hold on a device, as move-only owners, and the small helpers capi.hip and capi_sharded.hip
// share.  Host code only: no device translation unit includes this file (asset_asrl_amd/build.py lists it for those two).
// Nothing is freed anywhere else: a failing path returns, and whatever it had built so far goes with its locals.
// The device a resource lives on must be current when its owner lets go of it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>

#include "../../../include/asset_hip.h"

extern "C" __attribute__((visibility("hidden"))) void asset_hip_set_last_error(const char* msg);   // capi.hip

namespace asset_hip {

// a stream or an event of the HIP runtime
template <class H, hipError_t (*Destroy)(H)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) release(), h_ = std::exchange(o.h_, nullptr);
    return *this;
  }
  ~Owned() { release(); }
  void release() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }
  H get() const { return h_; }

 protected:
  H h_ = nullptr;
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
  hipError_t create() { return release(), hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
  hipError_t create() { return release(), hipEventCreate(&h_); }
};

// n elements of T in device memory (DeviceBuffer) or in page-locked host memory (PinnedBuffer); empty converts to false
inline hipError_t pinned_malloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
template <class T, hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
class Buffer {
 public:
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) release(), p_ = std::exchange(o.p_, nullptr), n_ = std::exchange(o.n_, 0);
    return *this;
  }
  ~Buffer() { release(); }
  hipError_t allocate(size_t n) {
    release();
    const hipError_t e = Alloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
    if (e == hipSuccess) n_ = n;
    else p_ = nullptr;
    return e;
  }
  void release() {
    if (p_) (void)Free(p_);
    p_ = nullptr, n_ = 0;
  }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};
template <class T> using DeviceBuffer = Buffer<T, hipMalloc, hipFree>;
template <class T> using PinnedBuffer = Buffer<T, pinned_malloc, hipHostFree>;

// The entry points of capi_sharded.hip walk the shards' devices (hipSetDevice is per thread): the calling thread's current device is
// put back on every exit path, so that a caller who also uses torch or another HIP client on this thread does not find its later
// allocations and launches on the last shard's GPU.
struct DeviceGuard {
  int dev = -1;
  DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) { dev = -1; (void)hipGetLastError(); } }
  ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Makes device `ordinal` current; 0, or the error code with the error text set.  no_fallback: "the evaluator has no CPU fallback".
inline int use_device(int ordinal, const char* no_fallback) {
  auto fail = [](int code, const char* msg) { asset_hip_set_last_error(msg); return code; };
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(ASSET_HIP_ENODEV, no_fallback);
  }
  if (ordinal < 0 || ordinal >= ndev) return fail(ASSET_HIP_EINVAL, "device ordinal out of range");
  const hipError_t e = hipSetDevice(ordinal);
  if (e != hipSuccess) return fail(int(e), (std::string("hipSetDevice: ") + hipGetErrorString(e)).c_str());
  return 0;
}

// does the evaluation kind contract with multipliers (adjoint gradient) / write KKT entries
inline bool wants_multipliers(int what) {
  what &= 0xff;
  return what == ASSET_HIP_CON_ADJGRAD || what == ASSET_HIP_JAC_ADJGRAD || what == ASSET_HIP_JAC_ADJGRAD_HESS;
}
inline bool wants_kkt(int what) { return (what & 0xff) >= ASSET_HIP_JAC; }

// the `stream` argument of a *_device entry point: NULL names the handle's own stream
template <class Handle>
hipStream_t stream_or(const Handle* h, void* stream) {
  return stream ? static_cast<hipStream_t>(stream) : h->stream.get();
}

}  // namespace asset_hip
