// relp_buffers.hpp -- the two owners of the host driver's memory: DeviceBuf<T> (device) and PinnedBuf<T> (pinned host).
// Move-only; both convert to T* so that launches and pointer arithmetic read as they do with a raw pointer.  Host files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>

namespace relp {

template <class T>
class DeviceBuf {
  public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept { swap(o); }
    DeviceBuf& operator=(DeviceBuf&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~DeviceBuf() { reset(); }
    operator T*() const { return p_; }
    bool owned() const { return owned_; }
    // Zero-initialised.  hipMemset runs on the null stream, which does not order with the engine's non-blocking stream: the
    // device is synchronised before the buffer is handed out, so a kernel enqueued right afterwards cannot be overtaken by it.
    hipError_t alloc(int64_t count) {
        if (count < 1) count = 1;
        hipError_t e = alloc_raw((size_t)count * sizeof(T));
        if (e == hipSuccess) e = hipMemset(p_, 0, (size_t)count * sizeof(T));
        return e == hipSuccess ? hipDeviceSynchronize() : e;
    }
    hipError_t alloc_raw(size_t bytes) {                   // hipMalloc alone: neither filled nor synchronised
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), bytes);
        owned_ = e == hipSuccess;
        if (!owned_) p_ = nullptr;
        return e;
    }
    void adopt(T* p) { reset(); p_ = p; }                  // a view of memory someone else frees
    void reset() { if (owned_) (void)hipFree(p_); p_ = nullptr; owned_ = false; }
    void swap(DeviceBuf& o) noexcept { std::swap(p_, o.p_); std::swap(owned_, o.owned_); }      // two words, no HIP call

  private:
    T* p_ = nullptr;
    bool owned_ = false;
};

template <class T>
class PinnedBuf {
  public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept { swap(o); }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~PinnedBuf() { reset(); }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    T* device() const { return dev_; }                     // the device's address of a mapped buffer (else null)
    hipError_t alloc(size_t bytes, bool mapped = false) {  // not cleared
        reset();
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        if (mapped && (e = hipHostGetDevicePointer(reinterpret_cast<void**>(&dev_), p_, 0)) != hipSuccess) reset();
        return e;
    }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; dev_ = nullptr; }
    void swap(PinnedBuf& o) noexcept { std::swap(p_, o.p_); std::swap(dev_, o.dev_); }

  private:
    T* p_ = nullptr;
    T* dev_ = nullptr;
};

}  // namespace relp
