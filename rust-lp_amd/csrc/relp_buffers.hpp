// relp_buffers.hpp -- the two owners of the host driver's memory, DeviceBuf<T> (device) and PinnedBuf<T> (pinned host), and every
// copy and fill the driver makes.  Move-only; both convert to T* so that launches and pointer arithmetic read as they
// do with a raw pointer.  Host files only.
// A copy or fill is enqueued on the stream the caller passes and has completed when the call returns: the host buffer may die, the
// data is there to read.  DeviceBuf's members refuse a range that does not fit the buffer (hipErrorInvalidValue, no HIP call); the
// free functions serve pointers carved out of a larger buffer and check nothing.  n = 0 is no HIP call.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace relp {

inline hipError_t first_error(hipError_t a, hipError_t b) { return a != hipSuccess ? a : b; }

// Where a copy runs: a plain hipStream_t means enqueue and wait.  enqueue_only(stream) is the exception, ENQUEUE ONLY: the host
// side is neither filled nor free to die until a waiting copy on the same stream has returned.  That copy follows in the same
// function with no `return` (so no HIP_TRY) in between; the results are collected with first_error.
struct On {
    hipStream_t s; bool wait;
    On(hipStream_t stream, bool wait_for_it = true) : s(stream), wait(wait_for_it) {}
    // (the wait is made even when the enqueue was refused: it is what ends a pair begun with enqueue_only)
    hipError_t done(hipError_t enqueued) const { return wait ? first_error(enqueued, hipStreamSynchronize(s)) : enqueued; }
};
inline On enqueue_only(hipStream_t s) { return On(s, false); }
enum Dir2d { kFromHost = hipMemcpyHostToDevice, kToHost = hipMemcpyDeviceToHost, kFromDevice = hipMemcpyDeviceToDevice };      // copy_2d

// ---- pieces carved out of a buffer: n elements of T between host memory and a device address, unchecked ----
template <class T> hipError_t upload_to(void* dev, const T* src, size_t n, On on) {
    return n ? on.done(hipMemcpyAsync(dev, src, n * sizeof(T), hipMemcpyHostToDevice, on.s)) : hipSuccess;
}
template <class T> hipError_t download_from(T* dst, const void* dev, size_t n, On on) {
    return n ? on.done(hipMemcpyAsync(dst, dev, n * sizeof(T), hipMemcpyDeviceToHost, on.s)) : hipSuccess;
}
template <class T> hipError_t download_from(std::vector<T>& dst, const void* dev, On on) { return download_from(dst.data(), dev, dst.size(), on); }
inline hipError_t fill_bytes_at(void* dev, int value, size_t bytes, On on) {
    return bytes ? on.done(hipMemsetAsync(dev, value, bytes, on.s)) : hipSuccess;
}

template <class T>
class DeviceBuf {
  public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept { swap(o); }
    DeviceBuf& operator=(DeviceBuf&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~DeviceBuf() { reset(); }
    operator T*() const { return p_; }
    bool owned() const { return owned_; }
    int64_t count() const { return count_; }               // elements; 0 when empty
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
        count_ = owned_ ? (int64_t)(bytes / sizeof(T)) : 0;
        return e;
    }
    // At least `count` elements (`bytes` bytes): nothing when the buffer is that large, else the old one is freed and max(count,
    // grown) are allocated as by alloc (alloc_raw); the contents are not kept.  A refused allocation leaves the buffer empty.
    hipError_t ensure(int64_t count, int64_t grown = 0) { return count <= count_ ? hipSuccess : alloc(std::max(count, grown)); }
    hipError_t ensure_raw(size_t bytes, size_t grown = 0) { return bytes <= (size_t)count_ * sizeof(T) ? hipSuccess : alloc_raw(std::max(bytes, grown)); }
    void adopt(T* p, int64_t count) { reset(); p_ = p; count_ = count; }      // a view of memory someone else frees
    void reset() { if (owned_) (void)hipFree(p_); p_ = nullptr; owned_ = false; count_ = 0; }
    void swap(DeviceBuf& o) noexcept { std::swap(p_, o.p_); std::swap(owned_, o.owned_); std::swap(count_, o.count_); }   // no HIP call

    // n elements from element `at` on
    hipError_t upload(const T* src, int64_t n, On on, int64_t at = 0) { return fits(at, n) ? upload_to(p_ + at, src, (size_t)n, on) : hipErrorInvalidValue; }
    hipError_t upload(const std::vector<T>& src, On on, int64_t at = 0) { return upload(src.data(), (int64_t)src.size(), on, at); }
    hipError_t download(T* dst, int64_t n, On on, int64_t at = 0) const { return fits(at, n) ? download_from(dst, p_ + at, (size_t)n, on) : hipErrorInvalidValue; }
    hipError_t download(std::vector<T>& dst, On on, int64_t at = 0) const { return download(dst.data(), (int64_t)dst.size(), on, at); }
    hipError_t zero(int64_t n, On on) { return fill_bytes(0, n, on); }
    hipError_t fill_bytes(int value, int64_t n, On on) {                      // every byte of the first n elements
        return fits(0, n) ? fill_bytes_at(p_, value, (size_t)n * sizeof(T), on) : hipErrorInvalidValue;
    }
    // 2-D: `columns` runs of `width` elements, `ld` apart here and `other_ld` apart at `other`: read into host memory there
    // (kToHost), or written from host (kFromHost) or device memory (kFromDevice) there; the first run starts at element `at` here
    hipError_t copy_2d(Dir2d dir, const T* other, int64_t other_ld, int64_t width, int64_t columns, int64_t ld, On on, int64_t at = 0) const {
        if (width < 0 || columns < 0 || at < 0 || width > ld || (width && columns && !fits(at + (columns - 1) * ld, width))) return hipErrorInvalidValue;
        if (!width || !columns) return hipSuccess;
        const size_t here = ld * sizeof(T), there = other_ld * sizeof(T), w = width * sizeof(T);
        return on.done(dir == kToHost ? hipMemcpy2DAsync(const_cast<T*>(other), there, p_ + at, here, w, columns, (hipMemcpyKind)dir, on.s)
                                      : hipMemcpy2DAsync(p_ + at, here, other, there, w, columns, (hipMemcpyKind)dir, on.s));
    }

  private:
    bool fits(int64_t at, int64_t n) const { return at >= 0 && n >= 0 && at <= count_ && n <= count_ - at; }
    T* p_ = nullptr;
    bool owned_ = false;
    int64_t count_ = 0;
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
    size_t bytes() const { return bytes_; }                // 0 when empty
    hipError_t alloc(size_t bytes, bool mapped = false) {  // not cleared
        reset();
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        bytes_ = bytes;
        if (mapped && (e = hipHostGetDevicePointer(reinterpret_cast<void**>(&dev_), p_, 0)) != hipSuccess) reset();
        return e;
    }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; dev_ = nullptr; bytes_ = 0; }
    void swap(PinnedBuf& o) noexcept { std::swap(p_, o.p_); std::swap(dev_, o.dev_); std::swap(bytes_, o.bytes_); }

  private:
    T* p_ = nullptr;
    T* dev_ = nullptr;
    size_t bytes_ = 0;
};

}  // namespace relp
