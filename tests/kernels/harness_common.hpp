// What every source of the kernel harness shares (test infrastructure; harness*.cpp, linked into ONE librelp_kernel_harness.so):
// the refusal codes and macros, the sticky HIP error, the device copy of a host image and the shape check of a sliced-ELL pool.
//
// Rules of every entry: a refusal (negative code) comes before any HIP call and launches nothing; a HIP error is returned as
// kHipErrorBase + hipError_t and is sticky for the whole library: g_sticky is one object, every entry of every family returns
// it before it touches the GPU, so after the first HIP error nothing is launched any more in this process.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "relp_kernels.h"

constexpr int kRefusedShape = -1;    // a size out of range (m < 1, p > kmax, kmax > 128, a count beyond its cap, ...)
constexpr int kRefusedIndex = -2;    // a row or column index, an offset or a list entry out of range
constexpr int kRefusedBatch = -3;    // a batch tab_load_batch would remap
constexpr int kRefusedOverlap = -3;  // harness_trial.cpp: a destination that overlaps another segment
constexpr int kRefusedLength = -4;   // a wrong array length
constexpr int kRefusedSplits = -5;   // splits < 1 or beyond min(count, the launcher's maximum)
constexpr int kRefusedOrder = -6;    // a list that is not strictly ascending, a repeated basis entry, a direct term on a basic column
constexpr int kHipErrorBase = 1000;  // + hipError_t of the first failed HIP call (sticky)
constexpr int64_t kPoolCap = 1 << 22;   // items, rows and columns a pool entry takes at most

inline int g_sticky = 0;             // one for the library: rkh_sticky_error() reads it

#define REFUSE_IF(cond, code) do { if (cond) return (code); } while (0)
#define REFUSE_LEN(len, want) do { if ((int64_t)(len) != (int64_t)(want)) return kRefusedLength; } while (0)
#define HIP_OK(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { g_sticky = kHipErrorBase + (int)e_; return g_sticky; } } while (0)
#define TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// a device copy of a host image; freed on every way out
template <class T>
struct Image {
    T* d = nullptr; T* h; int64_t n;
    Image(T* host, int64_t len) : h(host), n(len) {}
    Image(const Image&) = delete;
    Image& operator=(const Image&) = delete;
    ~Image() { if (d) (void)hipFree(d); }
    hipError_t up() {
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), sizeof(T) * (size_t)(n > 0 ? n : 1));
        return (e != hipSuccess || n == 0) ? e : hipMemcpy(d, h, sizeof(T) * (size_t)n, hipMemcpyHostToDevice);
    }
    hipError_t back() { return n == 0 ? hipSuccess : hipMemcpy(h, d, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost); }
};

// The sliced-ELL shape of a pool of `count` items over [0, bound): slice_ptr ascends from 0 in multiples of 64 entries, idx and val
// are as long as it says, the scalars and the flags one per item, every index in [-1, bound).
inline int check_sliced_ell(int64_t count, int64_t bound, const int64_t* slice_ptr, int64_t slice_ptr_len, const int32_t* idx, int64_t idx_len,
                            int64_t val_len, int64_t scalar_len, int64_t active_len) {
    const int64_t slices = (count + relp::kPoolSlice - 1) / relp::kPoolSlice;
    REFUSE_IF(slice_ptr_len != slices + 1 || scalar_len != count || active_len != count, kRefusedLength);
    REFUSE_IF(slice_ptr[0] != 0, kRefusedIndex);
    for (int64_t s = 0; s < slices; ++s)
        REFUSE_IF(slice_ptr[s + 1] < slice_ptr[s] || (slice_ptr[s + 1] - slice_ptr[s]) % relp::kPoolSlice != 0, kRefusedIndex);
    REFUSE_IF(idx_len != slice_ptr[slices] || val_len != idx_len || idx_len > 16 * kPoolCap, kRefusedLength);
    for (int64_t x = 0; x < idx_len; ++x) REFUSE_IF(idx[x] < -1 || idx[x] >= bound, kRefusedIndex);
    return 0;
}
