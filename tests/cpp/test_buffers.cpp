// test_buffers.cpp (no GPU, no library): rust-lp_amd/csrc/relp_buffers.hpp against stubs of the HIP entry points it calls.
// The stubs keep "device" memory on the heap, move the bytes at once and record every call, so the tests can say which calls
// a buffer operation made, on which stream and in which order -- and a sanitizer build sees every byte that moves.
#include "relp_buffers.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "check.hpp"

namespace {
struct Call { std::string name; hipStream_t stream; size_t bytes; };
std::vector<Call> calls;
std::map<void*, bool> device_live, pinned_live;         // allocation -> not freed yet (freeing anything else is an error)
int allocations = 0, frees = 0;
int refuse_malloc = 0;                                  // the next hipMalloc calls fail

hipStream_t const S1 = reinterpret_cast<hipStream_t>(0x1000), S2 = reinterpret_cast<hipStream_t>(0x2000);

bool made(size_t from, std::initializer_list<const char*> names, hipStream_t stream) {      // the calls since `from`, all on `stream`
    if (calls.size() - from != names.size()) return false;
    size_t k = from;
    for (const char* n : names) {
        if (calls[k].name != n) return false;
        if (calls[k].stream != stream && calls[k].name != "hipMalloc" && calls[k].name != "hipFree") return false;
        ++k;
    }
    return true;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    calls.push_back({"hipMalloc", nullptr, bytes});
    if (refuse_malloc > 0) { --refuse_malloc; *p = reinterpret_cast<void*>(0xBAD); return hipErrorOutOfMemory; }
    *p = std::malloc(bytes ? bytes : 1);
    device_live[*p] = true;
    ++allocations;
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    calls.push_back({"hipFree", nullptr, 0});
    if (!device_live.count(p) || !device_live[p]) { ++g_failed; std::printf("hipFree of memory that is not allocated\n"); return hipErrorInvalidValue; }
    device_live[p] = false; ++frees;
    std::free(p);
    return hipSuccess;
}
hipError_t hipMemset(void* p, int v, size_t bytes) { calls.push_back({"hipMemset", nullptr, bytes}); std::memset(p, v, bytes); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { calls.push_back({"hipDeviceSynchronize", nullptr, 0}); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { calls.push_back({"hipStreamSynchronize", s, 0}); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t s) {
    calls.push_back({"hipMemcpyAsync", s, bytes});
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t s) { calls.push_back({"hipMemsetAsync", s, bytes}); std::memset(p, v, bytes); return hipSuccess; }
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t s) {
    calls.push_back({"hipMemcpy2DAsync", s, width * height});
    for (size_t r = 0; r < height; ++r) std::memcpy(static_cast<char*>(dst) + r * dpitch, static_cast<const char*>(src) + r * spitch, width);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) {
    calls.push_back({"hipHostMalloc", nullptr, bytes});
    *p = std::malloc(bytes ? bytes : 1);
    pinned_live[*p] = true;
    ++allocations;
    return hipSuccess;
}
hipError_t hipHostFree(void* p) {
    calls.push_back({"hipHostFree", nullptr, 0});
    if (!pinned_live.count(p) || !pinned_live[p]) { ++g_failed; std::printf("hipHostFree of memory that is not allocated\n"); return hipErrorInvalidValue; }
    pinned_live[p] = false; ++frees;
    std::free(p);
    return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned int) { calls.push_back({"hipHostGetDevicePointer", nullptr, 0}); *d = h; return hipSuccess; }
}

using relp::DeviceBuf;
using relp::PinnedBuf;
using relp::enqueue_only;

static void test_alloc_and_ensure() {
    DeviceBuf<double> b;
    CHECK(b.count() == 0 && !b.owned() && static_cast<double*>(b) == nullptr);
    size_t at = calls.size();
    CHECK(b.alloc(0) == hipSuccess);                       // count 0 -> 1
    CHECK(b.count() == 1 && b.owned());
    CHECK(made(at, {"hipMalloc", "hipMemset", "hipDeviceSynchronize"}, nullptr));
    CHECK(calls[at].bytes == sizeof(double) && calls[at + 1].bytes == sizeof(double));
    CHECK(b[0] == 0.0);
    at = calls.size();
    CHECK(b.alloc(5) == hipSuccess && b.count() == 5);
    CHECK(made(at, {"hipFree", "hipMalloc", "hipMemset", "hipDeviceSynchronize"}, nullptr));
    at = calls.size();
    CHECK(b.ensure(5) == hipSuccess && b.ensure(3, 100) == hipSuccess && b.ensure_raw(40) == hipSuccess && b.ensure(0) == hipSuccess);
    CHECK(calls.size() == at && b.count() == 5);           // large enough: no call
    CHECK(b.ensure(6, 9) == hipSuccess && b.count() == 9); // grows to the slack asked for, zero-filled like alloc
    CHECK(made(at, {"hipFree", "hipMalloc", "hipMemset", "hipDeviceSynchronize"}, nullptr) && calls[at + 1].bytes == 9 * sizeof(double));
    at = calls.size();
    CHECK(b.ensure(12) == hipSuccess && b.count() == 12);  // without slack: exact
    CHECK(calls[at + 1].bytes == 12 * sizeof(double));
    at = calls.size();
    CHECK(b.ensure_raw(100, 256) == hipSuccess && b.count() == 32);      // raw: hipMalloc alone
    CHECK(made(at, {"hipFree", "hipMalloc"}, nullptr) && calls[at + 1].bytes == 256);
    at = calls.size();
    CHECK(b.alloc_raw(20) == hipSuccess && b.count() == 2);              // whole elements only
    refuse_malloc = 1;
    CHECK(b.ensure(3) == hipErrorOutOfMemory);             // refused: empty, length 0, the old buffer freed once
    CHECK(b.count() == 0 && !b.owned() && static_cast<double*>(b) == nullptr);
    refuse_malloc = 1;
    CHECK(b.ensure_raw(8) == hipErrorOutOfMemory && b.count() == 0 && static_cast<double*>(b) == nullptr);
    at = calls.size();
    CHECK(b.upload(nullptr, 1, S1) == hipErrorInvalidValue && calls.size() == at);       // nothing fits an empty buffer
    CHECK(b.ensure(2) == hipSuccess && b.count() == 2);    // and it can be used again
}

static void test_swap_move_adopt() {
    DeviceBuf<int32_t> a, b;
    CHECK(a.alloc(4) == hipSuccess && b.alloc(7) == hipSuccess);
    int32_t* const pa = a; int32_t* const pb = b;
    size_t at = calls.size();
    a.swap(b);
    CHECK(a.count() == 7 && b.count() == 4 && static_cast<int32_t*>(a) == pb && static_cast<int32_t*>(b) == pa);
    DeviceBuf<int32_t> c(std::move(a));
    CHECK(c.count() == 7 && static_cast<int32_t*>(c) == pb && a.count() == 0 && static_cast<int32_t*>(a) == nullptr);
    DeviceBuf<int32_t> empty;
    b.swap(empty);                                         // swapping with an empty one: the length goes with the pointer
    CHECK(b.count() == 0 && !b.owned() && empty.count() == 4 && empty.owned());
    CHECK(calls.size() == at);                             // no HIP call so far
    b = std::move(empty);                                  // move assignment frees what the target held (nothing here)
    CHECK(b.count() == 4 && static_cast<int32_t*>(b) == pa && empty.count() == 0 && calls.size() == at);
    c = std::move(b);                                      // ... and here the 7 elements
    CHECK(made(at, {"hipFree"}, nullptr) && c.count() == 4 && b.count() == 0);

    int32_t theirs[6] = {1, 2, 3, 4, 5, 6};
    at = calls.size();
    {
        DeviceBuf<int32_t> view;
        view.adopt(theirs, 6);
        CHECK(view.count() == 6 && !view.owned() && static_cast<int32_t*>(view) == theirs);
        int32_t got[2] = {0, 0};
        CHECK(view.download(got, 2, S1, 4) == hipSuccess && got[0] == 5 && got[1] == 6);
        CHECK(view.download(got, 2, S1, 5) == hipErrorInvalidValue);
        view.reset();
        CHECK(view.count() == 0);
        view.adopt(theirs, 6);
        DeviceBuf<int32_t> owned;
        CHECK(owned.alloc(1) == hipSuccess);
        owned.adopt(theirs, 3);                            // adopting frees what was owned, never what is adopted
        CHECK(!owned.owned() && owned.count() == 3);
    }
    int freed = 0;
    for (size_t k = at; k < calls.size(); ++k) freed += calls[k].name == "hipFree";
    CHECK(freed == 1);                                     // the one buffer `owned` had allocated

    PinnedBuf<char> p, q;
    CHECK(p.bytes() == 0);
    CHECK(p.alloc(100) == hipSuccess && p.bytes() == 100 && p.device() == nullptr);
    CHECK(q.alloc(16, true) == hipSuccess && q.bytes() == 16 && q.device() == static_cast<char*>(q));
    char* const pp = p;
    at = calls.size();
    p.swap(q);
    CHECK(p.bytes() == 16 && q.bytes() == 100 && static_cast<char*>(q) == pp && calls.size() == at);
    PinnedBuf<char> r(std::move(q));
    CHECK(r.bytes() == 100 && q.bytes() == 0 && calls.size() == at);
    r.reset();
    CHECK(r.bytes() == 0 && static_cast<char*>(r) == nullptr && made(at, {"hipHostFree"}, nullptr));
}

static void test_copies() {
    DeviceBuf<double> b;
    CHECK(b.alloc(8) == hipSuccess);
    const std::vector<double> src = {1, 2, 3, 4, 5, 6, 7, 8};
    std::vector<double> dst(8, -1.0);
    // each copy: exactly one async call on the given stream, then one wait for that stream
    size_t at = calls.size();
    CHECK(b.upload(src.data(), 8, S1) == hipSuccess);
    CHECK(made(at, {"hipMemcpyAsync", "hipStreamSynchronize"}, S1) && calls[at].bytes == 64);
    at = calls.size();
    CHECK(b.upload(src, S2) == hipSuccess && made(at, {"hipMemcpyAsync", "hipStreamSynchronize"}, S2));
    at = calls.size();
    CHECK(b.download(dst.data(), 8, S2) == hipSuccess && made(at, {"hipMemcpyAsync", "hipStreamSynchronize"}, S2) && dst == src);
    std::vector<double> part(3, 0.0);
    at = calls.size();
    CHECK(b.download(part, S1, 5) == hipSuccess && made(at, {"hipMemcpyAsync", "hipStreamSynchronize"}, S1));
    CHECK(part[0] == 6 && part[2] == 8);
    at = calls.size();
    CHECK(b.upload(part.data(), 2, S1, 1) == hipSuccess && made(at, {"hipMemcpyAsync", "hipStreamSynchronize"}, S1) && b[1] == 6 && b[2] == 7 && b[3] == 4);
    at = calls.size();
    CHECK(b.fill_bytes(0xFF, 2, S1) == hipSuccess && made(at, {"hipMemsetAsync", "hipStreamSynchronize"}, S1) && calls[at].bytes == 16);
    at = calls.size();
    CHECK(b.zero(8, S2) == hipSuccess && made(at, {"hipMemsetAsync", "hipStreamSynchronize"}, S2) && b[0] == 0.0 && b[7] == 0.0);
    // the enqueue-only download waits for nothing
    CHECK(b.upload(src, S1) == hipSuccess);
    at = calls.size();
    CHECK(b.download(dst.data(), 4, enqueue_only(S1), 4) == hipSuccess && made(at, {"hipMemcpyAsync"}, S1) && dst[0] == 5);
    at = calls.size();
    CHECK(relp::download_from(dst.data(), static_cast<double*>(b), 2, enqueue_only(S2)) == hipSuccess && made(at, {"hipMemcpyAsync"}, S2));
    at = calls.size();
    CHECK(b.upload(src, enqueue_only(S1)) == hipSuccess && made(at, {"hipMemcpyAsync"}, S1) && b[7] == 8);
    at = calls.size();
    CHECK(b.upload(std::vector<double>(9, 0.0), enqueue_only(S1)) == hipErrorInvalidValue && calls.size() == at);
    CHECK(relp::fill_bytes_at(static_cast<double*>(b), 0, 8, enqueue_only(S2)) == hipSuccess && made(at, {"hipMemsetAsync"}, S2) && b[0] == 0.0);
    CHECK(b.upload(src, S1) == hipSuccess);
    // the edges of the range: n = 0 (no call), at + n == count() (accepted), one more (refused, no call)
    at = calls.size();
    CHECK(b.upload(src.data(), 0, S1) == hipSuccess && b.download(dst.data(), 0, S1, 8) == hipSuccess && b.zero(0, S1) == hipSuccess);
    CHECK(b.download(dst.data(), 0, enqueue_only(S1)) == hipSuccess && calls.size() == at);
    CHECK(b.upload(src.data(), 3, S1, 5) == hipSuccess && b.download(dst.data(), 1, S1, 7) == hipSuccess);
    CHECK(b.download(dst.data(), 8, enqueue_only(S1)) == hipSuccess && b.fill_bytes(1, 8, S1) == hipSuccess);
    at = calls.size();
    CHECK(b.upload(src.data(), 4, S1, 5) == hipErrorInvalidValue && b.upload(src.data(), 9, S1) == hipErrorInvalidValue);
    CHECK(b.download(dst.data(), 1, S1, 8) == hipErrorInvalidValue && b.download(dst.data(), 9, S1) == hipErrorInvalidValue);
    CHECK(b.download(dst.data(), 2, enqueue_only(S1), 7) == hipErrorInvalidValue && b.zero(9, S1) == hipErrorInvalidValue);
    CHECK(b.fill_bytes(0, 9, S1) == hipErrorInvalidValue && b.upload(src.data(), 1, S1, -1) == hipErrorInvalidValue);
    CHECK(b.upload(src.data(), -1, S1) == hipErrorInvalidValue && b.upload(src.data(), 1, S1, INT64_MAX) == hipErrorInvalidValue);
    CHECK(calls.size() == at);
    // the free functions over carved pieces: the same call shape, no check
    at = calls.size();
    CHECK(relp::upload_to(b + 2, src.data(), 2, S1) == hipSuccess && made(at, {"hipMemcpyAsync", "hipStreamSynchronize"}, S1) && b[2] == 1 && b[3] == 2);
    at = calls.size();
    CHECK(relp::download_from(part, b + 2, S2) == hipSuccess && made(at, {"hipMemcpyAsync", "hipStreamSynchronize"}, S2) && part[1] == 2);
    at = calls.size();
    CHECK(relp::fill_bytes_at(b + 6, 0, 16, S1) == hipSuccess && made(at, {"hipMemsetAsync", "hipStreamSynchronize"}, S1) && b[7] == 0.0);
    CHECK(relp::upload_to(b + 0, src.data(), 0, S1) == hipSuccess && relp::fill_bytes_at(b + 0, 0, 0, S1) == hipSuccess && calls.size() == at + 2);
}

static void test_2d() {
    DeviceBuf<double> b;                                   // 3 columns of 2, leading dimension 4, the last column cut short: 10 elements
    CHECK(b.alloc(10) == hipSuccess);
    const double src[9] = {1, 2, 0, 3, 4, 0, 5, 6, 0};     // leading dimension 3
    size_t at = calls.size();
    CHECK(b.copy_2d(relp::kFromHost, src, 3, 2, 3, 4, S1) == hipSuccess && made(at, {"hipMemcpy2DAsync", "hipStreamSynchronize"}, S1));
    CHECK(b[0] == 1 && b[1] == 2 && b[2] == 0 && b[4] == 3 && b[5] == 4 && b[8] == 5 && b[9] == 6);
    double out[6] = {0};
    at = calls.size();
    CHECK(b.copy_2d(relp::kToHost, out, 2, 2, 3, 4, S2) == hipSuccess && made(at, {"hipMemcpy2DAsync", "hipStreamSynchronize"}, S2));
    CHECK(out[0] == 1 && out[1] == 2 && out[2] == 3 && out[3] == 4 && out[4] == 5 && out[5] == 6);
    at = calls.size();
    CHECK(b.copy_2d(relp::kFromHost, src, 3, 2, 0, 4, S1) == hipSuccess && b.copy_2d(relp::kFromHost, src, 3, 0, 3, 4, S1) == hipSuccess && calls.size() == at);
    CHECK(b.copy_2d(relp::kFromHost, src, 3, 3, 3, 4, S1) == hipErrorInvalidValue);     // the last column ends at element 11
    CHECK(b.copy_2d(relp::kFromHost, src, 3, 2, 4, 4, S1) == hipErrorInvalidValue && b.copy_2d(relp::kToHost, out, 2, 2, 4, 4, S1) == hipErrorInvalidValue);
    CHECK(b.copy_2d(relp::kFromHost, src, 3, 5, 1, 4, S1) == hipErrorInvalidValue && calls.size() == at);       // wider than the leading dimension
}

int main() {
    test_alloc_and_ensure();
    test_swap_move_adopt();
    test_copies();
    test_2d();
    // every allocation freed exactly once
    for (const auto& a : device_live) CHECK(!a.second);
    for (const auto& a : pinned_live) CHECK(!a.second);
    CHECK(allocations > 10 && frees == allocations);
    return finish("test_buffers");
}
