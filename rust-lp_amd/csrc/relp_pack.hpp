// relp_pack.hpp -- how the host driver cuts one buffer into 16-byte aligned pieces: Carver lays the pieces out (the buffer is
// allocated once its size is known), Packer fills a host copy of them on the way.  A piece is named once, where it is taken:
// take(&pointer, bytes) remembers where the piece's address goes, bind(base) writes every remembered pointer.  Host files only.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "relp_buffers.hpp"

namespace relp {

constexpr int64_t pack_up16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

class Carver {
  public:
    explicit Carver(int64_t min_piece = 0) : min_(min_piece) {}      // every piece takes at least min_piece bytes (rounded up to 16)
    int64_t take(int64_t bytes) { const int64_t at = size_; size_ += pack_up16(std::max(bytes, min_)); return at; }
    // the piece's address goes to *dst at bind(); wanted = false: the room is taken all the same, *dst becomes null
    template <class T> int64_t take(T** dst, int64_t bytes, bool wanted = true) {
        const int64_t at = take(bytes);
        point(dst, wanted ? at : -1);
        return at;
    }
    template <class T> void point(T** dst, int64_t at) { fix_.push_back(Fix{dst, at}); }      // at < 0: null
    // a piece some layouts do not have: no room and a null pointer without it
    template <class T> int64_t take_if(bool have, T** dst, int64_t bytes) { return take(dst, have ? bytes : 0, have); }
    int64_t size() const { return size_; }
    void bind(char* base) const {
        for (const Fix& f : fix_) {
            char* const p = f.at < 0 ? nullptr : base + f.at;
            std::memcpy(f.dst, &p, sizeof p);                // (*dst is a T* or a const T*: same representation)
        }
    }

  private:
    struct Fix { void* dst; int64_t at; };
    int64_t min_, size_ = 0;
    std::vector<Fix> fix_;
};

// Where a Packer keeps the host copy.  ensure(used, need): the buffer with room for `need` bytes and its first `used` bytes
// kept, or null.
struct VectorStore {
    std::vector<char> v;
    char* ensure(size_t, size_t need) { if (need > v.size()) v.resize(need); return v.data(); }
};
// pinned memory that outlives the Packer (the copy to the device is one DMA, not a staged one); grows to twice what is
// asked for, at least 1 MiB
struct PinnedStore {
    PinnedBuf<char>& buf;
    char* ensure(size_t used, size_t need) {
        if (need > buf.bytes()) {
            PinnedBuf<char> grown;
            if (grown.alloc(std::max<size_t>(need * 2, size_t(1) << 20)) != hipSuccess) return nullptr;
            if (used) std::memcpy(grown, buf, used);
            buf = std::move(grown);
        }
        return buf;
    }
};

template <class Store>
class Packer : public Carver {
  public:
    explicit Packer(Store store, int64_t min_piece = 0) : Carver(min_piece), store_(std::move(store)) {}
    // room for a piece the caller writes itself (every byte of it, padding included); null once the store has failed.  The
    // pointer holds until the next piece is taken.
    char* reserve(int64_t bytes, int64_t* at) {
        const size_t used = (size_t)size();
        *at = take(bytes);
        char* const base = failed_ ? nullptr : store_.ensure(used, (size_t)size());
        if (!base) { failed_ = true; return nullptr; }
        return base + *at;
    }
    // a copy of src, its padding zeroed
    int64_t put(const void* src, size_t bytes) {
        int64_t at = 0;
        if (char* const p = reserve((int64_t)bytes, &at)) {
            if (bytes) std::memcpy(p, src, bytes);
            std::memset(p + bytes, 0, (size_t)(size() - at) - bytes);
        }
        return at;
    }
    template <class V> int64_t put(const V& v) { return put(v.data(), sizeof(*v.data()) * v.size()); }
    template <class T, class V> int64_t put(T** dst, const V& v, bool wanted = true) {
        const int64_t at = put(v);
        point(dst, wanted ? at : -1);
        return at;
    }
    bool failed() const { return failed_; }
    const char* data() { return store_.ensure((size_t)size(), (size_t)size()); }

  private:
    Store store_;
    bool failed_ = false;
};

}  // namespace relp
