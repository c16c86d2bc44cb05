// relp_trial.hpp -- the host side of the trial scope (relp_trial_begin / relp_trial_end) that needs no device (plain C++17, no
// HIP): the segment table one launch of k_tab_trial_copy takes, and the planner that lays the saved arrays out in the snapshot
// buffer.  Engine::trial_begin plans once, copies live -> snapshot; Engine::trial_end(0) copies the same table the other way.
#pragma once
#include <cstdint>

namespace relp {

static constexpr int32_t kTrialMaxSegments = 32;
static constexpr int64_t kTrialUnit = 16;              // bytes per load / store of the copy, and the alignment of every segment

// One copy of `bytes` bytes, src -> dst; both 16-byte aligned (the planner's offsets are, device allocations are).
struct TrialSegment { const void* src; void* dst; int64_t bytes; };
// What k_tab_trial_copy takes by value: the segments and, per segment, the number of whole 16-byte units of all segments up to and
// including it (the grid strides over [0, unit_end[count - 1]); segment s owns [unit_end[s - 1], unit_end[s])).  The
// bytes % 16 bytes behind a segment's last unit are its tail.
struct TrialTable {
    int32_t count = 0, pad_ = 0;
    TrialSegment seg[kTrialMaxSegments];
    int64_t unit_end[kTrialMaxSegments];
};

// The layout of a snapshot: every array a trial can change, in the order it was named, at 16-byte-aligned offsets of one buffer.
class TrialPlan {
  public:
    // Names `bytes` bytes at `live` (16-byte aligned; bytes == 0 is a segment that copies nothing).  false: a 33rd segment, a
    // negative length or a misaligned address -- nothing is added.
    bool add(void* live, int64_t bytes) {
        if (count_ >= kTrialMaxSegments || bytes < 0 || (reinterpret_cast<uintptr_t>(live) & (kTrialUnit - 1)) != 0) return false;
        live_[count_] = live; bytes_[count_] = bytes; offset_[count_] = total_;
        total_ += (bytes + kTrialUnit - 1) / kTrialUnit * kTrialUnit;
        ++count_;
        return true;
    }
    int32_t count() const { return count_; }
    int64_t offset(int32_t s) const { return offset_[s]; }
    int64_t bytes(int32_t s) const { return bytes_[s]; }
    void* live(int32_t s) const { return live_[s]; }
    int64_t payload_bytes() const { int64_t sum = 0; for (int32_t s = 0; s < count_; ++s) sum += bytes_[s]; return sum; }
    int64_t buffer_bytes() const { return total_; }    // what the snapshot buffer must hold (a multiple of 16)
    // The table of one direction over the snapshot buffer at `buffer` (16-byte aligned): save = live -> buffer, else buffer -> live.
    TrialTable table(void* buffer, bool save) const {
        TrialTable t;
        t.count = count_;
        int64_t units = 0;
        for (int32_t s = 0; s < kTrialMaxSegments; ++s) {
            if (s < count_) {
                char* snap = static_cast<char*>(buffer) + offset_[s];
                t.seg[s] = save ? TrialSegment{live_[s], snap, bytes_[s]} : TrialSegment{snap, live_[s], bytes_[s]};
                units += bytes_[s] / kTrialUnit;
            } else {
                t.seg[s] = TrialSegment{nullptr, nullptr, 0};
            }
            t.unit_end[s] = units;
        }
        return t;
    }

  private:
    int32_t count_ = 0;
    int64_t total_ = 0;
    void* live_[kTrialMaxSegments] = {};
    int64_t bytes_[kTrialMaxSegments] = {}, offset_[kTrialMaxSegments] = {};
};

}  // namespace relp
