// The kernel harness of the trial snapshot (test infrastructure): one extern "C" entry that runs relp::launch_tab_trial_copy of the
// shipped librelp_engine.so once on ONE device image a test constructs (tests/kernel_harness_trial.py) and hands the image back.
// `make -C tests/kernels`
//
// The caller owns the layout: the segments are (source offset, destination offset, bytes) inside the image, and whatever lies
// between them is the caller's canaries.  This file only checks that nothing the launch may touch lies outside the image, that
// every offset is 16-byte aligned and that no destination overlaps another segment's bytes -- a refused call (negative code)
// launches nothing --, uploads, launches, synchronises and downloads.  A HIP error is returned as 1000 + code and is sticky
// for the whole library (harness_common.hpp): nothing is launched any more in this process.
#include "harness_common.hpp"

using namespace relp;

namespace {

bool overlap(int64_t a, int64_t a_len, int64_t b, int64_t b_len) { return a_len > 0 && b_len > 0 && a < b + b_len && b < a + a_len; }

}  // namespace

extern "C" {

int rkt_max_segments() { return kTrialMaxSegments; }
int rkt_grid() { return kTabTrialGrid; }

// launch_tab_trial_copy on `count` segments of the image: bytes[s] bytes from img + src_off[s] to img + dst_off[s].
int rkt_trial_copy(uint8_t* img, int64_t img_len, int64_t count, const int64_t* src_off, const int64_t* dst_off, const int64_t* bytes) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(!img || img_len < 16 || img_len > (int64_t(1) << 28) || count < 1 || count > kTrialMaxSegments, kRefusedShape);
    REFUSE_IF(!src_off || !dst_off || !bytes, kRefusedShape);
    for (int64_t s = 0; s < count; ++s) {
        REFUSE_IF(bytes[s] < 0 || src_off[s] < 0 || dst_off[s] < 0 || src_off[s] % kTrialUnit || dst_off[s] % kTrialUnit, kRefusedIndex);
        REFUSE_IF(bytes[s] > img_len || src_off[s] > img_len - bytes[s] || dst_off[s] > img_len - bytes[s], kRefusedIndex);
        REFUSE_IF(overlap(src_off[s], bytes[s], dst_off[s], bytes[s]), kRefusedOverlap);
        for (int64_t o = 0; o < count; ++o) {
            if (o == s) continue;
            REFUSE_IF(overlap(dst_off[s], bytes[s], dst_off[o], bytes[o]) || overlap(dst_off[s], bytes[s], src_off[o], bytes[o]), kRefusedOverlap);
        }
    }
    Image<uint8_t> image(img, img_len);
    HIP_OK(image.up());
    REFUSE_IF(reinterpret_cast<uintptr_t>(image.d) % kTrialUnit != 0, kRefusedIndex);
    TrialTable t;
    t.count = (int32_t)count;
    int64_t units = 0;
    for (int32_t s = 0; s < kTrialMaxSegments; ++s) {
        if (s < count) {
            t.seg[s] = TrialSegment{image.d + src_off[s], image.d + dst_off[s], bytes[s]};
            units += bytes[s] / kTrialUnit;
        } else {
            t.seg[s] = TrialSegment{nullptr, nullptr, 0};
        }
        t.unit_end[s] = units;
    }
    launch_tab_trial_copy(t, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(image.back());
    return 0;
}

}  // extern "C"
