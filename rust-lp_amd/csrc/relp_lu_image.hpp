// relp_lu_image.hpp -- the "ELL by pass" image of a schedule on the host side: an EllPacked (relp_lu.hpp: ell_pack) written as
// one contiguous image, and an image -- the host's or the device builder's (relp_lu_schedule_core.h) -- addressed as an
// EllSchedule.  Both go through luf_image_layout and nothing else.  Host files only.
#pragma once
#include <cstring>

#include "relp_lu.hpp"
#include "relp_lu_schedule_core.h"

namespace relp {

static_assert(sizeof(EllPassHost) == 16 && sizeof(EllPass) == 16, "the packed pass header is one 16-byte load");
static_assert(kEllLgShift == kEllLg && kEllLgShiftWide == kEllLgWide, "host packing and device decoding of sidx");

// the counts that fix an image's layout
struct EllImageShape {
    int32_t m, n_passes, n_levels, n_lanes, n_ovf;
    bool wide;                                             // 32-bit slot indices
    LufImageLayout layout() const { return luf_image_layout(m, n_passes, n_levels, n_lanes, n_ovf, wide); }
};
inline EllImageShape ell_image_shape(const EllPacked& e, int32_t m, bool wide) {
    return EllImageShape{m, (int32_t)e.passes.size(), (int32_t)e.lvl_pass.size() - 1, (int32_t)e.lanes(), (int32_t)e.overflow(), wide};
}

// e -> dst[0 .. layout().total): every array at its offset, the kEllPadHeaders empty headers and all padding zero.  False
// (nothing usable written) when an array of e has not the length the layout gives it.
inline bool ell_image_write(const EllPacked& e, const EllImageShape& s, char* dst) {
    const LufImageLayout L = s.layout();
    const size_t isz = s.wide ? 4 : 2, nl = (size_t)s.n_lanes, no = (size_t)s.n_ovf;
    if (e.rdiag.size() != (size_t)s.m + 1 || e.sval.size() != nl || e.oval.size() != no || e.rovf.size() != (no ? 2 * (size_t)s.m : 0) ||
        (s.wide ? e.sidx32.size() != nl || e.oidx32.size() != no : e.sidx.size() != nl || e.oidx.size() != no))
        return false;
    auto put = [dst](int64_t at, int64_t next, const void* src, size_t bytes) {
        if (bytes) std::memcpy(dst + at, src, bytes);
        std::memset(dst + at + bytes, 0, (size_t)(next - at) - bytes);
    };
    put(L.passes, L.lvl_pass, e.passes.data(), sizeof(EllPassHost) * e.passes.size());
    put(L.lvl_pass, L.rdiag, e.lvl_pass.data(), 4 * e.lvl_pass.size());
    put(L.rdiag, L.sval, e.rdiag.data(), 8 * e.rdiag.size());
    put(L.sval, L.oval, e.sval.data(), 8 * nl);
    put(L.oval, L.rovf, e.oval.data(), 8 * no);
    put(L.rovf, L.sidx, e.rovf.data(), 4 * e.rovf.size());
    put(L.sidx, L.oidx, s.wide ? (const void*)e.sidx32.data() : (const void*)e.sidx.data(), isz * nl);
    put(L.oidx, L.total, s.wide ? (const void*)e.oidx32.data() : (const void*)e.oidx.data(), isz * no);
    return true;
}

// the eight arrays of the image at `image`, its counts and its size -> d (the other members of d are the caller's)
inline void ell_image_view(char* image, const EllImageShape& s, EllSchedule* d) {
    const LufImageLayout L = s.layout();
    d->passes = reinterpret_cast<const EllPass*>(image + L.passes);
    d->lvl_pass = reinterpret_cast<const int32_t*>(image + L.lvl_pass);
    d->rdiag = reinterpret_cast<double*>(image + L.rdiag);
    d->sval = reinterpret_cast<double*>(image + L.sval);
    d->oval = reinterpret_cast<const double*>(image + L.oval);
    d->rovf = reinterpret_cast<const int32_t*>(image + L.rovf);
    d->sidx = reinterpret_cast<const uint16_t*>(image + L.sidx);       // (uint32_t when wide)
    d->oidx = reinterpret_cast<const uint16_t*>(image + L.oidx);
    d->n_passes = s.n_passes; d->n_levels = s.n_levels; d->m = s.m; d->n_lanes = s.n_lanes; d->n_ovf = s.n_ovf;
    d->bytes = (int32_t)L.total;
}

}  // namespace relp
