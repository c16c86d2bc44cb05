// relp_engine_internal.hpp -- helpers shared by the relp_engine*.cpp translation units.
#pragma once
#include "relp_engine.hpp"

namespace relp {

#define HIP_TRY(expr)                                                        \
    do {                                                                     \
        if (!hip_ok((expr), #expr)) return RELP_E_HIP;                       \
    } while (0)

// the last step of a function: RELP_OK, or the HIP failure
#define HIP_RETURN(expr) return hip_ok((expr), #expr) ? RELP_OK : RELP_E_HIP

static inline int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

}  // namespace relp
