// relp_gomory.hpp -- the host side of relp_gomory_cuts that needs no device (plain C++17, no HIP): the argument checks, what is
// decided once per list entry (its fraction f0 and whether it is skipped), the rows whose slack carries a coefficient out of the
// cut, and the right-hand side of the cut.  Engine::gomory_cuts is these steps around one launch_tab_gomory.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "relp_layout.hpp"

namespace relp {

// status[k] of relp_gomory_cuts
enum : int32_t { kGomoryCut = 0, kGomoryNotInteger = 1, kGomoryFraction = 2, kGomoryArtificial = 3, kGomoryContinuous = 4 };

// The RELP_E_ARG cases of relp_gomory_cuts (rows against m rows); nullptr when the arguments are in order.
inline const char* gomory_check_args(const int32_t* rows, int32_t count, int32_t m, int32_t kind, double away, const double* coefficients,
                                     const double* rhs, const int32_t* status) {
    if (count < 0) return "count < 0";
    if (kind != RELP_GOMORY_FRACTIONAL && kind != RELP_GOMORY_MIXED) return "kind is neither RELP_GOMORY_FRACTIONAL nor RELP_GOMORY_MIXED";
    if (!std::isfinite(away) || away < 0.0 || !(away < 0.5)) return "away outside [0, 0.5)";
    if (count > 0 && (!rows || !coefficients || !rhs || !status)) return "rows, coefficients, rhs or status missing";
    for (int32_t k = 0; k < count; ++k)
        if (rows[k] < 0 || rows[k] >= m) return "row out of range";
    return nullptr;
}

// What is decided once per list entry from b_r and the basic column of row r (a provider column, or a wrapped artificial index):
// *f0 = b_r - floor(b_r), and the status in the order 3 (a kept artificial is basic), 1 (the basic column is not flagged integer;
// is_integer == nullptr flags all), 2 (f0 < away or f0 > 1 - away), else 0.  Status 4 is the kernel's finding.
inline int32_t gomory_entry(double b_r, int32_t basic, const uint8_t* is_integer, int32_t n_provider, double away, double* f0) {
    *f0 = b_r - std::floor(b_r);
    if (basic >= kWrappedArtificialBase || basic < 0 || basic >= n_provider) return kGomoryArtificial;
    if (is_integer && !is_integer[basic]) return kGomoryNotInteger;
    if (*f0 < away || *f0 > 1.0 - away) return kGomoryFraction;
    return kGomoryCut;
}

// The rows whose slack takes a coefficient out of the cut: per engine row i the provider column of its slack and the sign sigma_i
// of that slack in the row, (-1, 0) for a row without one (an equality).  y_i = sigma_i * pi of that column.  From the descriptors
// the device reads (vrow0 / vsign); a range slack (two rows) and an added column (no row) are not substituted: the call refuses both.
inline void gomory_slack_rows(const Layout& lay, std::vector<int32_t>* column, std::vector<int32_t>* sign) {
    column->assign(lay.m, -1);
    sign->assign(lay.m, 0);
    for (int32_t v = 0; v < lay.nr_virtual; ++v) {
        const int32_t i = lay.vrow0[v];
        if (i < 0 || i >= lay.m || lay.vrow1[v] >= 0 || lay.added_of(lay.nr_normal + v) >= 0) continue;
        (*column)[i] = lay.nr_normal + v;
        (*sign)[i] = lay.vsign[v];
    }
}

// beta = -f0 + sum_i y_i rhs_i over the rows with y_i != 0 in ascending order, one fma per row from -f0.
inline double gomory_beta(double f0, const double* y, const double* rhs, int32_t m) {
    double beta = -f0;
    for (int32_t i = 0; i < m; ++i)
        if (y[i] != 0.0) beta = std::fma(y[i], rhs[i], beta);
    return beta;
}

}  // namespace relp
