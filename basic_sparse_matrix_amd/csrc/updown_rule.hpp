// updown_rule.hpp -- the scalar rule of the rank-k update and downdate of a
// kept factor (bsm_nd_factor_updown, kernels_nd_updown.hip): the
// column-by-column method (Gill, Golub, Murray, Saunders, method C1) for
// L L^T + sigma w w^T, sigma = +1 or -1. At pivot j
//     d = L_jj;  r = sqrt(d^2 + sigma w_j^2);  c = r / d;  s = w_j / d;  L_jj = r
// and for every row i > j
//     L_ij = (L_ij + sigma s w_i) / c;   w_i = c w_i - s L_ij   (the new L_ij)
// w_j == 0 skips the pivot (c = 1, s = 0: nothing is read or rounded, so
// padding pivots and inactive columns keep their bits). Explicit fma, one
// order: the same input gives the same bits. Header-only and free of device
// types, as pcg_rule.hpp: a plain C++ program drives it
// (tests/cpp/updown_rule_test.cpp) and the kernels call the same functions.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define BSM_UPDOWN_HD __host__ __device__
#else
#define BSM_UPDOWN_HD
#endif

namespace bsm {

BSM_UPDOWN_HD inline double updown_fma(double a, double b, double c) { return std::fma(a, b, c); }
BSM_UPDOWN_HD inline float updown_fma(float a, float b, float c) { return std::fma(a, b, c); }

// one pivot's coefficients; s == 0 marks a skipped pivot
template <typename T>
struct UpdownCoef {
    T c, s;
};

// r^2 <= 0 or not finite: sigma w w^T takes the matrix out of the positive definite ones at this pivot
template <typename T>
BSM_UPDOWN_HD inline bool updown_not_pd(T r2) {
    return !(r2 > (T)0) || !std::isfinite(r2);
}

// Pivot j: d = L_jj (in: the old one, out: the new one), wj = w_j. False:
// not positive definite (d and cs are then those of a skipped pivot).
template <typename T>
BSM_UPDOWN_HD inline bool updown_pivot(T& d, T wj, int sign, UpdownCoef<T>& cs) {
    cs.c = (T)1;
    cs.s = (T)0;
    if (wj == (T)0) return true;
    const T sw = sign < 0 ? -wj : wj;
    const T r2 = updown_fma(sw, wj, d * d);
    if (updown_not_pd(r2)) return false;
    const T r = std::sqrt(r2);
    cs.c = r / d;
    cs.s = wj / d;
    d = r;
    return true;
}

// Row i > j of pivot j: l = L_ij (in: old, out: new), wi = w_i (likewise)
template <typename T>
BSM_UPDOWN_HD inline void updown_row(T& l, T& wi, int sign, const UpdownCoef<T>& cs) {
    if (cs.s == (T)0) return;
    const T ss = sign < 0 ? -cs.s : cs.s;
    l = updown_fma(ss, wi, l) / cs.c;
    wi = updown_fma(-cs.s, l, cs.c * wi);
}

}  // namespace bsm
