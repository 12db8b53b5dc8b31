// refine_rule.hpp -- the per-column rule of the refined solve
// (bsm_nd_factor_solve_refined, kernels_refine.hip): the backward error of an
// iterate, the power-of-two scale of a residual, and which columns go on,
// have converged, have stagnated, and which iterate is the best so far.
// Header-only and free of device types, so that a plain C++ program can drive
// it (tests/cpp/refine_rule_test.cpp); the device's one-workgroup reduction
// calls the same functions.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BSM_RULE_HD __host__ __device__
#else
#define BSM_RULE_HD
#endif

namespace bsm {

// One right-hand column's state between the iterations.
struct RefineCol {
    double bnorm = 0.0;     // ||b_j||inf
    double omega = 0.0;     // the latest iterate's backward error
    double best = 0.0;      // the smallest backward error of any iterate: berr
    double scale = 1.0;     // 2^floor(log2 ||r_j||inf) of the latest residual (1 where that is 0 or not finite)
    uint32_t iters = 0;     // the corrections made
    uint32_t active = 0;    // another correction is wanted
    uint32_t use_prev = 0;  // the best iterate is the one before the latest
    uint32_t zero = 0;      // b_j == 0: x_j = 0, berr 0, nothing solved
};

// 2^floor(log2 v) for a finite v > 0, else 1: dividing by it is exact short
// of underflow, and v / scale lies in [1, 2)
BSM_RULE_HD inline double refine_scale(double v) {
    if (!(v > 0.0) || std::isinf(v)) return 1.0;
    int e = 0;
    (void)std::frexp(v, &e);  // v = m 2^e, m in [0.5, 1)
    return std::ldexp(1.0, e - 1);
}

// omega = ||r||inf / (||S||inf ||x||inf + ||b||inf); 0 / 0 (a zero system) is 0
BSM_RULE_HD inline double refine_omega(double rmax, double xmax, double bnorm, double snorm) {
    const double den = snorm * xmax + bnorm;
    if (rmax == 0.0 && den == 0.0) return 0.0;
    return rmax / den;
}

// a column goes on while its error is finite, above tol, and (LAPACK's
// stagnation rule, xPORFS) at most half the one before
BSM_RULE_HD inline bool refine_wants_more(double omega, double tol) { return std::isfinite(omega) && omega > tol; }

// The first iterate X_0 = M^-1 b.
BSM_RULE_HD inline void refine_rule_init(RefineCol& c, double bnorm, double omega0, double rmax, double tol) {
    c.bnorm = bnorm;
    c.iters = 0;
    c.use_prev = 0;
    c.zero = bnorm == 0.0;
    if (c.zero) omega0 = 0.0;
    c.omega = omega0;
    c.best = omega0;
    c.scale = refine_scale(rmax);
    c.active = !c.zero && refine_wants_more(omega0, tol);
}

// Correction `it` (1-based) of an active column gave an iterate of error
// omega_new. A non-finite error stops the column and is never the best.
BSM_RULE_HD inline void refine_rule_step(RefineCol& c, uint32_t it, double omega_new, double rmax, double tol) {
    if (!c.active) return;
    c.iters = it;
    const bool better = omega_new < c.best;  // false for NaN
    if (better) c.best = omega_new;
    c.use_prev = !better;
    c.active = refine_wants_more(omega_new, tol) && omega_new <= c.omega / 2;
    c.omega = omega_new;
    c.scale = refine_scale(rmax);
}

// tol == 0: the rounding bound of the f64 residual itself, gamma_{m+1} with m
// the longest row of S, below which omega is noise
BSM_RULE_HD inline double refine_default_tol(uint64_t max_row_len) {
    return (double)(max_row_len + 2) * 0x1p-53;
}

}  // namespace bsm
