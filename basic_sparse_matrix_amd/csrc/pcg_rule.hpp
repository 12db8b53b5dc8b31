// pcg_rule.hpp -- the per-column rule of the preconditioned conjugate
// gradients on a kept factor (bsm_nd_factor_solve_pcg, kernels_pcg.hip): what
// a column does with the dots and norms of a step -- its step length, its
// flexible beta, when it asks for its true residual, when it restarts, stops
// or has broken down. Header-only and free of device types, as
// refine_rule.hpp, whose scale and backward error it uses: a plain C++
// program drives it (tests/cpp/pcg_rule_test.cpp) and the device's
// one-workgroup reductions call the same functions.
#pragma once

#include "refine_rule.hpp"

namespace bsm {

// One right-hand column's state between the steps.
struct PcgCol {
    double bnorm = 0.0;      // ||b_j||inf
    double omega = 0.0;      // the latest iterate's backward error (of the recurrence's r unless `verified`)
    double rho = 0.0;        // r . z of the latest preconditioned residual
    double alpha = 0.0;      // the latest step length rho / (p . q)
    double beta = 0.0;       // the latest direction's p = z + beta p
    double scale = 1.0;      // 2^floor(log2 ||r_j||inf) of the residual the next solve gets (refine_scale)
    uint32_t iters = 0;      // the CG steps completed
    uint32_t active = 0;     // another step is wanted
    uint32_t verify = 0;     // the recurrence's omega is at or below tol: the true residual is asked for
    uint32_t restart = 0;    // the next direction is z alone (beta = 0): the first one, or r was replaced
    uint32_t breakdown = 0;  // p . q or r . z was <= 0 or not finite: S or the factor is not positive definite
    uint32_t zero = 0;       // b_j == 0: x_j = 0, berr 0, nothing solved
    uint32_t verified = 0;   // omega is the true residual's (b - S x formed anew)
};

BSM_RULE_HD inline bool pcg_positive(double v) { return v > 0.0 && std::isfinite(v); }

// The first iterate X_0 = M^-1 b with its true residual (refine's first
// iterate and refine_rule_init's omega: max_iter == 0 is solve_refined's).
BSM_RULE_HD inline void pcg_rule_init(PcgCol& c, double bnorm, double omega0, double rmax, double tol) {
    c = PcgCol{};
    c.bnorm = bnorm;
    c.zero = bnorm == 0.0;
    if (c.zero) omega0 = 0.0;
    c.omega = omega0;
    c.verified = 1;
    c.scale = refine_scale(rmax);
    c.restart = 1;  // the first direction is z
    c.active = !c.zero && refine_wants_more(omega0, tol);
}

// After z = M^-1 r: beta from q . z (flexible, with r_new - r_old = -alpha q),
// 0 for the first direction and after a restart; rho = r . z. A rho that is
// not positive stops the column: x stays that of its last completed step.
BSM_RULE_HD inline void pcg_rule_beta(PcgCol& c, double rz, double qz) {
    if (!c.active) return;
    double beta = 0.0;
    if (!c.restart) beta = -c.alpha * qz / c.rho;
    c.restart = 0;
    if (!pcg_positive(rz) || !std::isfinite(beta)) {
        c.active = 0;
        c.breakdown = 1;
        return;
    }
    c.beta = beta;
    c.rho = rz;
}

// After q = S p: alpha = rho / (p . q); p . q <= 0 or not finite is a breakdown.
BSM_RULE_HD inline void pcg_rule_alpha(PcgCol& c, double pq) {
    if (!c.active) return;
    const double alpha = pcg_positive(pq) ? c.rho / pq : 0.0;
    if (!pcg_positive(alpha)) {
        c.active = 0;
        c.breakdown = 1;
        return;
    }
    c.alpha = alpha;
}

// Step `it` (1-based) gave x += alpha p, r -= alpha q with the recurrence's
// backward error omega_rec. At or below tol the column asks for its true
// residual; a non-finite error stops it.
BSM_RULE_HD inline void pcg_rule_step(PcgCol& c, uint32_t it, double omega_rec, double rmax, double tol) {
    if (!c.active) return;
    c.iters = it;
    c.omega = omega_rec;
    c.verified = 0;
    c.scale = refine_scale(rmax);
    if (!std::isfinite(omega_rec)) c.active = 0;
    else if (omega_rec <= tol) c.verify = 1;
}

// The true residual of a column that asked: at or below tol it has converged,
// otherwise it goes on from the true residual (which replaces r) with beta = 0.
BSM_RULE_HD inline void pcg_rule_verified(PcgCol& c, double omega_true, double rmax_true, double tol) {
    if (!c.verify) return;
    c.verify = 0;
    c.omega = omega_true;
    c.verified = 1;
    if (!refine_wants_more(omega_true, tol)) {
        c.active = 0;
        return;
    }
    c.restart = 1;
    c.scale = refine_scale(rmax_true);
}

// The end: the true backward error of the returned x of a column that stopped
// without one (max_iter, a breakdown after a step, a non-finite recurrence).
BSM_RULE_HD inline void pcg_rule_final(PcgCol& c, double omega_true) {
    c.active = 0;
    c.verify = 0;
    if (c.zero || c.verified) return;
    c.omega = omega_true;
    c.verified = 1;
}

}  // namespace bsm
