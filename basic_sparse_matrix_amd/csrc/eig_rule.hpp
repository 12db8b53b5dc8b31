// eig_rule.hpp -- the rule of the block shift-invert Lanczos on a kept factor
// (bsm_nd_factor_eigsh, kernels_eig.hip): the argument checks, the start
// block's values, the p x p Cholesky of a Gram matrix with its rank rule, the
// block-tridiagonal matrix T, the symmetric eigen-solver of T (cyclic Jacobi,
// plain C++), the residual estimate of a Ritz pair and the stop rule, and the
// generalised problem's test of its mass matrix (bsm_nd_factor_eigsh_gen).
// Header-only and free of device types, as pcg_rule.hpp: a plain C++ program
// drives the whole loop through it with a dense operator
// (tests/cpp/eig_rule_test.cpp), the device's one-workgroup judge calls the
// Cholesky, and the host loop of kernels_eig.hip calls the rest.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "bsm_synth.h"
#include "refine_rule.hpp"

namespace bsm {

constexpr uint64_t EIG_MAX_BLOCK = 32;
constexpr uint64_t EIG_DEFAULT_NCV = 128;
constexpr uint64_t EIG_MAX_NCV = 8192;  // the Ritz problem is dense on the host: 8192^2 f64 are 512 MiB
constexpr uint64_t EIG_SALT_START = 6;  // bsm_hash's salt of the start block (bsm_synth.h ends at 5)
constexpr uint32_t EIG_EXHAUSTED = 1u;  // info[3] bit 0: the block lost rank, the Krylov space is invariant
constexpr uint32_t EIG_INEXACT = 2u;    // info[3] bit 1: a solve's backward error ended above the refined solve's tol
constexpr double EIG_RANK_TOL = 0x1p-50;  // pivot <= this x the column's squared norm before the projections

// ---- arguments -----------------------------------------------------------------
enum EigArg { EIG_ARG_OK = 0, EIG_ARG_TOL, EIG_ARG_NEV, EIG_ARG_BLOCK, EIG_ARG_NCV };

inline const char* eig_arg_name(EigArg a) {
    switch (a) {
        case EIG_ARG_TOL: return "tol must be >= 0 (0 = the default)";
        case EIG_ARG_NEV: return "nev must be >= 1 (0 for an empty matrix, and only then)";
        case EIG_ARG_BLOCK: return "block must be in 1..32";
        case EIG_ARG_NCV: return "ncv (rounded down to a multiple of block) must be in nev..n";
        default: return "";
    }
}

// sqrt of the unit roundoff of a's dtype
inline double eig_default_tol(bool f64) { return f64 ? 0x1p-26 : 0x1p-12; }

// ncv == 0: min(n, 128); either way rounded down to a multiple of block
inline uint64_t eig_ncv_in_use(uint64_t n, uint64_t block, uint64_t ncv) {
    if (ncv == 0) ncv = std::min<uint64_t>(n, EIG_DEFAULT_NCV);
    return ncv / block * block;
}

// The checks that need no matrix. n == 0 is accepted with nev == 0 (nothing
// is computed); *ncv_out is the basis size in use.
inline EigArg eig_check_args(uint64_t n, uint64_t nev, uint64_t block, uint64_t ncv, double tol, uint64_t* ncv_out) {
    if (!(tol >= 0.0)) return EIG_ARG_TOL;
    if (block < 1 || block > EIG_MAX_BLOCK) return EIG_ARG_BLOCK;
    if (n == 0 ? nev != 0 : nev < 1) return EIG_ARG_NEV;
    const uint64_t m = eig_ncv_in_use(n, block, ncv);
    if (m < nev || m > n) return EIG_ARG_NCV;
    *ncv_out = m;
    return EIG_ARG_OK;
}

// ---- the start block -----------------------------------------------------------
// uniform in [-1, 1) from 53 hash bits; exact on host and device
BSM_RULE_HD inline double eig_start_value(uint64_t seed, uint64_t row, uint64_t col) {
    return 2.0 * (bsm_unit_uniform(bsm_hash(seed, row, col, EIG_SALT_START)) - 1.0);
}

// ---- Cholesky-QR's p x p part --------------------------------------------------
// G = R^T R with R upper triangular, and U = R^-1 (both p x p row-major, the
// strict lower parts zero); G's upper triangle is read. norm2 (or null): the
// columns' squared norms before the projections; a pivot <= EIG_RANK_TOL x
// norm2[j] means the block has lost rank (sine of the angle <= 2^-25: one
// Cholesky-QR pass has no orthogonality left). A pivot that is not positive
// and finite always does. Returns 1 for full rank; 0 leaves R = 0, U = I.
BSM_RULE_HD inline int eig_chol_rank(int p, const double* G, const double* norm2, double* R, double* U) {
    int ok = 1;
    for (int i = 0; i < p * p; ++i) R[i] = 0.0;
    for (int j = 0; j < p && ok; ++j) {
        for (int i = 0; i < j; ++i) {
            double v = G[i * p + j];
            for (int k = 0; k < i; ++k) v -= R[k * p + i] * R[k * p + j];
            R[i * p + j] = v / R[i * p + i];
        }
        double d = G[j * p + j];
        for (int k = 0; k < j; ++k) d -= R[k * p + j] * R[k * p + j];
        if (!(d > 0.0) || !std::isfinite(d) || (norm2 && d <= EIG_RANK_TOL * norm2[j])) ok = 0;
        else R[j * p + j] = std::sqrt(d);
    }
    for (int i = 0; i < p * p; ++i) U[i] = 0.0;
    if (!ok) {
        for (int i = 0; i < p * p; ++i) R[i] = 0.0;
        for (int i = 0; i < p; ++i) U[i * p + i] = 1.0;
        return 0;
    }
    for (int j = 0; j < p; ++j) {
        U[j * p + j] = 1.0 / R[j * p + j];
        for (int i = j - 1; i >= 0; --i) {
            double v = 0.0;
            for (int k = i + 1; k <= j; ++k) v += R[i * p + k] * U[k * p + j];
            U[i * p + j] = -v / R[i * p + i];
        }
    }
    return 1;
}

// B = R2 R1 (upper triangular): W_before = V_next B
inline void eig_mul_upper(int p, const double* R2, const double* R1, double* B) {
    for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) {
            double v = 0.0;
            for (int k = i; k <= j; ++k) v += R2[i * p + k] * R1[k * p + j];
            B[i * p + j] = v;
        }
}

// ---- the generalised problem's mass matrix ---------------------------------------
// S y = lambda S_M y (bsm_nd_factor_eigsh_gen) runs the same loop in the S_M
// inner product, and norm2[c] = w_c^T S_M w_c of a block's p columns is then a
// squared norm. One that is <= 0 or not finite shows that S_M is not positive
// definite (a zero column of a caller's start block reads the same).
inline bool eig_mass_pd(int p, const double* norm2) {
    for (int c = 0; c < p; ++c)
        if (!(norm2[c] > 0.0) || !std::isfinite(norm2[c])) return false;
    return true;
}

// ---- the symmetric eigen-solver -------------------------------------------------
// Cyclic Jacobi on a dense symmetric m x m matrix (row-major, overwritten):
// w ascending, Z's column i (Z[r * m + i]) the unit eigenvector of w[i].
inline void eig_sym_solve(int m, std::vector<double>& A, std::vector<double>& w, std::vector<double>& Z) {
    std::vector<double> V((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) V[(size_t)i * m + i] = 1.0;
    auto at = [&](int r, int c) -> double& { return A[(size_t)r * m + c]; };
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < m; ++p)
            for (int q = p + 1; q < m; ++q) off += std::fabs(at(p, q));
        if (off == 0.0) break;
        for (int p = 0; p < m; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = at(p, q);
                if (apq == 0.0) continue;
                const double g = 100.0 * std::fabs(apq), app = at(p, p), aqq = at(q, q);
                // an entry that no longer moves either diagonal is dropped (Rutishauser)
                if (sweep > 3 && std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
                    at(p, q) = at(q, p) = 0.0;
                    continue;
                }
                const double h = aqq - app;
                double t;
                if (std::fabs(h) + g == std::fabs(h)) {
                    t = apq / h;
                } else {
                    const double theta = 0.5 * h / apq;
                    t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                }
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
                at(p, p) = app - t * apq;
                at(q, q) = aqq + t * apq;
                at(p, q) = at(q, p) = 0.0;
                for (int r = 0; r < m; ++r) {
                    if (r != p && r != q) {
                        const double arp = at(r, p), arq = at(r, q);
                        at(r, p) = at(p, r) = arp - s * (arq + tau * arp);
                        at(r, q) = at(q, r) = arq + s * (arp - tau * arq);
                    }
                    const double vrp = V[(size_t)r * m + p], vrq = V[(size_t)r * m + q];
                    V[(size_t)r * m + p] = vrp - s * (vrq + tau * vrp);
                    V[(size_t)r * m + q] = vrq + s * (vrp - tau * vrq);
                }
            }
    }
    std::vector<int> order((size_t)m);
    for (int i = 0; i < m; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return at(a, a) < at(b, b); });
    w.assign((size_t)m, 0.0);
    Z.assign((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) {
        const int src = order[(size_t)i];
        w[(size_t)i] = at(src, src);
        for (int r = 0; r < m; ++r) Z[(size_t)r * m + i] = V[(size_t)r * m + src];
    }
}

// ---- the loop's host state -------------------------------------------------------
// T, block tridiagonal in the basis V_0, V_1, ...: A^-1 V_j = V_{j-1} B_j^T +
// V_j A_j + V_{j+1} B_{j+1}. After step j (0-based) the caller gives A_j (the
// summed projections onto V_j, symmetrised here) and, unless the block lost
// rank, B_{j+1} = R2 R1; `ritz` solves the leading m x m part.
struct EigLoop {
    int p = 0;         // block
    int nev = 0;       // wanted pairs
    int ncv = 0;       // the basis columns at most, a multiple of p
    double tol = 0.0;  // on est
    int steps = 0;     // completed: the basis so far has steps * p columns
    std::vector<double> T;          // ncv x ncv row-major
    std::vector<double> Bnext;      // B_{steps}: p x p (what the latest step's W left outside the basis)
    std::vector<double> theta, S;   // the latest Ritz solve: ascending, eigenvectors in columns, of size m_ritz
    int m_ritz = 0;
    std::vector<double> est;        // of the nev largest theta, the largest first

    void init(int block, int nev_, int ncv_, double tol_) {
        p = block;
        nev = nev_;
        ncv = ncv_;
        tol = tol_;
        steps = 0;
        m_ritz = 0;
        T.assign((size_t)ncv * ncv, 0.0);
        Bnext.assign((size_t)p * p, 0.0);
        est.clear();
    }
    int m() const { return steps * p; }

    // step `steps` is done: its A block and (b_next non-null) the next B block
    void push(const double* a_raw, const double* b_next) {
        const int o = steps * p;
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j) T[(size_t)(o + i) * ncv + o + j] = 0.5 * (a_raw[i * p + j] + a_raw[j * p + i]);
        for (int i = 0; i < p * p; ++i) Bnext[(size_t)i] = b_next ? b_next[i] : 0.0;
        if (b_next && o + 2 * p <= ncv)
            for (int i = 0; i < p; ++i)
                for (int j = 0; j < p; ++j) {
                    T[(size_t)(o + p + i) * ncv + o + j] = b_next[i * p + j];
                    T[(size_t)(o + j) * ncv + o + p + i] = b_next[i * p + j];
                }
        ++steps;
    }

    // When the Ritz check runs depends on the step number alone (1-based
    // `step`): at every step that has nev columns.
    bool check_due(int step) const { return step * p >= nev; }

    // T s = theta s on the basis so far, and est_i = ||B_next s_i[last p rows]||2 / |theta_i|
    // of the nev largest. gram (or null): the exhausted block's W^T W, which
    // stands for B^T B (no Cholesky of it exists).
    void ritz(const double* gram = nullptr) {
        const int mm = m();
        std::vector<double> A((size_t)mm * mm);
        for (int i = 0; i < mm; ++i)
            for (int j = 0; j < mm; ++j) A[(size_t)i * mm + j] = T[(size_t)i * ncv + j];
        eig_sym_solve(mm, A, theta, S);
        m_ritz = mm;
        const int cnt = std::min(nev, mm);
        est.assign((size_t)cnt, 0.0);
        for (int i = 0; i < cnt; ++i) {
            const int col = mm - 1 - i;
            const double* last = &S[(size_t)(mm - p) * mm + col];  // rows mm - p .., stride mm
            double sum = 0.0;
            if (gram) {
                for (int r = 0; r < p; ++r)
                    for (int c = 0; c < p; ++c) sum += last[(size_t)r * mm] * gram[r * p + c] * last[(size_t)c * mm];
                sum = std::max(sum, 0.0);
            } else {
                for (int r = 0; r < p; ++r) {
                    double v = 0.0;
                    for (int c = r; c < p; ++c) v += Bnext[(size_t)r * p + c] * last[(size_t)c * mm];
                    sum += v * v;
                }
            }
            est[(size_t)i] = std::sqrt(sum) / std::fabs(theta[(size_t)col]);
        }
    }

    // the pairs among the nev wanted whose estimate is at or below tol
    int converged() const {
        int c = 0;
        for (double e : est) c += e <= tol;  // false for NaN
        return c;
    }
    // after a Ritz check: every wanted pair is there and at or below tol
    bool done() const { return (int)est.size() == nev && converged() == nev; }
    // another block fits into the basis
    bool room() const { return m() + p <= ncv; }
    // wanted pair i (0 = the largest theta = the smallest lambda): theta and its column of S
    double theta_of(int i) const { return theta[(size_t)(m_ritz - 1 - i)]; }
    double s_of(int i, int row) const { return S[(size_t)row * m_ritz + (m_ritz - 1 - i)]; }
};

}  // namespace bsm
