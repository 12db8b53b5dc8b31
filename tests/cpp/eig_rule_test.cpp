// The rule of the block shift-invert Lanczos (csrc/eig_rule.hpp) as a
// stand-alone CPU program: the symmetric eigen-solver against the analytic
// eigenvalues of the 12 x 12 (-1, 2, -1) matrix, on a double eigenvalue and
// on 1 x 1; the Cholesky rank rule on a full-rank Gram matrix, on two equal
// columns and on a zero block; the stop rule; the argument checks; and the
// whole loop on the host with a dense operator on the 5 x 5-grid Poisson
// matrix, which must return both copies of the double eigenvalues with block
// 4 and must not with block 1. Built with -fsanitize=address,undefined by
// tests/test_eig_rule.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "eig_rule.hpp"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) {                                                               \
            ++g_fail;                                                                \
            std::fprintf(stderr, "  CHECK failed: %s (line %d)\n", #cond, __LINE__); \
        }                                                                            \
    } while (0)

using Mat = std::vector<double>;  // row-major
static const double PI = 3.14159265358979323846;

// G = X^T Y for n x p blocks
static Mat gram(int n, int p, const Mat& X, const Mat& Y) {
    Mat g((size_t)p * p, 0.0);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < p; ++c)
            for (int d = 0; d < p; ++d) g[(size_t)c * p + d] += X[(size_t)r * p + c] * Y[(size_t)r * p + d];
    return g;
}

// W = W U
static void times(int n, int p, Mat& W, const Mat& U) {
    Mat out((size_t)n * p, 0.0);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < p; ++c)
            for (int d = 0; d < p; ++d) out[(size_t)r * p + d] += W[(size_t)r * p + c] * U[(size_t)c * p + d];
    W = out;
}

// Cholesky-QR twice; B = R2 R1; false when the block has lost rank (G_out: the Gram matrix it had)
static bool orthonormalise(int n, int p, Mat& W, const Mat& norm2, Mat& B, Mat& G_out) {
    Mat R1((size_t)p * p), R2((size_t)p * p), U((size_t)p * p);
    G_out = gram(n, p, W, W);
    if (!bsm::eig_chol_rank(p, G_out.data(), norm2.data(), R1.data(), U.data())) return false;
    times(n, p, W, U);
    const Mat G2 = gram(n, p, W, W);
    if (!bsm::eig_chol_rank(p, G2.data(), nullptr, R2.data(), U.data())) return false;
    times(n, p, W, U);
    B.assign((size_t)p * p, 0.0);
    bsm::eig_mul_upper(p, R2.data(), R1.data(), B.data());
    return true;
}

static Mat diag_of(int p, const Mat& G) {
    Mat d((size_t)p);
    for (int c = 0; c < p; ++c) d[(size_t)c] = G[(size_t)c * p + c];
    return d;
}

struct Run {
    std::vector<double> lam;
    int steps = 0, m = 0, converged = 0;
    bool exhausted = false;
    double orth = 0.0;  // max |V^T V - I|
};

// the loop of kernels_eig.hip, with a dense n x n operator for A^-1
static Run lanczos(int n, const Mat& Ainv, int nev, int p, int ncv, double tol, uint64_t seed) {
    Run out;
    bsm::EigLoop loop;
    loop.init(p, nev, ncv, tol);
    std::vector<Mat> V;
    Mat W((size_t)n * p), B, G;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < p; ++c) W[(size_t)r * p + c] = bsm::eig_start_value(seed, (uint64_t)r, (uint64_t)c);
    if (!orthonormalise(n, p, W, diag_of(p, gram(n, p, W, W)), B, G)) {
        out.exhausted = true;
        return out;
    }
    V.push_back(W);
    for (;;) {
        const Mat& Vj = V.back();
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < p; ++c) {
                double v = 0.0;
                for (int k = 0; k < n; ++k) v += Ainv[(size_t)r * n + k] * Vj[(size_t)k * p + c];
                W[(size_t)r * p + c] = v;
            }
        const Mat norm2 = diag_of(p, gram(n, p, W, W));
        Mat a_raw((size_t)p * p, 0.0);
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<Mat> C;
            for (const Mat& Vb : V) C.push_back(gram(n, p, Vb, W));
            for (size_t b = 0; b < V.size(); ++b)
                for (int r = 0; r < n; ++r)
                    for (int c = 0; c < p; ++c)
                        for (int d = 0; d < p; ++d)
                            W[(size_t)r * p + d] -= V[b][(size_t)r * p + c] * C[b][(size_t)c * p + d];
            for (int i = 0; i < p * p; ++i) a_raw[(size_t)i] += C.back()[(size_t)i];
        }
        const bool full = orthonormalise(n, p, W, norm2, B, G);
        loop.push(a_raw.data(), full ? B.data() : nullptr);
        if (!full) {
            out.exhausted = true;
            loop.ritz(G.data());
            break;
        }
        if (loop.check_due(loop.steps)) {
            loop.ritz();
            if (loop.done()) break;
        }
        if (!loop.room()) break;
        V.push_back(W);
    }
    if (loop.m_ritz != loop.m()) loop.ritz();
    for (int i = 0; i < std::min(nev, loop.m()); ++i) out.lam.push_back(1.0 / loop.theta_of(i));
    std::sort(out.lam.begin(), out.lam.end());
    out.steps = loop.steps;
    out.m = loop.m();
    out.converged = loop.converged();
    for (size_t a = 0; a < V.size(); ++a)
        for (size_t b = 0; b < V.size(); ++b) {
            const Mat g = gram(n, p, V[a], V[b]);
            for (int c = 0; c < p; ++c)
                for (int d = 0; d < p; ++d)
                    out.orth = std::max(out.orth, std::fabs(g[(size_t)c * p + d] - (a == b && c == d ? 1.0 : 0.0)));
        }
    return out;
}

// the inverse of a dense symmetric positive definite matrix by Gauss-Jordan
static Mat inverse(int n, Mat a) {
    Mat inv((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) inv[(size_t)i * n + i] = 1.0;
    for (int k = 0; k < n; ++k) {
        const double piv = a[(size_t)k * n + k];
        for (int j = 0; j < n; ++j) {
            a[(size_t)k * n + j] /= piv;
            inv[(size_t)k * n + j] /= piv;
        }
        for (int i = 0; i < n; ++i) {
            if (i == k) continue;
            const double f = a[(size_t)i * n + k];
            for (int j = 0; j < n; ++j) {
                a[(size_t)i * n + j] -= f * a[(size_t)k * n + j];
                inv[(size_t)i * n + j] -= f * inv[(size_t)k * n + j];
            }
        }
    }
    return inv;
}

int main() {
    {  // the (-1, 2, -1) matrix of order 12: 2 - 2 cos(j pi / 13), to 16 ulp of ||T|| = 4
        const int m = 12;
        Mat a((size_t)m * m, 0.0), w, z;
        for (int i = 0; i < m; ++i) {
            a[(size_t)i * m + i] = 2.0;
            if (i + 1 < m) a[(size_t)i * m + i + 1] = a[(size_t)(i + 1) * m + i] = -1.0;
        }
        const Mat a0 = a;
        bsm::eig_sym_solve(m, a, w, z);
        double worst = 0.0, res = 0.0, orth = 0.0;
        for (int j = 1; j <= m; ++j) worst = std::max(worst, std::fabs(w[(size_t)j - 1] - (2.0 - 2.0 * std::cos(j * PI / 13))));
        for (int i = 0; i < m; ++i)
            for (int r = 0; r < m; ++r) {
                double v = -w[(size_t)i] * z[(size_t)r * m + i], d = 0.0;
                for (int k = 0; k < m; ++k) {
                    v += a0[(size_t)r * m + k] * z[(size_t)k * m + i];
                    d += z[(size_t)k * m + i] * z[(size_t)k * m + r];
                }
                res = std::max(res, std::fabs(v));
                orth = std::max(orth, std::fabs(d - (i == r ? 1.0 : 0.0)));
            }
        std::printf("tridiagonal 12: eigenvalue error %.3e, residual %.3e, orthogonality %.3e\n", worst, res, orth);
        CHECK(worst <= 16 * 0x1p-53 * 4);
        CHECK(res <= 64 * 0x1p-53 * 4);
        CHECK(orth <= 64 * 0x1p-53);
    }
    {  // a double eigenvalue: Q diag(1, 3, 3, 7) Q^T with Q a Householder reflector
        const int m = 4;
        const double d[4] = {1.0, 3.0, 3.0, 7.0}, u[4] = {0.5, -0.5, 0.5, 0.5};
        Mat a((size_t)m * m, 0.0), w, z;
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j)
                for (int k = 0; k < m; ++k)
                    a[(size_t)i * m + j] += ((i == k) - 2.0 * u[i] * u[k]) * d[k] * ((k == j) - 2.0 * u[k] * u[j]);
        bsm::eig_sym_solve(m, a, w, z);
        for (int i = 0; i < m; ++i) CHECK(std::fabs(w[(size_t)i] - d[i]) <= 16 * 0x1p-53 * 7);
        double dot = 0.0;
        for (int r = 0; r < m; ++r) dot += z[(size_t)r * m + 1] * z[(size_t)r * m + 2];
        CHECK(std::fabs(dot) <= 16 * 0x1p-53);  // the double value's vectors are orthogonal
    }
    {  // 1 x 1
        Mat a{-2.5}, w, z;
        bsm::eig_sym_solve(1, a, w, z);
        CHECK(w.size() == 1 && w[0] == -2.5 && z.size() == 1 && z[0] == 1.0);
    }
    {  // the Cholesky rank rule
        const int p = 3;
        Mat R((size_t)p * p), U((size_t)p * p);
        const Mat full{4, 2, 0, 2, 5, 1, 0, 1, 3};
        const Mat n2{4, 5, 3};
        CHECK(bsm::eig_chol_rank(p, full.data(), n2.data(), R.data(), U.data()) == 1);
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j) {
                double g = 0.0, id = 0.0;
                for (int k = 0; k < p; ++k) {
                    g += R[(size_t)k * p + i] * R[(size_t)k * p + j];
                    id += R[(size_t)i * p + k] * U[(size_t)k * p + j];
                }
                CHECK(std::fabs(g - full[(size_t)i * p + j]) <= 1e-14);
                CHECK(std::fabs(id - (i == j ? 1.0 : 0.0)) <= 1e-14);
                if (i > j) CHECK(R[(size_t)i * p + j] == 0.0 && U[(size_t)i * p + j] == 0.0);
            }
        // the same columns, almost all of them projected away: a pivot at 2^-52 of the norm before
        const Mat huge{4 * 0x1p52, 5 * 0x1p52, 3 * 0x1p52};
        CHECK(bsm::eig_chol_rank(p, full.data(), huge.data(), R.data(), U.data()) == 0);
        CHECK(R[0] == 0.0 && U[0] == 1.0 && U[4] == 1.0 && U[1] == 0.0);
        const Mat edge{4 * 0x1p49, 5 * 0x1p49, 3 * 0x1p49};  // pivots above 2^-50 of it: kept
        CHECK(bsm::eig_chol_rank(p, full.data(), edge.data(), R.data(), U.data()) == 1);
        const Mat twins{1, 1, 0, 1, 1, 0, 0, 0, 1};  // two equal columns
        const Mat ones{1, 1, 1};
        CHECK(bsm::eig_chol_rank(p, twins.data(), ones.data(), R.data(), U.data()) == 0);
        const Mat zero((size_t)p * p, 0.0), zeros((size_t)p, 0.0);  // a zero block
        CHECK(bsm::eig_chol_rank(p, zero.data(), zeros.data(), R.data(), U.data()) == 0);
        CHECK(bsm::eig_chol_rank(p, zero.data(), nullptr, R.data(), U.data()) == 0);
        const Mat nan{std::numeric_limits<double>::quiet_NaN(), 0, 0, 0, 1, 0, 0, 0, 1};
        CHECK(bsm::eig_chol_rank(p, nan.data(), nullptr, R.data(), U.data()) == 0);
        double r1[1], u1[1];
        const double g1[1] = {9.0};
        CHECK(bsm::eig_chol_rank(1, g1, g1, r1, u1) == 1 && r1[0] == 3.0 && u1[0] == 1.0 / 3.0);
    }
    {  // the stop rule: T = diag(2, 1) with B_next = [[0.5]]: est_i = 0.5 |s_i[last]| / theta_i
        bsm::EigLoop loop;
        loop.init(1, 1, 4, 0.1);
        CHECK(loop.check_due(1) && loop.room() && !loop.done());
        const double a0[1] = {2.0}, a1[1] = {1.0}, b0[1] = {0.0}, b1[1] = {0.5};
        loop.push(a0, b0);
        loop.push(a1, b1);
        CHECK(loop.steps == 2 && loop.m() == 2 && loop.room());
        loop.ritz();
        CHECK(loop.est.size() == 1 && loop.theta_of(0) == 2.0 && loop.est[0] == 0.0);  // s = e_0: nothing in the last row
        CHECK(loop.done() && loop.converged() == 1);
        loop.init(1, 2, 2, 0.1);
        CHECK(!loop.check_due(1) && loop.check_due(2));
        loop.push(a0, b0);
        loop.push(a1, b1);
        CHECK(!loop.room());
        loop.ritz();
        CHECK(loop.est.size() == 2 && loop.est[0] == 0.0 && loop.est[1] == 0.5);  // theta 1, s = e_1
        CHECK(!loop.done() && loop.converged() == 1);
        loop.tol = 0.5;
        CHECK(loop.done());
        const double gram1[1] = {0.25};  // an exhausted block: sqrt(s G s) stands for ||B s||
        loop.ritz(gram1);
        CHECK(loop.est[1] == 0.5);
        loop.est[1] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!loop.done());
    }
    {  // the argument checks
        uint64_t m = 0;
        CHECK(bsm::eig_check_args(25, 6, 4, 0, 0.0, &m) == bsm::EIG_ARG_OK && m == 24);
        CHECK(bsm::eig_check_args(1000, 6, 4, 0, 1e-3, &m) == bsm::EIG_ARG_OK && m == 128);
        CHECK(bsm::eig_check_args(1000, 6, 4, 63, 0.0, &m) == bsm::EIG_ARG_OK && m == 60);
        CHECK(bsm::eig_check_args(25, 6, 4, 0, -1.0, &m) == bsm::EIG_ARG_TOL);
        CHECK(bsm::eig_check_args(25, 6, 4, 0, std::nan(""), &m) == bsm::EIG_ARG_TOL);
        CHECK(bsm::eig_check_args(25, 0, 4, 0, 0.0, &m) == bsm::EIG_ARG_NEV);
        CHECK(bsm::eig_check_args(25, 6, 0, 0, 0.0, &m) == bsm::EIG_ARG_BLOCK);
        CHECK(bsm::eig_check_args(25, 6, 33, 0, 0.0, &m) == bsm::EIG_ARG_BLOCK);
        CHECK(bsm::eig_check_args(25, 6, 4, 7, 0.0, &m) == bsm::EIG_ARG_NCV);   // rounds to 4 < nev
        CHECK(bsm::eig_check_args(25, 6, 4, 28, 0.0, &m) == bsm::EIG_ARG_NCV);  // > n
        CHECK(bsm::eig_check_args(25, 25, 4, 0, 0.0, &m) == bsm::EIG_ARG_NCV);  // the default rounds to 24 < nev
        CHECK(bsm::eig_check_args(0, 0, 4, 0, 0.0, &m) == bsm::EIG_ARG_OK && m == 0);
        CHECK(bsm::eig_check_args(0, 1, 4, 0, 0.0, &m) == bsm::EIG_ARG_NEV);
        CHECK(bsm::eig_check_args(0, 0, 4, 4, 0.0, &m) == bsm::EIG_ARG_NCV);
        CHECK(bsm::eig_default_tol(true) == 0x1p-26 && bsm::eig_default_tol(false) == 0x1p-12);
        for (uint64_t r = 0; r < 50; ++r) {
            const double v = bsm::eig_start_value(3, r, r % 4);
            CHECK(v >= -1.0 && v < 1.0);
        }
    }
    {  // the whole loop on the 5 x 5-grid Poisson matrix: lambda(p, q) = 4 - 2 cos(p pi / 6) - 2 cos(q pi / 6)
        const int g = 5, n = g * g;
        Mat a((size_t)n * n, 0.0);
        for (int i = 0; i < g; ++i)
            for (int j = 0; j < g; ++j) {
                const int r = i * g + j;
                a[(size_t)r * n + r] = 4.0;
                if (i > 0) a[(size_t)r * n + r - g] = -1.0;
                if (i + 1 < g) a[(size_t)r * n + r + g] = -1.0;
                if (j > 0) a[(size_t)r * n + r - 1] = -1.0;
                if (j + 1 < g) a[(size_t)r * n + r + 1] = -1.0;
            }
        const Mat ainv = inverse(n, a);
        std::vector<double> exact;
        for (int p = 1; p <= g; ++p)
            for (int q = 1; q <= g; ++q) exact.push_back(4.0 - 2.0 * std::cos(p * PI / 6) - 2.0 * std::cos(q * PI / 6));
        std::sort(exact.begin(), exact.end());
        CHECK(std::fabs(exact[1] - exact[2]) < 1e-14 && std::fabs(exact[4] - exact[5]) < 1e-14);  // the double ones
        const int nev = 6;
        const Run b4 = lanczos(n, ainv, nev, 4, 24, 0x1p-26, 0);
        std::printf("block 4: %d steps, %d columns, %d converged, orthogonality %.3e\n", b4.steps, b4.m, b4.converged,
                    b4.orth);
        // (24 of the 25 dimensions: the last block may well have lost rank, which `exhausted` reports)
        CHECK((int)b4.lam.size() == nev && b4.converged == nev);
        CHECK(b4.orth <= 1e-13);
        for (int i = 0; i < nev && i < (int)b4.lam.size(); ++i) {
            std::printf("  lambda %d: %.16f, exact %.16f\n", i, b4.lam[(size_t)i], exact[(size_t)i]);
            CHECK(std::fabs(b4.lam[(size_t)i] - exact[(size_t)i]) <= 1e-12);  // tol^2 kappa, far above rounding
        }
        // one vector sees one copy of each eigenvalue: the list it returns is not the 6 smallest
        const Run b1 = lanczos(n, ainv, nev, 1, 24, 0x1p-26, 0);
        std::printf("block 1: %d steps, %d columns, exhausted %d\n", b1.steps, b1.m, (int)b1.exhausted);
        bool missed = b1.lam.size() != (size_t)nev;
        for (int i = 0; i < nev && i < (int)b1.lam.size(); ++i)
            missed = missed || std::fabs(b1.lam[(size_t)i] - exact[(size_t)i]) > 1e-6;
        CHECK(missed);
        CHECK(b1.lam.size() >= 2 && std::fabs(b1.lam[0] - exact[0]) <= 1e-12 &&
              std::fabs(b1.lam[1] - exact[1]) <= 1e-12);        // it does find each distinct value once
        CHECK(b1.lam.size() >= 3 && std::fabs(b1.lam[2] - exact[3]) <= 1e-12);  // lambda_3 is (2, 2)'s, not the second (1, 2)
    }
    std::printf("summary: %d failed, %d checks\n", g_fail, g_checks);
    return g_fail ? 1 : 0;
}
