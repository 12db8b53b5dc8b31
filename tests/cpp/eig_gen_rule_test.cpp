// The generalised problem A y = lambda M y through the rule of the block
// shift-invert Lanczos (csrc/eig_rule.hpp) as a stand-alone CPU program: the
// whole loop of kernels_eig.hip's eigsh_gen_t on the host, in the M inner
// product, with a dense A^-1 and a dense M, on the 9 x 9-grid Poisson matrix
// and its consistent mass matrix kron(M1, M1), M1 = tridiag(1/6, 4/6, 1/6).
// Block 4 must return both copies of the double eigenvalues, against values
// computed here by the header's own Jacobi solver on L_M^-1 A L_M^-T; the
// vectors must be M-orthonormal; and the positive-definiteness rule must fire
// on M = -I and on a zero block. Built with -fsanitize=address,undefined by
// tests/test_eig_gen_rule.py.
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

// G = X^T Y for n x p blocks
static Mat gram(int n, int p, const Mat& X, const Mat& Y) {
    Mat g((size_t)p * p, 0.0);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < p; ++c)
            for (int d = 0; d < p; ++d) g[(size_t)c * p + d] += X[(size_t)r * p + c] * Y[(size_t)r * p + d];
    return g;
}

// out = D X for a dense n x n D and an n x p block
static Mat apply(int n, int p, const Mat& D, const Mat& X) {
    Mat out((size_t)n * p, 0.0);
    for (int r = 0; r < n; ++r)
        for (int k = 0; k < n; ++k) {
            const double d = D[(size_t)r * n + k];
            if (d == 0.0) continue;
            for (int c = 0; c < p; ++c) out[(size_t)r * p + c] += d * X[(size_t)k * p + c];
        }
    return out;
}

// W = W U
static void times(int n, int p, Mat& W, const Mat& U) {
    Mat out((size_t)n * p, 0.0);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < p; ++c)
            for (int d = 0; d < p; ++d) out[(size_t)r * p + d] += W[(size_t)r * p + c] * U[(size_t)c * p + d];
    W = out;
}

static Mat diag_of(int p, const Mat& G) {
    Mat d((size_t)p);
    for (int c = 0; c < p; ++c) d[(size_t)c] = G[(size_t)c * p + c];
    return d;
}

// Cholesky-QR twice in the M inner product: W and Q = M W go through the two
// W R^-1 passes together (M (W U) = (M W) U); B = R2 R1; false when the block
// has lost rank (G_out: the Gram matrix it had)
static bool orthonormalise(int n, int p, Mat& W, Mat& Q, const Mat& norm2, Mat& B, Mat& G_out) {
    Mat R1((size_t)p * p), R2((size_t)p * p), U((size_t)p * p);
    G_out = gram(n, p, W, Q);
    if (!bsm::eig_chol_rank(p, G_out.data(), norm2.data(), R1.data(), U.data())) return false;
    times(n, p, W, U);
    times(n, p, Q, U);
    const Mat G2 = gram(n, p, W, Q);
    if (!bsm::eig_chol_rank(p, G2.data(), nullptr, R2.data(), U.data())) return false;
    times(n, p, W, U);
    times(n, p, Q, U);
    B.assign((size_t)p * p, 0.0);
    bsm::eig_mul_upper(p, R2.data(), R1.data(), B.data());
    return true;
}

struct Run {
    std::vector<double> lam;
    Mat Y;  // n x nev, the Ritz vectors Y = V Z
    int steps = 0, m = 0, converged = 0, products = 0;
    bool exhausted = false, not_pd = false;
    double orth = 0.0;  // max |V^T M V - I|
};

// the loop of eigsh_gen_t, with a dense n x n operator for A^-1 and a dense M
static Run lanczos(int n, const Mat& Ainv, const Mat& M, int nev, int p, int ncv, double tol, uint64_t seed) {
    Run out;
    bsm::EigLoop loop;
    loop.init(p, nev, ncv, tol);
    std::vector<Mat> V;
    Mat W((size_t)n * p), Q, B, G;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < p; ++c) W[(size_t)r * p + c] = bsm::eig_start_value(seed, (uint64_t)r, (uint64_t)c);
    Q = apply(n, p, M, W);
    ++out.products;
    Mat norm2 = diag_of(p, gram(n, p, W, Q));
    if (!bsm::eig_mass_pd(p, norm2.data())) {
        out.not_pd = true;
        return out;
    }
    if (!orthonormalise(n, p, W, Q, norm2, B, G)) {
        out.exhausted = true;
        return out;
    }
    V.push_back(W);  // Q = M V_0
    for (;;) {
        W = apply(n, p, Ainv, Q);  // A^-1 (M V_j)
        Q = apply(n, p, M, W);
        ++out.products;
        norm2 = diag_of(p, gram(n, p, W, Q));
        if (!bsm::eig_mass_pd(p, norm2.data())) {
            out.not_pd = true;
            return out;
        }
        Mat a_raw((size_t)p * p, 0.0);
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<Mat> C;
            for (const Mat& Vb : V) C.push_back(gram(n, p, Vb, Q));
            for (size_t b = 0; b < V.size(); ++b)
                for (int r = 0; r < n; ++r)
                    for (int c = 0; c < p; ++c)
                        for (int d = 0; d < p; ++d)
                            W[(size_t)r * p + d] -= V[b][(size_t)r * p + c] * C[b][(size_t)c * p + d];
            for (int i = 0; i < p * p; ++i) a_raw[(size_t)i] += C.back()[(size_t)i];
            Q = apply(n, p, M, W);
            ++out.products;
        }
        const bool full = orthonormalise(n, p, W, Q, norm2, B, G);
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
    const int got = std::min(nev, loop.m());
    std::vector<int> order((size_t)got);
    for (int i = 0; i < got; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return loop.theta_of(x) > loop.theta_of(y); });
    out.Y.assign((size_t)n * nev, 0.0);
    for (int i = 0; i < got; ++i) {
        out.lam.push_back(1.0 / loop.theta_of(order[(size_t)i]));
        for (int b = 0; b < loop.steps; ++b)
            for (int c = 0; c < p; ++c) {
                const double z = loop.s_of(order[(size_t)i], b * p + c);
                for (int r = 0; r < n; ++r) out.Y[(size_t)r * nev + i] += V[(size_t)b][(size_t)r * p + c] * z;
            }
    }
    out.steps = loop.steps;
    out.m = loop.m();
    out.converged = loop.converged();
    for (size_t a = 0; a < V.size(); ++a) {
        const Mat MV = apply(n, p, M, V[a]);
        for (size_t b = 0; b < V.size(); ++b) {
            const Mat g = gram(n, p, V[b], MV);
            for (int c = 0; c < p; ++c)
                for (int d = 0; d < p; ++d)
                    out.orth = std::max(out.orth, std::fabs(g[(size_t)c * p + d] - (a == b && c == d ? 1.0 : 0.0)));
        }
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

// the eigenvalues of A y = lambda M y, ascending: Jacobi on L^-1 A L^-T, M = L L^T
static std::vector<double> reference(int n, const Mat& A, const Mat& M) {
    Mat L((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        double d = M[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        L[(size_t)j * n + j] = std::sqrt(d);
        for (int i = j + 1; i < n; ++i) {
            double v = M[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) v -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = v / L[(size_t)j * n + j];
        }
    }
    // X = L^-1 A (forward substitution on the columns), then C = X L^-T = (L^-1 X^T)^T
    auto forward = [&](const Mat& Bm) {
        Mat X((size_t)n * n, 0.0);
        for (int c = 0; c < n; ++c)
            for (int i = 0; i < n; ++i) {
                double v = Bm[(size_t)i * n + c];
                for (int k = 0; k < i; ++k) v -= L[(size_t)i * n + k] * X[(size_t)k * n + c];
                X[(size_t)i * n + c] = v / L[(size_t)i * n + i];
            }
        return X;
    };
    const Mat X = forward(A);
    Mat Xt((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Xt[(size_t)i * n + j] = X[(size_t)j * n + i];
    Mat C = forward(Xt);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) C[(size_t)i * n + j] = C[(size_t)j * n + i] = 0.5 * (C[(size_t)i * n + j] + C[(size_t)j * n + i]);
    std::vector<double> w, z;
    bsm::eig_sym_solve(n, C, w, z);
    return w;
}

int main() {
    {  // the positive-definiteness rule
        const double good[3] = {1.0, 0x1p-1000, 3.0}, zero[3] = {0.0, 0.0, 0.0}, neg[3] = {1.0, -1e-300, 1.0};
        const double nan[2] = {1.0, std::numeric_limits<double>::quiet_NaN()};
        const double inf[1] = {std::numeric_limits<double>::infinity()};
        CHECK(bsm::eig_mass_pd(3, good));
        CHECK(!bsm::eig_mass_pd(3, zero));  // a zero block
        CHECK(!bsm::eig_mass_pd(3, neg));
        CHECK(!bsm::eig_mass_pd(2, nan));
        CHECK(!bsm::eig_mass_pd(1, inf));
    }
    const int g = 9, n = g * g;
    Mat a((size_t)n * n, 0.0), m((size_t)n * n, 0.0);
    for (int i = 0; i < g; ++i)
        for (int j = 0; j < g; ++j) {
            const int r = i * g + j;
            a[(size_t)r * n + r] = 4.0;
            if (i > 0) a[(size_t)r * n + r - g] = -1.0;
            if (i + 1 < g) a[(size_t)r * n + r + g] = -1.0;
            if (j > 0) a[(size_t)r * n + r - 1] = -1.0;
            if (j + 1 < g) a[(size_t)r * n + r + 1] = -1.0;
            for (int di = -1; di <= 1; ++di)
                for (int dj = -1; dj <= 1; ++dj) {
                    const int i2 = i + di, j2 = j + dj;
                    if (i2 < 0 || i2 >= g || j2 < 0 || j2 >= g) continue;
                    m[(size_t)r * n + i2 * g + j2] = (di == 0 ? 4.0 : 1.0) * (dj == 0 ? 4.0 : 1.0) / 36.0;
                }
        }
    const Mat ainv = inverse(n, a);
    const int nev = 6;
    {  // the whole generalised loop
        const std::vector<double> ref = reference(n, a, m);
        CHECK(std::fabs(ref[1] - ref[2]) < 1e-12 && std::fabs(ref[4] - ref[5]) < 1e-12);  // the double ones
        CHECK(ref[3] - ref[2] > 1e-2 && ref[1] - ref[0] > 1e-2);
        const Run b4 = lanczos(n, ainv, m, nev, 4, 80, 0x1p-26, 0);
        std::printf("block 4: %d steps, %d columns, %d converged, M-orthogonality of the basis %.3e, %d products with M\n",
                    b4.steps, b4.m, b4.converged, b4.orth, b4.products);
        CHECK(!b4.not_pd && !b4.exhausted);
        CHECK((int)b4.lam.size() == nev && b4.converged == nev);
        CHECK(b4.orth <= 1e-13);
        CHECK(b4.products == 3 * b4.steps + 1);  // three products with M per step and one for the start block
        for (int i = 0; i < nev && i < (int)b4.lam.size(); ++i) {
            std::printf("  lambda %d: %.16f, reference %.16f\n", i, b4.lam[(size_t)i], ref[(size_t)i]);
            CHECK(std::fabs(b4.lam[(size_t)i] - ref[(size_t)i]) <= 1e-11);  // tol^2 kappa, far above rounding
        }
        // the Ritz vectors are M-orthonormal
        const Mat MY = apply(n, nev, m, b4.Y);
        const Mat yy = gram(n, nev, b4.Y, MY);
        double worst = 0.0;
        for (int c = 0; c < nev; ++c)
            for (int d = 0; d < nev; ++d) worst = std::max(worst, std::fabs(yy[(size_t)c * nev + d] - (c == d ? 1.0 : 0.0)));
        std::printf("  max |Y^T M Y - I| %.3e\n", worst);
        CHECK(worst <= 1e-12);
        // and eigenvectors: A y - lambda M y is small
        const Mat AY = apply(n, nev, a, b4.Y);
        double res = 0.0;
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < nev; ++c)
                res = std::max(res, std::fabs(AY[(size_t)r * nev + c] - b4.lam[(size_t)c] * MY[(size_t)r * nev + c]));
        std::printf("  max |A y - lambda M y| %.3e\n", res);
        // tol ||A||inf sqrt(mu_max / mu_min) ||y||2 with ||A||inf = 8, the root below 3 and ||y||2 <= mu_min^-1/2 < 3.2
        CHECK(res <= 2 * 0x1p-26 * 8.0 * 3.0 * 3.2);
    }
    {  // M = -I: the rule fires on the start block, before any solve
        Mat minus((size_t)n * n, 0.0);
        for (int i = 0; i < n; ++i) minus[(size_t)i * n + i] = -1.0;
        const Run r = lanczos(n, ainv, minus, nev, 4, 80, 0x1p-26, 0);
        CHECK(r.not_pd && r.steps == 0 && r.products == 1 && r.lam.empty());
        const Mat none((size_t)n * n, 0.0);  // no mass at all: a zero block
        const Run z = lanczos(n, ainv, none, nev, 4, 80, 0x1p-26, 0);
        CHECK(z.not_pd && z.steps == 0 && z.lam.empty());
    }
    std::printf("summary: %d failed, %d checks\n", g_fail, g_checks);
    return g_fail ? 1 : 0;
}
