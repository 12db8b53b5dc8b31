// The scalar rule of the rank-k update and downdate of a kept factor
// (csrc/updown_rule.hpp) as a stand-alone CPU program, over the dense L of
// the 9 x 9 grid's Poisson matrix: L L^T after an update and after a
// downdate against the dense matrix, a downdate that reports "not positive
// definite" at a named pivot, w_j == 0 leaving column j's bits, and a rank-3
// call in column order. Built with -fsanitize=address,undefined by
// tests/test_updown_rule.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "updown_rule.hpp"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) {                                                               \
            ++g_fail;                                                                \
            std::fprintf(stderr, "  CHECK failed: %s (line %d)\n", #cond, __LINE__); \
        }                                                                            \
    } while (0)

constexpr int G = 9, N = G * G;

template <typename T>
using Mat = std::vector<T>;  // N x N, row-major

// the 5-point Laplacian of the G x G grid plus the identity (SPD)
static Mat<double> poisson() {
    Mat<double> a((size_t)N * N, 0.0);
    for (int y = 0; y < G; ++y)
        for (int x = 0; x < G; ++x) {
            const int i = y * G + x;
            a[(size_t)i * N + i] = 5.0;
            if (x > 0) a[(size_t)i * N + i - 1] = -1.0;
            if (x + 1 < G) a[(size_t)i * N + i + 1] = -1.0;
            if (y > 0) a[(size_t)i * N + i - G] = -1.0;
            if (y + 1 < G) a[(size_t)i * N + i + G] = -1.0;
        }
    return a;
}

template <typename T>
static Mat<T> cholesky(const Mat<double>& a) {
    Mat<T> l((size_t)N * N, (T)0);
    for (int j = 0; j < N; ++j) {
        T d = (T)a[(size_t)j * N + j];
        for (int t = 0; t < j; ++t) d -= l[(size_t)j * N + t] * l[(size_t)j * N + t];
        d = std::sqrt(d);
        l[(size_t)j * N + j] = d;
        for (int i = j + 1; i < N; ++i) {
            T v = (T)a[(size_t)i * N + j];
            for (int t = 0; t < j; ++t) v -= l[(size_t)i * N + t] * l[(size_t)j * N + t];
            l[(size_t)i * N + j] = v / d;
        }
    }
    return l;
}

// The sweep as the kernels run it: at each pivot the k columns in column
// order. w: k columns of N, overwritten. Returns -1, or the first failing
// pivot * 16 + column (L is then partly rewritten: a caller that must not
// write runs it on a copy first, as the dry pass does).
template <typename T>
static int sweep(Mat<T>& l, std::vector<std::vector<T>>& w, int sign) {
    for (int j = 0; j < N; ++j)
        for (size_t c = 0; c < w.size(); ++c) {
            bsm::UpdownCoef<T> cs;
            if (!bsm::updown_pivot(l[(size_t)j * N + j], w[c][(size_t)j], sign, cs)) return j * 16 + (int)c;
            for (int i = j + 1; i < N; ++i) bsm::updown_row(l[(size_t)i * N + j], w[c][(size_t)i], sign, cs);
        }
    return -1;
}

// max |L L^T - A| / max |A|
template <typename T>
static double residual(const Mat<T>& l, const Mat<double>& a) {
    double err = 0.0, scale = 0.0;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int t = 0; t <= j; ++t) s += (double)l[(size_t)i * N + t] * (double)l[(size_t)j * N + t];
            err = std::fmax(err, std::fabs(s - a[(size_t)i * N + j]));
            scale = std::fmax(scale, std::fabs(a[(size_t)i * N + j]));
        }
    return err / scale;
}

static void add_outer(Mat<double>& a, const std::vector<double>& w, double sign) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) a[(size_t)i * N + j] += sign * w[(size_t)i] * w[(size_t)j];
}

template <typename T>
static std::vector<T> rounded(const std::vector<double>& w) {
    return std::vector<T>(w.begin(), w.end());
}
template <typename T>
static std::vector<double> widened(const std::vector<T>& w) {
    return std::vector<double>(w.begin(), w.end());
}

template <typename T>
static void run(const char* name) {
    const double eps = std::numeric_limits<T>::epsilon();
    // A backward stable factor has |L L^T - A| <= (N + 1) eps |L| |L|^T
    // entrywise, and |L| |L|^T <= max A_ii here; the sweep adds at most that
    // again per column. 4 (N + 2) eps bounds a factor, an update and a downdate.
    const double tol = 4.0 * (N + 2) * eps;
    const Mat<double> a = poisson();
    const Mat<T> l0 = cholesky<T>(a);
    CHECK(residual(l0, a) <= tol);
    // an edge of the grid, sqrt(c) (e_i - e_j), as T holds it
    std::vector<double> edge((size_t)N, 0.0);
    edge[30] = std::sqrt(0.75);
    edge[31] = -std::sqrt(0.75);
    const std::vector<double> edge_t = widened(rounded<T>(edge));
    {  // update, then the downdate that takes it back
        Mat<T> l = l0;
        std::vector<std::vector<T>> w{rounded<T>(edge)};
        CHECK(sweep(l, w, +1) == -1);
        Mat<double> a2 = a;
        add_outer(a2, edge_t, +1.0);
        const double up = residual(l, a2);
        CHECK(up <= tol);
        CHECK(residual(l, a) > 100 * tol);  // it did change the factor
        // w_j == 0 for j < 30: those columns keep their bits
        for (int j = 0; j < 30; ++j)
            for (int i = j; i < N; ++i)
                CHECK(std::memcmp(&l[(size_t)i * N + j], &l0[(size_t)i * N + j], sizeof(T)) == 0);
        w = {rounded<T>(edge)};
        CHECK(sweep(l, w, -1) == -1);
        const double down = residual(l, a);
        CHECK(down <= tol);
        std::printf("%s: update %.3e, update + downdate %.3e (tol %.3e)\n", name, up, down, tol);
    }
    {  // a downdate alone
        Mat<T> l = l0;
        std::vector<std::vector<T>> w{rounded<T>(edge)};
        CHECK(sweep(l, w, -1) == -1);
        Mat<double> a2 = a;
        add_outer(a2, edge_t, -1.0);
        CHECK(residual(l, a2) <= tol);
    }
    {  // not positive definite, at pivot 40 and nowhere before: w = 2 sqrt(A_ii) e_i
        Mat<T> l = l0;
        std::vector<double> wd((size_t)N, 0.0);
        wd[40] = 2.0 * std::sqrt(a[(size_t)40 * N + 40]);
        std::vector<std::vector<T>> w{rounded<T>(wd)};
        CHECK(sweep(l, w, -1) == 40 * 16 + 0);
        CHECK(std::memcmp(l.data(), l0.data(), l.size() * sizeof(T)) == 0);  // pivots 0 .. 39 were skipped whole
        // the same column as an update is fine
        w = {rounded<T>(wd)};
        CHECK(sweep(l, w, +1) == -1);
        // the test itself: r^2 <= 0, NaN and infinity fail, a tiny positive passes
        CHECK(bsm::updown_not_pd((T)0) && bsm::updown_not_pd((T)-1) &&
              bsm::updown_not_pd(std::numeric_limits<T>::quiet_NaN()) &&
              bsm::updown_not_pd(std::numeric_limits<T>::infinity()) &&
              !bsm::updown_not_pd(std::numeric_limits<T>::min()));
        T d = (T)2;
        bsm::UpdownCoef<T> cs;
        CHECK(!bsm::updown_pivot(d, (T)2, -1, cs) && d == (T)2 && cs.c == (T)1 && cs.s == (T)0);  // r^2 == 0
        CHECK(!bsm::updown_pivot(d, std::numeric_limits<T>::infinity(), +1, cs) && d == (T)2);
    }
    {  // a skipped pivot reads and rounds nothing: NaN in L and w comes through as it is
        T l = std::numeric_limits<T>::quiet_NaN(), wi = (T)3, d = (T)7;
        bsm::UpdownCoef<T> cs;
        CHECK(bsm::updown_pivot(d, (T)0, -1, cs) && d == (T)7 && cs.s == (T)0);
        bsm::updown_row(l, wi, -1, cs);
        CHECK(std::isnan(l) && wi == (T)3);
    }
    {  // rank 3, the columns in column order at each pivot: L L^T, and the bits of three calls of one column
        std::vector<std::vector<double>> cols(3, std::vector<double>((size_t)N, 0.0));
        cols[0][12] = 0.5, cols[0][13] = -0.5, cols[0][21] = 0.25;  // overlapping supports
        cols[1][13] = 1.5;
        cols[2][5] = 0.3, cols[2][13] = 0.7, cols[2][80] = -0.2;
        Mat<T> l = l0;
        std::vector<std::vector<T>> w;
        Mat<double> a2 = a;
        for (const auto& c : cols) {
            w.push_back(rounded<T>(c));
            add_outer(a2, widened(w.back()), +1.0);
        }
        CHECK(sweep(l, w, +1) == -1);
        CHECK(residual(l, a2) <= 3 * tol);
        Mat<T> ls = l0;
        for (const auto& c : cols) {
            std::vector<std::vector<T>> w1{rounded<T>(c)};
            CHECK(sweep(ls, w1, +1) == -1);
        }
        CHECK(std::memcmp(l.data(), ls.data(), l.size() * sizeof(T)) == 0);
        // column order matters to the bits: the reverse order is another rounding
        Mat<T> lr = l0;
        std::vector<std::vector<T>> wrv{rounded<T>(cols[2]), rounded<T>(cols[1]), rounded<T>(cols[0])};
        CHECK(sweep(lr, wrv, +1) == -1);
        CHECK(residual(lr, a2) <= 3 * tol);
        // and the three come out again
        w.clear();
        for (const auto& c : cols) w.push_back(rounded<T>(c));
        CHECK(sweep(l, w, -1) == -1);
        CHECK(residual(l, a) <= 4 * tol);
    }
}

int main() {
    run<double>("f64");
    run<float>("f32");
    std::printf("summary: %d failed, %d checks\n", g_fail, g_checks);
    return g_fail ? 1 : 0;
}
