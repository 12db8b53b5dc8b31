// bsm::cholesky_nd_schur / NdFactor<T>::schur, schur_condense, schur_expand,
// schur_index (include/bsm.hpp) on a 2-D Poisson system with a grid line as
// the set: the index comes back as given and perm() ends in it; S is
// symmetric, repeats, and S x_G = g holds for the solve's x (so S and g are
// the Schur complement and its right-hand side); expand returns the solve bit
// for bit; a factor without a set, another pattern and a bad set are refused.
//   (no argument)        the GPU run
//   --expect-no-device   the constructor must throw bsm::DeviceError
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "nd_test.hpp"

using bsm::Dense;

template <class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const std::exception&) {
        return true;
    }
    return false;
}

static void run_gpu() {
    const uint64_t g = 11, n = g * g, m = g;
    const auto a = poisson(g);
    std::vector<uint64_t> idx(m);
    for (uint64_t i = 0; i < m; ++i) idx[i] = 5 * g + (m - 1 - i);  // the middle line, descending
    const auto f = bsm::cholesky_nd_schur<double>(a, idx);
    CHECK(f.schur_index() == idx);
    const auto perm = f.perm();
    for (uint64_t i = 0; i < m; ++i) CHECK((uint64_t)perm[n - m + i] == 5 * g + i);
    const auto S = f.schur(a);
    CHECK(S.size() == m * m);
    CHECK(S == f.schur(a));
    for (uint64_t i = 0; i < m; ++i)
        for (uint64_t j = 0; j < m; ++j) CHECK(S[i + j * m] == S[j + i * m]);
    std::vector<std::vector<double>> cols(2, std::vector<double>(n));
    for (uint64_t i = 0; i < n; ++i) {
        cols[0][i] = 1.0 + 0.01 * (double)i;
        cols[1][i] = std::sin((double)i);
    }
    const auto b = Dense<double>::from_data(cols);
    const auto x = f.solve(b);
    const auto gd = f.schur_condense(b);
    CHECK(gd.get_dims().rows == m && gd.get_dims().cols == 2);
    // S x_G = g to rounding: |S x_G - g| <= 1e-12 (|S| |x_G| + |g|) (m = 11 terms of f64)
    std::vector<std::vector<double>> xg(2, std::vector<double>(m));
    for (size_t c = 0; c < 2; ++c) {
        for (uint64_t i = 0; i < m; ++i) xg[c][i] = x.get_col(c)[idx[i]];
        for (uint64_t i = 0; i < m; ++i) {
            double s = 0.0, mag = std::fabs(gd.get_col(c)[i]);
            for (uint64_t j = 0; j < m; ++j) {
                s += S[i + j * m] * xg[c][j];
                mag += std::fabs(S[i + j * m] * xg[c][j]);
            }
            CHECK(std::fabs(s - gd.get_col(c)[i]) <= 1e-12 * mag);
        }
    }
    const auto xe = f.schur_expand(b, Dense<double>::from_data(xg));
    for (size_t c = 0; c < 2; ++c)
        for (uint64_t i = 0; i < n; ++i) CHECK(xe.get_col(c)[i] == x.get_col(c)[i]);
    // refusals
    bsm::NdFactor<double> plain(a);
    CHECK(plain.schur_index().empty());
    CHECK(throws([&] { plain.schur(a); }));
    CHECK(throws([&] { plain.schur_condense(b); }));
    CHECK(throws([&] { plain.schur_expand(b, Dense<double>::from_data(xg)); }));
    CHECK(throws([&] { f.schur(poisson(10)); }));
    CHECK(throws([&] { bsm::cholesky_nd_schur<double>(a, {1, n}); }));
    CHECK(throws([&] { bsm::cholesky_nd_schur<double>(a, {1, 2, 1}); }));
}

static void touch_device() { bsm::cholesky_nd_schur<double>(poisson(4), {1, 2}); }

int main(int argc, char** argv) {
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "NdFactor schur (DeviceError without a GPU: no CPU fallback)");
}
