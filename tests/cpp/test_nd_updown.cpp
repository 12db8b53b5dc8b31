// bsm::NdFactor<T>::update / downdate (include/bsm.hpp) on a 2-D Poisson
// system: a rank-2 update (a diagonal column and a stored edge) changes logdet
// by log det(I + W^T S^-1 W) from the factor's own solves, its downdate
// brings the solves back, a downdate that is not positive definite and a w of
// another dtype or row count are refused with the factor untouched. Prints
// logdet after the update ("logdet <hexfloat>") for
// tests/test_cpp_nd_updown.py, which compares it with Python's.
//   (no argument)        the GPU run
//   --expect-no-device   the constructor must throw bsm::DeviceError
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "nd_test.hpp"

using bsm::Csr;
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
    const uint64_t g = 11, n = g * g;
    const auto a = poisson(g);
    bsm::NdFactor<double> f(a);
    const auto perm = f.perm();
    // column 0: 0.5 e_v, v the first vertex of the new order; column 1: the edge
    // from the second vertex u to a neighbour that comes later in the new order
    std::vector<uint64_t> pinv(n);
    for (uint64_t q = 0; q < n; ++q) pinv[(size_t)perm[q]] = q;
    const uint64_t v0 = (uint64_t)perm[0];
    uint64_t u = n, t = n;
    for (uint64_t q = 1; q < n && t == n; ++q) {
        u = (uint64_t)perm[q];
        for (uint64_t e = a.row_index()[u]; e < a.row_index()[u + 1]; ++e)
            if (a.col_index()[e] != u && pinv[a.col_index()[e]] > q) t = a.col_index()[e];
    }
    CHECK(t < n);
    std::vector<std::vector<double>> wd(n, std::vector<double>(2, 0.0));
    wd[v0][0] = 0.5;
    wd[u][1] = std::sqrt(0.75);
    wd[t][1] = -std::sqrt(0.75);
    const auto w = Csr<double>::from_data(wd);
    std::vector<std::vector<double>> cols(2, std::vector<double>(n, 0.0));
    for (uint64_t i = 0; i < n; ++i) cols[0][i] = wd[i][0], cols[1][i] = wd[i][1];
    const auto rhs = Dense<double>::from_data(cols);  // a list of columns
    const auto x0 = f.solve(rhs);  // S^-1 W
    double m[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            m[i][j] = i == j ? 1.0 : 0.0;
            for (uint64_t r = 0; r < n; ++r) m[i][j] += cols[i][r] * x0.get_col(j)[r];
        }
    const double ld0 = f.logdet(), want = ld0 + std::log(m[0][0] * m[1][1] - m[0][1] * m[1][0]);
    f.update(w);
    const double ld1 = f.logdet();
    std::printf("logdet %a\n", ld1);
    std::printf("perm0 %lld u %llu t %llu\n", (long long)perm[0], (unsigned long long)u, (unsigned long long)t);
    CHECK(std::fabs(ld1 - want) <= 1e-12 * std::fabs(want));
    const auto x1 = f.solve(rhs);
    CHECK(std::memcmp(x1.get_col(0).data(), x0.get_col(0).data(), n * sizeof(double)) != 0);
    f.downdate(w);
    CHECK(std::fabs(f.logdet() - ld0) <= 1e-12 * std::fabs(ld0));
    const auto x2 = f.solve(rhs);
    double worst = 0.0, scale = 0.0;
    for (uint64_t r = 0; r < n; ++r) {
        worst = std::fmax(worst, std::fabs(x2.get_col(1)[r] - x0.get_col(1)[r]));
        scale = std::fmax(scale, std::fabs(x0.get_col(1)[r]));
    }
    CHECK(worst <= 1e-12 * scale);
    // refusals leave the factor as it is
    const double before = f.logdet();
    std::vector<std::vector<double>> bad(n, std::vector<double>(1, 0.0));
    bad[v0][0] = 4.0;  // 16 > S_vv = 4
    CHECK(throws([&] { f.downdate(Csr<double>::from_data(bad)); }));
    std::vector<std::vector<float>> wf(n, std::vector<float>(1, 0.0f));
    wf[v0][0] = 0.5f;
    CHECK(throws([&] { f.update(Csr<float>::from_data(wf)); }));
    bad.push_back({1.0});
    CHECK(throws([&] { f.update(Csr<double>::from_data(bad)); }));
    const double after = f.logdet();
    CHECK(std::memcmp(&before, &after, sizeof(double)) == 0);
}

static void touch_device() {
    bsm::NdFactor<double> f(poisson(4));
    f.update(Csr<double>::from_data({{1.0}}));
}

int main(int argc, char** argv) {
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "NdFactor (DeviceError without a GPU: no CPU fallback)");
}
