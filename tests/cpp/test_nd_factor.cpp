// bsm::NdFactor<double> (include/bsm.hpp) on a 2-D Poisson system: the kept
// factor's solve against bsm::solve_nd, bit for bit, and its export's
// conventions. Driven by tests/test_cpp_nd_factor.py.
//   (no argument)        the GPU run
//   --expect-no-device   the constructor must throw bsm::DeviceError
#include <cstdio>
#include <cstring>
#include <vector>

#include "nd_test.hpp"

using bsm::Csr;
using bsm::Dense;

static void run_gpu() {
    const uint64_t g = 11, n = g * g, k = 2;
    auto a = poisson(g);
    std::vector<double> b(n * k);
    orc_gen_x_colmajor(3001, n, k, 0, b.data());
    const auto rhs = Dense<double>::from_data(
        {std::vector<double>(b.begin(), b.begin() + n), std::vector<double>(b.begin() + n, b.end())});
    bsm::NdFactor<double> f(a);
    CHECK(f.rows() == n);
    CHECK(f.nbytes() > 0);
    const auto x = f.solve(rhs);
    const auto fused = bsm::solve_nd(a, rhs);
    for (uint64_t j = 0; j < k; ++j)
        CHECK(std::memcmp(x.get_col(j).data(), fused.get_col(j).data(), n * sizeof(double)) == 0);
    // a second solve on the same factor, after solve_nd overwrote the plan's kept fronts
    const auto x2 = f.solve(rhs);
    for (uint64_t j = 0; j < k; ++j)
        CHECK(std::memcmp(x2.get_col(j).data(), fused.get_col(j).data(), n * sizeof(double)) == 0);
    const auto p = f.perm();
    std::vector<char> seen(n, 0);
    for (int64_t o : p) {
        CHECK(o >= 0 && (uint64_t)o < n && !seen[(size_t)o]);
        if (o >= 0 && (uint64_t)o < n) seen[(size_t)o] = 1;
    }
    const auto l = f.l();
    const auto ls = f.l_star();
    CHECK(l.get_dims().rows == n && ls.get_dims().rows == n);
    CHECK(ls == l.transpose());
    for (uint64_t i = 0; i < n; ++i) {
        CHECK(l.col_index()[l.row_index()[i + 1] - 1] == i && l.v()[l.row_index()[i + 1] - 1] > 0);  // diagonal last
        CHECK(ls.col_index()[ls.row_index()[i]] == i);                                              // diagonal first
    }
    // the export feeds the reference-order triangular solves
    std::vector<std::vector<double>> pb(k, std::vector<double>(n));
    for (uint64_t j = 0; j < k; ++j)
        for (uint64_t q = 0; q < n; ++q) pb[j][q] = b[j * n + (uint64_t)p[q]];
    const auto xp = bsm::backward_substitution(ls, bsm::forward_substitution(l, Dense<double>::from_data(pb)));
    for (uint64_t j = 0; j < k; ++j) {
        double num = 0, den = 0;
        for (uint64_t q = 0; q < n; ++q) {
            const double e = xp.get_col(j)[q] - x.get_col(j)[(uint64_t)p[q]];
            num += e * e;
            den += xp.get_col(j)[q] * xp.get_col(j)[q];
        }
        CHECK(num <= 1e-20 * den);  // 1e-10 relative, the project's f64 bar
    }
    bool panicked = false;
    try {
        (void)f.solve(Dense<double>::from_data({std::vector<double>(n - 1, 1.0)}));
    } catch (const bsm::Panic&) {
        panicked = true;
    }
    CHECK(panicked);
}

static void touch_device() {
    bsm::NdFactor<double> f(poisson(4));
}

int main(int argc, char** argv) {
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "NdFactor (DeviceError without a GPU: no CPU fallback)");
}
