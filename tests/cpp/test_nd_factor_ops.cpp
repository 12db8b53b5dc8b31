// bsm::NdFactor<double> (include/bsm.hpp) on a 2-D Poisson system: refactor
// against a fresh factor bit for bit, logdet against the host sum over l(),
// and NdSystem::L then NdSystem::Lt around the permutation against solve.
// Driven by tests/test_cpp_nd_factor_ops.py.
//   (no argument)        the GPU run
//   --expect-no-device   the constructor must throw bsm::DeviceError
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nd_test.hpp"

using bsm::Csr;
using bsm::Dense;
using bsm::NdSystem;

// scale 1: the Poisson matrix A; otherwise D A D with d_i = 1 + (i % 7) / 8 (SPD with A)
static Csr<double> poisson(uint64_t g, bool scaled) {
    Grid a(g);
    if (scaled)
        for (uint64_t i = 0; i < a.n; ++i)
            for (uint64_t e = a.rp[i]; e < a.rp[i + 1]; ++e)
                a.v[e] *= (1.0 + (double)(i % 7) / 8.0) * (1.0 + (double)(a.ci[e] % 7) / 8.0);
    return a.csr();
}

static bool same_cols(const Dense<double>& x, const Dense<double>& y, uint64_t k, uint64_t n) {
    for (uint64_t j = 0; j < k; ++j)
        if (std::memcmp(x.get_col(j).data(), y.get_col(j).data(), n * sizeof(double)) != 0) return false;
    return true;
}

static void run_gpu() {
    const uint64_t g = 11, n = g * g, k = 2;
    const auto a = poisson(g, false), a2 = poisson(g, true);
    std::vector<double> b(n * k);
    orc_gen_x_colmajor(3001, n, k, 0, b.data());
    const auto rhs = Dense<double>::from_data(
        {std::vector<double>(b.begin(), b.begin() + n), std::vector<double>(b.begin() + n, b.end())});
    bsm::NdFactor<double> f(a);
    const bsm::NdFactor<double> fresh(a2);
    const auto x_a = f.solve(rhs);
    const uint64_t nbytes = f.nbytes();

    // refactor: the bits of a fresh factor, and back
    f.refactor(a2);
    CHECK(same_cols(f.solve(rhs), fresh.solve(rhs), k, n));
    CHECK(!same_cols(f.solve(rhs), x_a, k, n));
    CHECK(f.l() == fresh.l());
    CHECK(f.l_star() == fresh.l_star());
    CHECK(f.perm() == fresh.perm());
    CHECK(f.nbytes() == nbytes);
    CHECK(f.logdet() == fresh.logdet());
    f.refactor(a);
    CHECK(same_cols(f.solve(rhs), x_a, k, n));
    bool refused = false;
    try {
        f.refactor(poisson(g - 1, false));
    } catch (const std::exception&) {
        refused = true;
    }
    CHECK(refused);
    CHECK(same_cols(f.solve(rhs), x_a, k, n));

    // logdet against the host sum over l(): the same numbers, another order
    const auto l = f.l();
    double host = 0.0;
    for (uint64_t i = 0; i < n; ++i) host += std::log(l.v()[l.row_index()[i + 1] - 1]);  // the diagonal is last
    host *= 2.0;
    const double ld = f.logdet();
    CHECK(std::fabs(ld - host) <= 1e-12 * std::fabs(host));
    CHECK(ld == f.logdet());

    // L then L^T around the permutation is the solve, bit for bit
    const auto p = f.perm();
    std::vector<std::vector<double>> pb(k, std::vector<double>(n));
    for (uint64_t j = 0; j < k; ++j)
        for (uint64_t q = 0; q < n; ++q) pb[j][q] = b[j * n + (uint64_t)p[q]];
    const auto y = f.solve(Dense<double>::from_data(pb), NdSystem::L);
    const auto xp = f.solve(y, NdSystem::Lt);
    CHECK(same_cols(f.solve(rhs, NdSystem::A), x_a, k, n));
    for (uint64_t j = 0; j < k; ++j) {
        bool same = true;
        for (uint64_t q = 0; q < n; ++q)
            same = same && std::memcmp(&xp.get_col(j)[q], &x_a.get_col(j)[(uint64_t)p[q]], sizeof(double)) == 0;
        CHECK(same);
    }
    // y against the reference-order forward substitution on the exported L
    const auto yref = bsm::forward_substitution(l, Dense<double>::from_data(pb));
    for (uint64_t j = 0; j < k; ++j) {
        double num = 0, den = 0;
        for (uint64_t q = 0; q < n; ++q) {
            const double e = y.get_col(j)[q] - yref.get_col(j)[q];
            num += e * e;
            den += yref.get_col(j)[q] * yref.get_col(j)[q];
        }
        CHECK(num <= 1e-20 * den);  // 1e-10 relative, the project's f64 bar
    }
}

static void touch_device() {
    bsm::NdFactor<double> f(poisson(4, false));
    f.refactor(poisson(4, true));
    (void)f.logdet();
}

int main(int argc, char** argv) {
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "NdFactor (DeviceError without a GPU: no CPU fallback)");
}
