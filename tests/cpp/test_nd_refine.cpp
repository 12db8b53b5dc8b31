// bsm::cholesky_nd_as<float> of a Csr<double> and NdFactor::solve_refined
// (include/bsm.hpp) on a 2-D Poisson system: an f32 factor, half the f64
// factor's bytes, refined to f64 backward error. Prints x ("x <column> <row>
// <hexfloat>") and the per-column info ("info <column> <iters> <berr>") for
// tests/test_cpp_nd_refine.py, which compares them with Python's.
//   (no argument)        the GPU run
//   --expect-no-device   the factorisation must throw bsm::DeviceError
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nd_test.hpp"

using bsm::Csr;
using bsm::Dense;

static void run_gpu() {
    const uint64_t g = 11, n = g * g;
    const auto a = poisson(g);
    const bsm::NdFactor<float> f = bsm::cholesky_nd_as<float>(a);
    const bsm::NdFactor<double> f64(a);
    CHECK(f.rows() == n);
    CHECK(2 * f.nbytes() == f64.nbytes());
    std::vector<std::vector<double>> cols(2, std::vector<double>(n));
    for (uint64_t i = 0; i < n; ++i) {
        cols[0][i] = 1.0 + (double)(i % 7) * 0.125;
        cols[1][i] = (double)((i * 37) % 11) - 5.0;
    }
    const auto b = Dense<double>::from_data(cols);
    const auto r = f.solve_refined(a, b);
    CHECK(r.iters.size() == 2 && r.berr.size() == 2 && r.converged.size() == 2);
    CHECK(r.tol == 7 * 0x1p-53);  // the longest row of the 5-point stencil is 5
    for (size_t j = 0; j < 2; ++j) {
        CHECK(r.converged[j] && r.iters[j] >= 1 && r.iters[j] <= 3 && r.berr[j] <= r.tol);
        std::printf("info %zu %u %a\n", j, r.iters[j], r.berr[j]);
        for (uint64_t i = 0; i < n; ++i) std::printf("x %zu %llu %a\n", j, (unsigned long long)i, r.x.get_col(j)[i]);
    }
    // against the f64 factor's plain solve
    const auto x64 = f64.solve(b);
    double worst = 0.0, scale = 0.0;
    for (size_t j = 0; j < 2; ++j)
        for (uint64_t i = 0; i < n; ++i) {
            worst = std::fmax(worst, std::fabs(r.x.get_col(j)[i] - x64.get_col(j)[i]));
            scale = std::fmax(scale, std::fabs(x64.get_col(j)[i]));
        }
    CHECK(worst <= 1e-10 * scale);
    // no correction: the f32 factor's own accuracy, reported and not converged
    const auto r0 = f.solve_refined(a, b, 0);
    CHECK(r0.iters[0] == 0 && !r0.converged[0] && r0.berr[0] > r.berr[0]);
    bool refused = false;
    try {
        (void)f.solve_refined(a, b, 5, -1.0);
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    CHECK(refused);
    refused = false;
    try {
        (void)f.solve_refined(poisson(4), b);
    } catch (const bsm::Panic&) {
        refused = true;
    }
    CHECK(refused);
}

static void touch_device() {
    const auto f = bsm::cholesky_nd_as<float>(poisson(4));
    (void)f.rows();
}

int main(int argc, char** argv) {
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "cholesky_nd_as (DeviceError without a GPU: no CPU fallback)");
}
