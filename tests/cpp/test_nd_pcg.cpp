// bsm::NdFactor::solve_pcg (include/bsm.hpp) on a 2-D Poisson system: the f32
// factor of A as the preconditioner of conjugate gradients on A / 2, which
// iterative refinement cannot solve. Prints x ("x <column> <row> <hexfloat>")
// and the per-column info ("info <column> <iters> <berr> <breakdown>") for
// tests/test_cpp_nd_pcg.py, which compares them with Python's.
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
    const auto a = poisson(g), half = poisson(g, 0.5), neg = poisson(g, -1.0);
    const bsm::NdFactor<float> f = bsm::cholesky_nd_as<float>(a);
    const bsm::NdFactor<double> f_half(half);
    std::vector<std::vector<double>> cols(2, std::vector<double>(n));
    for (uint64_t i = 0; i < n; ++i) {
        cols[0][i] = 1.0 + (double)(i % 7) * 0.125;
        cols[1][i] = (double)((i * 37) % 11) - 5.0;
    }
    const auto b = Dense<double>::from_data(cols);
    const auto r = f.solve_pcg(half, b);
    CHECK(r.iters.size() == 2 && r.berr.size() == 2 && r.converged.size() == 2 && r.breakdown.size() == 2);
    CHECK(r.tol == 7 * 0x1p-53);  // the longest row of the 5-point stencil is 5
    for (size_t j = 0; j < 2; ++j) {
        CHECK(r.converged[j] && !r.breakdown[j] && r.iters[j] >= 1 && r.iters[j] <= 30 && r.berr[j] <= r.tol);
        std::printf("info %zu %u %a %d\n", j, r.iters[j], r.berr[j], (int)r.breakdown[j]);
        for (uint64_t i = 0; i < n; ++i) std::printf("x %zu %llu %a\n", j, (unsigned long long)i, r.x.get_col(j)[i]);
    }
    // against the plain solve by the f64 factor of A / 2 itself
    const auto x64 = f_half.solve(b);
    double worst = 0.0, scale = 0.0;
    for (size_t j = 0; j < 2; ++j)
        for (uint64_t i = 0; i < n; ++i) {
            worst = std::fmax(worst, std::fabs(r.x.get_col(j)[i] - x64.get_col(j)[i]));
            scale = std::fmax(scale, std::fabs(x64.get_col(j)[i]));
        }
    CHECK(worst <= 1e-10 * scale);
    // refinement on the same system reports failure: why the call exists
    const auto refined = f.solve_refined(half, b, 30);
    CHECK(!refined.converged[0] && !refined.converged[1]);
    // no step: the refined solve's first iterate
    const auto r0 = f.solve_pcg(half, b, 0);
    const auto q0 = f.solve_refined(half, b, 0);
    CHECK(r0.iters[0] == 0 && !r0.converged[0] && r0.berr[0] == q0.berr[0] && r0.berr[1] == q0.berr[1]);
    for (uint64_t i = 0; i < n; ++i) CHECK(r0.x.get_col(1)[i] == q0.x.get_col(1)[i]);
    // a negative definite system breaks down, and says so
    const auto rn = f.solve_pcg(neg, b);
    CHECK(rn.breakdown[0] && rn.breakdown[1] && !rn.converged[0] && rn.iters[0] <= 1);
    bool refused = false;
    try {
        (void)f.solve_pcg(a, b, 50, -1.0);
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    CHECK(refused);
    refused = false;
    try {
        (void)f.solve_pcg(poisson(4), b);
    } catch (const bsm::Panic&) {
        refused = true;
    }
    CHECK(refused);
}

static void touch_device() {
    const auto f = bsm::cholesky_nd_as<float>(poisson(4));
    const auto b = Dense<double>::from_data({std::vector<double>(16, 1.0)});
    (void)f.solve_pcg(poisson(4), b);
}

int main(int argc, char** argv) {
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "solve_pcg (DeviceError without a GPU: no CPU fallback)");
}
