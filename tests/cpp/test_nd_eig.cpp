// bsm::NdFactor::eigsh (include/bsm.hpp) on the 11 x 11-grid Poisson matrix:
// the six smallest eigenpairs by block shift-invert Lanczos on the f32 factor,
// against the analytic eigenvalues. Prints lam and resid ("pair <i> <lam>
// <resid>"), the vectors ("y <pair> <row> <hexfloat>") and the info ("info
// <steps> <ncv_used> <converged> <exhausted> <inexact>") for
// tests/test_cpp_nd_eig.py, which compares them with Python's.
//   (no argument)        the GPU run
//   --expect-no-device   the factorisation must throw bsm::DeviceError
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nd_test.hpp"

using bsm::Csr;
using bsm::Dense;

static void run_gpu() {
    const uint64_t g = 11, n = g * g;
    const size_t nev = 6;
    const auto a = poisson(g);
    const bsm::NdFactor<float> f = bsm::cholesky_nd_as<float>(a);
    const auto r = f.eigsh(a, nev, 4, 60);
    CHECK(r.lam.size() == nev && r.resid.size() == nev && r.tol == 0x1p-26);
    CHECK(r.converged == nev && !r.inexact && r.ncv_used <= 60 && r.steps * 4 == r.ncv_used);
    std::vector<double> exact;
    const double pi = 3.14159265358979323846;
    for (uint64_t p = 1; p <= g; ++p)
        for (uint64_t q = 1; q <= g; ++q) exact.push_back(4.0 - 2.0 * std::cos(p * pi / 12) - 2.0 * std::cos(q * pi / 12));
    std::sort(exact.begin(), exact.end());
    std::printf("info %u %u %u %d %d\n", r.steps, r.ncv_used, r.converged, (int)r.exhausted, (int)r.inexact);
    for (size_t i = 0; i < nev; ++i) {
        // ||S||inf = 8; Weyl: |lam - exact| <= resid, with the rounding of the values themselves
        CHECK(r.resid[i] <= 2 * r.tol * 8.0);
        CHECK(std::fabs(r.lam[i] - exact[i]) <= r.resid[i] + 4 * (double)n * 0x1p-53 * 8.0);
        std::printf("pair %zu %a %a\n", i, r.lam[i], r.resid[i]);
        for (uint64_t row = 0; row < n; ++row)
            std::printf("y %zu %llu %a\n", i, (unsigned long long)row, r.vectors.get_col(i)[row]);
    }
    bool refused = false;
    try {
        (void)f.eigsh(a, nev, 4, 0, -1.0);
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    CHECK(refused);
    refused = false;
    try {
        (void)f.eigsh(poisson(4), nev);
    } catch (const bsm::Panic&) {
        refused = true;
    }
    CHECK(refused);
    refused = false;
    try {
        (void)f.eigsh(a, nev, 33);  // the library names the argument
    } catch (const std::exception& e) {
        refused = std::strstr(e.what(), "block") != nullptr;
    }
    CHECK(refused);
}

static void touch_device() {
    const auto f = bsm::cholesky_nd_as<float>(poisson(4));
    (void)f.eigsh(poisson(4), 2);
}

int main(int argc, char** argv) {
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "eigsh (DeviceError without a GPU: no CPU fallback)");
}
