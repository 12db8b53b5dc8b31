// bsm::NdFactor::eigsh_gen (include/bsm.hpp) on the 11 x 11-grid Poisson matrix
// with its consistent mass matrix kron(M1, M1), M1 = tridiag(1/6, 4/6, 1/6):
// the six smallest pairs of S y = lam S_M y by block shift-invert Lanczos on
// the f32 factor, against the analytic values (k_p + k_q) / (m_p m_q). Prints
// lam and resid ("pair <i> <lam> <resid>"), the vectors ("y <pair> <row>
// <hexfloat>") and the info ("info <steps> <ncv_used> <converged> <exhausted>
// <inexact>") for tests/test_cpp_nd_eig_gen.py, which compares them with
// Python's. The argument errors of the C entry points are checked first, in
// every mode: they need no device.
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

// kron(M1, M1), rows and columns ascending: the values 16/36, 4/36 and 1/36 as Python's np.kron(m1, m1) rounds them
static Csr<double> consistent_mass(uint64_t g) {
    const uint64_t n = g * g;
    std::vector<size_t> rp{0}, ci;
    std::vector<double> v;
    auto m1 = [](int64_t d) { return (d == 0 ? 4.0 : 1.0) / 6.0; };
    for (int64_t i = 0; i < (int64_t)g; ++i)
        for (int64_t j = 0; j < (int64_t)g; ++j) {
            for (int64_t di = -1; di <= 1; ++di)
                for (int64_t dj = -1; dj <= 1; ++dj) {
                    const int64_t i2 = i + di, j2 = j + dj;
                    if (i2 < 0 || i2 >= (int64_t)g || j2 < 0 || j2 >= (int64_t)g) continue;
                    ci.push_back((size_t)(i2 * (int64_t)g + j2));
                    v.push_back(m1(di) * m1(dj));
                }
            rp.push_back(ci.size());
        }
    return Csr<double>::from_csr_arrays({n, n}, rp, ci, v);
}

// the C entry points refuse bad arguments before any device is asked for, and touch no output
static void args_without_device() {
    int fake[1024] = {0};  // never read past the refused argument; all zero: a 0 x 0 factor
    const bsm_nd_factor* f = reinterpret_cast<const bsm_nd_factor*>(fake);
    const bsm_csr* a = reinterpret_cast<const bsm_csr*>(fake);
    double y[2] = {7.0, 7.0}, lam[1] = {7.0}, resid[1] = {7.0};
    uint32_t info[4] = {7, 7, 7, 7};
    void* yc[1] = {y};
    for (const bsm_csr* m : {static_cast<const bsm_csr*>(nullptr), a}) {
        CHECK(bsm_nd_factor_eigsh_gen(nullptr, a, m, 1, 4, 0, 0.0, 0, nullptr, lam, yc, resid, info) == BSM_ERR_INVALID);
        CHECK(bsm_nd_factor_eigsh_gen(f, a, m, 1, 4, 0, -1.0, 0, nullptr, lam, yc, resid, info) == BSM_ERR_INVALID);
        CHECK(bsm_nd_factor_eigsh_gen(f, a, m, 0, 0, 0, 0.0, 0, nullptr, lam, yc, resid, info) == BSM_ERR_INVALID);
        CHECK(bsm_dev_nd_factor_eigsh_gen(f, nullptr, m, 1, 4, 0, 0.0, 0, nullptr, lam, y, resid, info, nullptr) ==
              BSM_ERR_INVALID);
        CHECK(bsm_dev_nd_factor_eigsh_gen(f, a, m, 0, 4, 0, 0.0, 0, nullptr, nullptr, y, resid, info, nullptr) ==
              BSM_ERR_INVALID);
        CHECK(bsm_dev_nd_factor_eigsh_gen(f, a, m, 0, 33, 0, 0.0, 0, nullptr, lam, y, resid, nullptr, nullptr) ==
              BSM_ERR_INVALID);
    }
    CHECK(y[0] == 7.0 && y[1] == 7.0 && lam[0] == 7.0 && resid[0] == 7.0 && info[0] == 7 && info[3] == 7);
}

static void run_gpu() {
    const uint64_t g = 11, n = g * g;
    const size_t nev = 6;
    const auto a = poisson(g);
    const auto m = consistent_mass(g);
    const bsm::NdFactor<float> f = bsm::cholesky_nd_as<float>(a);
    const auto r = f.eigsh_gen(a, m, nev, 4, 60);
    CHECK(r.lam.size() == nev && r.resid.size() == nev && r.tol == 0x1p-26);
    CHECK(r.converged == nev && !r.inexact && !r.exhausted && r.ncv_used <= 60 && r.steps * 4 == r.ncv_used);
    std::vector<double> exact;
    const double pi = 3.14159265358979323846;
    for (uint64_t p = 1; p <= g; ++p)
        for (uint64_t q = 1; q <= g; ++q) {
            const double cp = std::cos(p * pi / 12), cq = std::cos(q * pi / 12);
            exact.push_back(((2.0 - 2.0 * cp) + (2.0 - 2.0 * cq)) / (((4.0 + 2.0 * cp) / 6.0) * ((4.0 + 2.0 * cq) / 6.0)));
        }
    std::sort(exact.begin(), exact.end());
    std::printf("info %u %u %u %d %d\n", r.steps, r.ncv_used, r.converged, (int)r.exhausted, (int)r.inexact);
    for (size_t i = 0; i < nev; ++i) {
        // ||S||inf = 8, ||S_M||inf = 1, mu_min > 1/9 and mu_max < 1: resid <= 2 tol ||S||inf sqrt(mu_max / mu_min),
        // and |lam - exact| <= resid ||y||2 / sqrt(mu_min) with ||y||2 <= mu_min^-1/2, plus the values' rounding
        CHECK(r.resid[i] <= 2 * r.tol * 8.0 * 3.0);
        CHECK(std::fabs(r.lam[i] - exact[i]) <= 9.0 * r.resid[i] + 4 * (double)n * 0x1p-53 * (8.0 + exact[nev - 1]) * 9.0);
        std::printf("pair %zu %a %a\n", i, r.lam[i], r.resid[i]);
        for (uint64_t row = 0; row < n; ++row)
            std::printf("y %zu %llu %a\n", i, (unsigned long long)row, r.vectors.get_col(i)[row]);
    }
    bool refused = false;
    try {
        (void)f.eigsh_gen(a, m, nev, 4, 0, -1.0);
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    CHECK(refused);
    refused = false;
    try {
        (void)f.eigsh_gen(a, consistent_mass(4), nev);
    } catch (const bsm::Panic&) {
        refused = true;
    }
    CHECK(refused);
    refused = false;
    try {
        (void)f.eigsh_gen(a, m, nev, 33);  // the library names the argument
    } catch (const std::exception& e) {
        refused = std::strstr(e.what(), "block") != nullptr;
    }
    CHECK(refused);
}

static void touch_device() {
    const auto f = bsm::cholesky_nd_as<float>(poisson(4));
    (void)f.eigsh_gen(poisson(4), consistent_mass(4), 2);
}

int main(int argc, char** argv) {
    args_without_device();
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "eigsh_gen (argument errors without a device; DeviceError without a GPU: no CPU fallback)");
}
