// What the test_nd_*.cpp drivers of the C++ mirror (include/bsm.hpp) share:
// the check counters, the 2-D Poisson matrix from the oracle's generator, and
// the two modes of main. The functions are inline, not static: the drivers
// compile with -Wall -Wextra -Werror, and not every driver uses every one.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "bsm.hpp"
#include "../../oracle/bsm_oracle.h"

inline int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            ++g_fail;                                                      \
            std::fprintf(stderr, "  CHECK failed: %s (line %d)\n", #cond, __LINE__); \
        }                                                                  \
    } while (0)

// the CSR arrays of the g x g grid's 5-point matrix (orc_gen_poisson2d), for a driver that changes values first
struct Grid {
    uint64_t n;
    std::vector<uint64_t> rp, ci;
    std::vector<double> v;

    explicit Grid(uint64_t g) : n(g * g), rp(n + 1), ci(5 * n), v(5 * n) {
        const uint64_t nnz = orc_gen_poisson2d(g, rp.data(), ci.data(), v.data());
        ci.resize(nnz);
        v.resize(nnz);
    }
    bsm::Csr<double> csr() const {
        return bsm::Csr<double>::from_csr_arrays({n, n}, {rp.begin(), rp.end()}, {ci.begin(), ci.end()}, v);
    }
};

inline bsm::Csr<double> poisson(uint64_t g, double factor = 1.0) {
    Grid a(g);
    for (double& e : a.v) e *= factor;
    return a.csr();
}

// main: with --expect-no-device, touch_device (the feature's calls on a small system) must throw bsm::DeviceError
// and no CHECK may have failed before; otherwise run_gpu, then the summary line the Python driver looks for.
// `what` names the feature in the PASS / FAIL line.
inline int nd_test_main(int argc, char** argv, void (*run_gpu)(), void (*touch_device)(), const char* what) {
    if (argc > 1 && std::strcmp(argv[1], "--expect-no-device") == 0) {
        bool dev_err = false;
        try {
            touch_device();
        } catch (const bsm::DeviceError&) {
            dev_err = true;
        } catch (...) {
        }
        const bool ok = dev_err && g_fail == 0;
        std::printf("%s %s\n", ok ? "PASS" : "FAIL", what);
        return ok ? 0 : 1;
    }
    try {
        run_gpu();
    } catch (const std::exception& e) {
        ++g_fail;
        std::fprintf(stderr, "  EXCEPTION: %s\n", e.what());
    }
    std::printf("summary: %d failed, %d checks\n", g_fail, g_checks);
    return g_fail ? 1 : 0;
}
