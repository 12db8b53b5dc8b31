// bsm::NdFactor<double>::inv_diag / inv_entries (include/bsm.hpp) on a 2-D
// Poisson system: the diagonal against n solves with unit vectors, the
// diagonal pairs through inv_entries bit for bit, both triangles, and the
// refusals. Prints the diagonal ("diag <index> <hexfloat>") for
// tests/test_cpp_nd_selinv.py, which compares it with Python's.
//   (no argument)        the GPU run
//   --expect-no-device   the constructor must throw bsm::DeviceError
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
    const bsm::NdFactor<double> f(a);
    const std::vector<double> d = f.inv_diag();
    CHECK(d.size() == n);
    for (uint64_t i = 0; i < n; ++i) std::printf("diag %llu %a\n", (unsigned long long)i, d[i]);
    // against the solves with unit vectors
    std::vector<std::vector<double>> eye(n, std::vector<double>(n, 0.0));
    for (uint64_t i = 0; i < n; ++i) eye[i][i] = 1.0;
    const auto x = f.solve(Dense<double>::from_data(eye));
    double worst = 0.0;
    for (uint64_t i = 0; i < n; ++i) worst = std::fmax(worst, std::fabs(d[i] - x.get_col(i)[i]) / std::fabs(d[i]));
    CHECK(worst <= 1e-12);
    // the diagonal pairs and A's own entries through inv_entries
    std::vector<uint64_t> idx(n);
    for (uint64_t i = 0; i < n; ++i) idx[i] = i;
    const auto dd = f.inv_entries(idx, idx);
    CHECK(std::memcmp(dd.data(), d.data(), n * sizeof(double)) == 0);
    std::vector<uint64_t> rows;
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t e = a.row_index()[i]; e < a.row_index()[i + 1]; ++e) rows.push_back(i);
    const std::vector<uint64_t> cols(a.col_index().begin(), a.col_index().end());
    const auto lower = f.inv_entries(rows, cols), upper = f.inv_entries(cols, rows);
    CHECK(lower.size() == cols.size());
    CHECK(std::memcmp(lower.data(), upper.data(), lower.size() * sizeof(double)) == 0);
    double werr = 0.0;
    for (size_t e = 0; e < rows.size(); ++e)
        werr = std::fmax(werr, std::fabs(lower[e] - x.get_col(cols[e])[rows[e]]));
    CHECK(werr <= 1e-12);
    CHECK(f.inv_entries({}, {}).empty());
    bool refused = false;
    try {
        (void)f.inv_entries({0, n}, {0, 0});
    } catch (const std::exception&) {
        refused = true;
    }
    CHECK(refused);
    CHECK(f.inv_diag() == d);
}

static void touch_device() {
    bsm::NdFactor<double> f(poisson(4));
    (void)f.inv_diag();
}

int main(int argc, char** argv) {
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "NdFactor (DeviceError without a GPU: no CPU fallback)");
}
