// bsm::NdFactor<T>::solve_sparse / inv_block (include/bsm.hpp) on a 2-D
// Poisson system: a sparse b of three columns (two point sources and an empty
// column) at a few rows and at every row equals the dense solve of the
// densified b, entry for entry; inv_block equals the solves of unit columns;
// the counts say that fronts were skipped; a b of another row count and a row
// >= n are refused.
//   (no argument)        the GPU run
//   --expect-no-device   the constructor must throw bsm::DeviceError
#include <array>
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
    bsm::NdFactor<double> f(poisson(g));
    std::vector<std::vector<double>> bd(n, std::vector<double>(3, 0.0));  // rows of b
    bd[5][0] = 1.0;
    bd[97][0] = -0.5;
    bd[60][2] = 2.0;
    const auto b = Csr<double>::from_data(bd);
    std::vector<std::vector<double>> cols(3, std::vector<double>(n, 0.0));
    for (uint64_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) cols[c][i] = bd[i][c];
    const auto want = f.solve(Dense<double>::from_data(cols));
    const std::vector<uint64_t> rows = {120, 0, 60, 60, 5};
    std::array<uint32_t, 4> info{};
    const auto x = f.solve_sparse(b, &rows, &info);
    CHECK(x.get_dims().rows == rows.size() && x.get_dims().cols == 3);
    for (size_t c = 0; c < 3; ++c)
        for (size_t e = 0; e < rows.size(); ++e) CHECK(x.get_col(c)[e] == want.get_col(c)[rows[e]]);
    CHECK(info[0] > 0 && info[0] < info[2] && info[1] > 0 && info[1] < info[2] && info[3] == 1);
    const auto xa = f.solve_sparse(b);
    CHECK(xa.get_dims().rows == n);
    for (size_t c = 0; c < 3; ++c)
        for (uint64_t i = 0; i < n; ++i) CHECK(xa.get_col(c)[i] == want.get_col(c)[i]);
    const std::vector<uint64_t> none;
    CHECK(f.solve_sparse(b, &none).get_dims().rows == 0);
    // inv_block against the solves of unit columns
    const std::vector<uint64_t> bc = {5, 60};
    std::vector<std::vector<double>> unit(2, std::vector<double>(n, 0.0));
    unit[0][5] = 1.0;
    unit[1][60] = 1.0;
    const auto z = f.solve(Dense<double>::from_data(unit));
    const auto blk = f.inv_block(rows, bc);
    CHECK(blk.size() == rows.size() * 2);
    for (size_t e = 0; e < rows.size(); ++e)
        for (size_t j = 0; j < 2; ++j) CHECK(blk[e * 2 + j] == z.get_col(j)[rows[e]]);
    // refusals
    bd.push_back({0.0, 0.0, 1.0});
    CHECK(throws([&] { f.solve_sparse(Csr<double>::from_data(bd)); }));
    const std::vector<uint64_t> far = {n};
    CHECK(throws([&] { f.solve_sparse(b, &far); }));
    CHECK(throws([&] { f.inv_block(rows, far); }));
}

static void touch_device() {
    bsm::NdFactor<double> f(poisson(4));
    f.solve_sparse(Csr<double>::from_data({{1.0}}));
}

int main(int argc, char** argv) {
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "NdFactor (DeviceError without a GPU: no CPU fallback)");
}
