// bsm::NdFactor<T>::refactor_partial / refactor_since (include/bsm.hpp) on a
// 2-D Poisson system (g = 11; the driver sets BSM_ND_LEAF=8, several levels):
// new values at a few named places, then the places found from the old matrix,
// and each time L's values, a solve, logdet and inv_diag EQUAL a fresh
// factor's, entry for entry; the counts say that fronts were skipped; a pair
// that is not stored, an index >= n, lists of different lengths and a call
// after an update are refused.
//   (no argument)        the GPU run
//   --expect-no-device   the constructor must throw bsm::DeviceError
#include <array>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include "nd_test.hpp"

using bsm::Csr;
using bsm::Dense;

// the grid's matrix with other values at the given (row, col, value), both triangles where off the diagonal
static Csr<double> poisson(uint64_t g, const std::vector<std::array<double, 3>>& ch) {
    Grid a(g);
    for (const auto& c : ch)
        for (uint64_t i = 0; i < a.n; ++i)
            for (uint64_t e = a.rp[i]; e < a.rp[i + 1]; ++e)
                if ((i == (uint64_t)c[0] && a.ci[e] == (uint64_t)c[1]) ||
                    (i == (uint64_t)c[1] && a.ci[e] == (uint64_t)c[0]))
                    a.v[e] = c[2];
    return a.csr();
}

template <class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const std::exception&) {
        return true;
    }
    return false;
}

static void same(bsm::NdFactor<double>& f, bsm::NdFactor<double>& w, uint64_t n) {
    const auto lf = f.l(), lw = w.l();
    CHECK(lf.v() == lw.v() && lf.col_index() == lw.col_index() && lf.row_index() == lw.row_index());
    std::vector<std::vector<double>> b(1, std::vector<double>(n));
    for (uint64_t i = 0; i < n; ++i) b[0][i] = ((double)(i % 7) - 3.0) / 4.0;
    const auto bd = Dense<double>::from_data(b);
    const auto xf = f.solve(bd), xw = w.solve(bd);
    bool eq = true;
    for (uint64_t i = 0; i < n; ++i) eq = eq && xf.get_col(0)[i] == xw.get_col(0)[i];
    CHECK(eq);
    CHECK(f.logdet() == w.logdet());
    CHECK(f.inv_diag() == w.inv_diag());
}

static void run_gpu() {
    const uint64_t g = 11, n = g * g;
    bsm::NdFactor<double> f(poisson(g));
    // a diagonal entry, an edge given as (j, i), a repeat
    const std::vector<std::array<double, 3>> ch = {{5, 5, 4.5}, {60, 61, -0.75}};
    const auto a2 = poisson(g, ch);
    const std::vector<uint64_t> rows = {5, 60, 5}, cols = {5, 61, 5};
    const auto info = f.refactor_partial(a2, rows, cols);
    CHECK(info[0] > 0 && info[0] < info[1] && info[2] == 3);
    {
        bsm::NdFactor<double> fresh(a2);
        same(f, fresh, n);
    }
    // the places found from the old matrix
    const std::vector<std::array<double, 3>> ch3 = {{5, 5, 4.5}, {60, 61, -0.75}, {120, 120, 5.0}, {17, 6, -0.5}};
    const auto a3 = poisson(g, ch3);
    const auto since = f.refactor_since(a2, a3);
    CHECK(since[0] > 0 && since[0] < since[1] && since[2] == 2);
    {
        bsm::NdFactor<double> fresh(a3);
        same(f, fresh, n);
    }
    const auto none = f.refactor_since(a3, a3);
    CHECK(none[0] == 0 && none[2] == 0);
    // refusals: the factor stays
    CHECK(throws([&] { f.refactor_partial(a3, {5, 0}, {5, 120}); }));  // (0, 120) is not stored
    CHECK(throws([&] { f.refactor_partial(a3, {n}, {0}); }));
    CHECK(throws([&] { f.refactor_partial(a3, {5, 6}, {5}); }));
    CHECK(throws([&] { f.refactor_partial(poisson(g + 1), {5}, {5}); }));
    {
        bsm::NdFactor<double> fresh(a3);
        same(f, fresh, n);
    }
    // after an update: refactor first
    std::vector<std::vector<double>> w(n, std::vector<double>(1, 0.0));
    w[5][0] = 0.5;
    f.update(Csr<double>::from_data(w));
    CHECK(throws([&] { f.refactor_partial(a3, {5}, {5}); }));
    f.refactor(a2);
    const auto again = f.refactor_partial(a3, {120, 17}, {120, 6});
    CHECK(again[0] == since[0]);
    {
        bsm::NdFactor<double> fresh(a3);
        same(f, fresh, n);
    }
}

static void touch_device() {
    bsm::NdFactor<double> f(poisson(4));
    f.refactor_partial(poisson(4), {0}, {0});
}

int main(int argc, char** argv) {
    return nd_test_main(argc, argv, run_gpu, touch_device,
                        "NdFactor (DeviceError without a GPU: no CPU fallback)");
}
