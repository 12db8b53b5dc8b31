// The per-column rule of the refined solve (csrc/refine_rule.hpp) as a
// stand-alone CPU program: omega sequences that converge, stagnate at the
// floor, diverge, turn NaN, a zero right-hand side, and columns of several
// kinds side by side; the scale and the default tol. Built with
// -fsanitize=address,undefined by tests/test_refine_rule.py.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "refine_rule.hpp"

using bsm::RefineCol;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) {                                                               \
            ++g_fail;                                                                \
            std::fprintf(stderr, "  CHECK failed: %s (line %d)\n", #cond, __LINE__); \
        }                                                                            \
    } while (0)

// Drive one column through omegas[0] (the first iterate), omegas[1], ... as
// the device loop does, for at most max_iter corrections; returns the index
// of the iterate the rule calls best.
static int drive(RefineCol& c, double bnorm, const std::vector<double>& omegas, unsigned max_iter, double tol) {
    bsm::refine_rule_init(c, bnorm, omegas[0], omegas[0], tol);
    int best = 0;
    for (unsigned it = 1; it <= max_iter && it < omegas.size() && c.active; ++it) {
        bsm::refine_rule_step(c, it, omegas[it], omegas[it], tol);
        best = c.use_prev ? (int)it - 1 : (int)it;
    }
    return best;
}

int main() {
    const double tol = 7 * 0x1p-53, nan = std::numeric_limits<double>::quiet_NaN(),
                 inf = std::numeric_limits<double>::infinity();
    {  // converging: an f32 factor's 1e-7 -> 4e-14 -> 7e-17
        RefineCol c;
        const int best = drive(c, 1.0, {1e-7, 4.2e-14, 6.6e-17, 1e-30}, 5, tol);
        CHECK(best == 2 && c.iters == 2 && !c.active && c.best == 6.6e-17 && !c.use_prev && !c.zero);
    }
    {  // already below tol: no correction
        RefineCol c;
        const int best = drive(c, 1.0, {1e-17, 1.0}, 5, tol);
        CHECK(best == 0 && c.iters == 0 && !c.active && c.best == 1e-17);
    }
    {  // max_iter ends it: the latest iterate is the best, the column still wants more
        RefineCol c;
        const int best = drive(c, 1.0, {1e-2, 1e-4, 1e-6, 1e-8, 1e-10}, 3, tol);
        CHECK(best == 3 && c.iters == 3 && c.active && c.best == 1e-8);
    }
    {  // stagnating above tol: better than before, but not by half -> stops, keeps the better one
        RefineCol c;
        const int best = drive(c, 1.0, {1e-7, 1e-12, 0.9e-12, 1e-20}, 9, tol);
        CHECK(best == 2 && c.iters == 2 && !c.active && c.best == 0.9e-12 && c.best > tol);
    }
    {  // stagnating and worse: the iterate before is kept
        RefineCol c;
        const int best = drive(c, 1.0, {1e-7, 1e-12, 1.1e-12, 1e-20}, 9, tol);
        CHECK(best == 1 && c.iters == 2 && !c.active && c.best == 1e-12 && c.use_prev);
    }
    {  // diverging: the first iterate stays
        RefineCol c;
        const int best = drive(c, 1.0, {0.5, 1.0, 2.0}, 5, tol);
        CHECK(best == 0 && c.iters == 1 && !c.active && c.best == 0.5 && c.use_prev);
    }
    {  // NaN after a step: stops, never the best
        RefineCol c;
        const int best = drive(c, 1.0, {1e-3, nan, 1e-9}, 5, tol);
        CHECK(best == 0 && c.iters == 1 && !c.active && c.best == 1e-3 && c.use_prev);
    }
    {  // not finite from the start: nothing is tried
        RefineCol c, d;
        CHECK(drive(c, 1.0, {nan, 1e-9}, 5, tol) == 0 && c.iters == 0 && !c.active && std::isnan(c.best));
        CHECK(drive(d, 1.0, {inf, 1e-9}, 5, tol) == 0 && d.iters == 0 && !d.active && std::isinf(d.best));
    }
    {  // inf after a step
        RefineCol c;
        CHECK(drive(c, 1.0, {1e-3, inf}, 5, tol) == 0 && c.iters == 1 && !c.active && c.best == 1e-3);
    }
    {  // a zero right-hand side: x = 0, berr 0, whatever omega came out of 0 / 0
        RefineCol c;
        CHECK(drive(c, 0.0, {nan, 1.0}, 5, tol) == 0 && c.zero && !c.active && c.iters == 0 && c.best == 0.0);
        CHECK(bsm::refine_omega(0.0, 0.0, 0.0, 8.0) == 0.0);
    }
    {  // mixed columns in one loop: each stops on its own, an inactive one is never touched again
        const std::vector<std::vector<double>> seq = {{1e-7, 1e-14, 1e-17, 1.0, 1.0},
                                                      {1e-3, 1e-4, 1e-5, 1e-6, 1e-7},
                                                      {1e-17, 1.0, 1.0, 1.0, 1.0},
                                                      {0.5, 1.0, 1e-20, 1e-20, 1e-20}};
        std::vector<RefineCol> cols(seq.size());
        for (size_t j = 0; j < seq.size(); ++j) bsm::refine_rule_init(cols[j], 1.0, seq[j][0], seq[j][0], tol);
        unsigned it = 0;
        for (;;) {
            bool any = false;
            for (const auto& c : cols) any = any || c.active;
            if (!any || it >= 4) break;
            ++it;
            for (size_t j = 0; j < seq.size(); ++j) bsm::refine_rule_step(cols[j], it, seq[j][it], seq[j][it], tol);
        }
        CHECK(it == 4);
        CHECK(cols[0].iters == 2 && cols[0].best == 1e-17 && !cols[0].use_prev);
        CHECK(cols[1].iters == 4 && cols[1].best == 1e-7 && cols[1].active);
        CHECK(cols[2].iters == 0 && cols[2].best == 1e-17);
        CHECK(cols[3].iters == 1 && cols[3].best == 0.5 && cols[3].use_prev);
    }
    // the scale: 2^floor(log2 v), 1 where there is nothing to scale by
    CHECK(bsm::refine_scale(1.0) == 1.0 && bsm::refine_scale(1.999) == 1.0 && bsm::refine_scale(2.0) == 2.0);
    CHECK(bsm::refine_scale(0.75) == 0.5 && bsm::refine_scale(1e-13) == std::ldexp(1.0, -44));
    CHECK(bsm::refine_scale(0x1p-1060) == 0x1p-1060 && bsm::refine_scale(std::numeric_limits<double>::max()) == 0x1p1023);
    CHECK(bsm::refine_scale(0.0) == 1.0 && bsm::refine_scale(nan) == 1.0 && bsm::refine_scale(inf) == 1.0 &&
          bsm::refine_scale(-3.0) == 1.0);
    for (double v : {1e-300, 3e-20, 0.1, 5.0, 1e200}) {
        const double q = v / bsm::refine_scale(v);
        CHECK(q >= 1.0 && q < 2.0);
    }
    CHECK(bsm::refine_omega(1.0, 2.0, 3.0, 4.0) == 1.0 / 11.0);
    CHECK(std::isnan(bsm::refine_omega(nan, 1.0, 1.0, 1.0)));
    CHECK(bsm::refine_default_tol(5) == 7 * 0x1p-53 && bsm::refine_default_tol(0) == 2 * 0x1p-53);
    std::printf("summary: %d failed, %d checks\n", g_fail, g_checks);
    return g_fail ? 1 : 0;
}
