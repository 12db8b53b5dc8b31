// The per-column rule of the pcg solve (csrc/pcg_rule.hpp) as a stand-alone
// CPU program: a column that converges at x_0, a verification that passes,
// one that fails and restarts with beta = 0, breakdowns on p . q <= 0, on NaN
// and on r . z <= 0, max_iter reached, a non-finite omega, a zero right-hand
// side. Built with -fsanitize=address,undefined by tests/test_pcg_rule.py.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "pcg_rule.hpp"

using bsm::PcgCol;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) {                                                               \
            ++g_fail;                                                                \
            std::fprintf(stderr, "  CHECK failed: %s (line %d)\n", #cond, __LINE__); \
        }                                                                            \
    } while (0)

// One step of the device loop on a column, from the numbers its kernels
// would have reduced: r . z and q . z after the solve, p . q after the
// product, the recurrence's omega, and the true omega should it be asked for.
struct Step {
    double rz, qz, pq, omega_rec, omega_true;
};

// Drives the column as kernels_pcg.hip's host loop does; returns the steps
// on which the true residual was formed.
static std::vector<unsigned> drive(PcgCol& c, double bnorm, double omega0, const std::vector<Step>& steps,
                                   unsigned max_iter, double tol, std::vector<double>* betas = nullptr) {
    std::vector<unsigned> verified_at;
    bsm::pcg_rule_init(c, bnorm, omega0, omega0, tol);
    for (unsigned it = 1; it <= max_iter && it <= steps.size() && c.active; ++it) {
        const Step& s = steps[it - 1];
        bsm::pcg_rule_beta(c, s.rz, s.qz);
        if (betas && c.active) betas->push_back(c.beta);
        bsm::pcg_rule_alpha(c, s.pq);
        bsm::pcg_rule_step(c, it, s.omega_rec, s.omega_rec, tol);
        if (c.verify) {
            verified_at.push_back(it);
            bsm::pcg_rule_verified(c, s.omega_true, s.omega_true, tol);
        }
    }
    return verified_at;
}

int main() {
    const double tol = 7 * 0x1p-53, nan = std::numeric_limits<double>::quiet_NaN(),
                 inf = std::numeric_limits<double>::infinity();
    {  // converged at x_0: nothing runs
        PcgCol c;
        const auto v = drive(c, 1.0, tol, {{1, 1, 1, 0, 0}}, 50, tol);
        CHECK(!c.active && c.iters == 0 && c.verified && c.omega == tol && !c.breakdown && !c.zero && v.empty());
        bsm::pcg_rule_final(c, 0.5);  // an omega it has no use for
        CHECK(c.omega == tol);
    }
    {  // two steps, the second's verification passes
        PcgCol c;
        std::vector<double> betas;
        const auto v = drive(c, 1.0, 1e-3, {{4.0, 9.0, 2.0, 1e-6, nan}, {1.0, -0.25, 0.5, 1e-17, 2e-16}}, 50, tol, &betas);
        CHECK(v.size() == 1 && v[0] == 2);
        CHECK(!c.active && c.iters == 2 && c.verified && c.omega == 2e-16 && !c.breakdown && !c.verify);
        CHECK(betas.size() == 2 && betas[0] == 0.0);    // the first direction is z
        CHECK(betas[1] == -(4.0 / 2.0) * -0.25 / 4.0);  // -alpha (q . z) / rho
        CHECK(c.alpha == 1.0 / 0.5 && c.rho == 1.0);
    }
    {  // a verification that fails: the true residual replaces r, beta = 0 once, the step counts
        PcgCol c;
        std::vector<double> betas;
        const std::vector<Step> steps = {{4.0, 0.0, 2.0, 1e-17, 1e-9},    // asks, fails
                                         {3.0, 5.0, 1.0, 1e-12, nan},     // the restart's step: beta = 0
                                         {2.0, -1.0, 1.0, 1e-16, 1e-16}};  // beta from the dots again; passes
        const auto v = drive(c, 1.0, 1e-3, steps, 50, tol, &betas);
        CHECK(v.size() == 2 && v[0] == 1 && v[1] == 3);
        CHECK(betas.size() == 3 && betas[0] == 0.0 && betas[1] == 0.0 && betas[2] == -(3.0 / 1.0) * -1.0 / 3.0);
        CHECK(!c.active && c.iters == 3 && c.verified && c.omega == 1e-16 && !c.restart);
        PcgCol d;  // the state right after the failed verification
        (void)drive(d, 1.0, 1e-3, {steps[0]}, 50, tol);
        CHECK(d.active && d.restart && d.verified && !d.verify && d.omega == 1e-9 && d.iters == 1);
        CHECK(d.scale == bsm::refine_scale(1e-9));
    }
    {  // breakdown on p . q <= 0 in the first step: x stays x_0
        PcgCol c;
        (void)drive(c, 1.0, 1e-3, {{4.0, 0.0, -2.0, 1e-6, nan}}, 50, tol);
        CHECK(!c.active && c.breakdown && c.iters == 0 && c.verified && c.omega == 1e-3);
        PcgCol z;
        (void)drive(z, 1.0, 1e-3, {{4.0, 0.0, 0.0, 1e-6, nan}}, 50, tol);
        CHECK(!z.active && z.breakdown && z.iters == 0);
    }
    {  // breakdown on NaN and infinity, after a completed step: the end asks for that x's true omega
        for (double bad : {nan, inf, -inf}) {
            PcgCol c;
            (void)drive(c, 1.0, 1e-3, {{4.0, 0.0, 2.0, 1e-6, nan}, {1.0, 0.5, bad, 1e-9, nan}}, 50, tol);
            CHECK(!c.active && c.breakdown && c.iters == 1 && !c.verified && c.omega == 1e-6);
            bsm::pcg_rule_final(c, 3e-6);
            CHECK(c.verified && c.omega == 3e-6 && c.breakdown && c.iters == 1);
        }
    }
    {  // breakdown on r . z <= 0 or NaN
        for (double bad : {0.0, -1.0, nan}) {
            PcgCol c;
            (void)drive(c, 1.0, 1e-3, {{4.0, 0.0, 2.0, 1e-6, nan}, {bad, 0.5, 1.0, 1e-9, nan}}, 50, tol);
            CHECK(!c.active && c.breakdown && c.iters == 1 && c.rho == 4.0);
        }
        PcgCol c;  // a q . z that is not finite gives no beta
        (void)drive(c, 1.0, 1e-3, {{4.0, 0.0, 2.0, 1e-6, nan}, {1.0, nan, 1.0, 1e-9, nan}}, 50, tol);
        CHECK(!c.active && c.breakdown && c.iters == 1);
    }
    {  // max_iter reached: still active for the rule, the end reports the true omega
        PcgCol c;
        const std::vector<Step> steps(10, Step{1.0, 0.1, 1.0, 1e-6, nan});
        (void)drive(c, 1.0, 1e-3, steps, 4, tol);
        CHECK(c.active && c.iters == 4 && !c.verified && !c.breakdown);
        bsm::pcg_rule_final(c, 2e-6);
        CHECK(!c.active && c.verified && c.omega == 2e-6 && c.iters == 4);
        PcgCol d;  // max_iter == 0: the first iterate alone
        (void)drive(d, 1.0, 1e-3, steps, 0, tol);
        CHECK(d.active && d.iters == 0 && d.verified && d.omega == 1e-3);
    }
    {  // a non-finite omega stops the column, at x_0 and after a step
        PcgCol c;
        (void)drive(c, 1.0, nan, {{1, 1, 1, 0, 0}}, 50, tol);
        CHECK(!c.active && c.iters == 0 && !c.breakdown && std::isnan(c.omega));
        PcgCol d;
        (void)drive(d, 1.0, 1e-3, {{4.0, 0.0, 2.0, inf, nan}, {1, 1, 1, 0, 0}}, 50, tol);
        CHECK(!d.active && d.iters == 1 && !d.breakdown && !d.verify);
    }
    {  // a zero right-hand side
        PcgCol c;
        (void)drive(c, 0.0, nan, {{1, 1, 1, 0, 0}}, 50, tol);
        CHECK(c.zero && !c.active && c.iters == 0 && c.omega == 0.0 && !c.breakdown);
        bsm::pcg_rule_final(c, 1.0);
        CHECK(c.omega == 0.0);
    }
    {  // a stopped column ignores every call
        PcgCol c;
        (void)drive(c, 1.0, tol / 2, {}, 50, tol);
        const PcgCol before = c;
        bsm::pcg_rule_beta(c, 1.0, 1.0);
        bsm::pcg_rule_alpha(c, 1.0);
        bsm::pcg_rule_step(c, 9, 1e-3, 1e-3, tol);
        bsm::pcg_rule_verified(c, 1e-3, 1e-3, tol);
        CHECK(c.iters == before.iters && c.omega == before.omega && c.active == 0 && c.rho == before.rho &&
              c.alpha == before.alpha && !c.breakdown);
    }
    std::printf("summary: %d failed, %d checks\n", g_fail, g_checks);
    return g_fail ? 1 : 0;
}
