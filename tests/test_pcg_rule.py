"""The pcg solve's per-column rule (csrc/pcg_rule.hpp: the step length, the
flexible beta, when a column asks for its true residual, restarts, stops or
has broken down) as a stand-alone CPU program (tests/cpp/pcg_rule_test.cpp),
built with -fsanitize=address,undefined as tests/test_refine_rule.py builds
refine_rule.hpp's: convergence at x_0, a verification that passes, one that
fails and restarts with beta = 0, breakdowns, max_iter, a zero column."""

from cpp_support import run_sanitized


def test_pcg_rule_under_sanitizer():
    run_sanitized("pcg_rule_test.cpp")
