"""The refined solve's per-column rule (csrc/refine_rule.hpp: which columns go
on, have converged, have stagnated, which iterate is the best; the scale; the
default tol) as a stand-alone CPU program (tests/cpp/refine_rule_test.cpp),
built with -fsanitize=address,undefined as tests/test_xfer_host.py builds
xfer_host.hpp's: omega sequences that converge, stagnate at the floor, diverge,
turn NaN, a zero right-hand side, mixed columns."""

from cpp_support import run_sanitized


def test_refine_rule_under_sanitizer():
    run_sanitized("refine_rule_test.cpp")
