"""The host rule of the kept factor's partial refactor (csrc/partial_rule.hpp:
per level that occurs, the plan's tasks, the selected tasks' count and place in
the contiguous arrays, and the chunks the device marks, scans and scatters) as a
stand-alone CPU program (tests/cpp/partial_rule_test.cpp), built with
-fsanitize=address,undefined as tests/test_reach_rule.py builds
reach_rule.hpp's: against a brute-force selection on 300 small random forests
with fronts without tiles, skipped start nodes and chunk lengths from 1 to 7."""

from cpp_support import run_sanitized


def test_partial_rule_under_sanitizer():
    run_sanitized("partial_rule_test.cpp")
