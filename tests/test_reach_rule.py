"""The host rule of the kept factor's solve with sparse right-hand sides and
selected rows (csrc/reach_rule.hpp: the fronts on the paths from some start
nodes to the roots, in (level, node) order with each level's first place, and
per front which of its two children are in the set) as a stand-alone CPU
program (tests/cpp/reach_rule_test.cpp), built with
-fsanitize=address,undefined as tests/test_updown_rule.py builds
updown_rule.hpp's: against a brute-force union of root paths on 300 small
random forests with roots on several levels, nodes with one child in either
slot, empty, repeated and skipped start nodes."""

from cpp_support import run_sanitized


def test_reach_rule_under_sanitizer():
    run_sanitized("reach_rule_test.cpp")
