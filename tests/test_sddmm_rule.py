"""The host rule of the SDDMM's dot product (csrc/sddmm_rule.hpp: W(k), the
lanes per entry, and sddmm_tree, the one order in which an entry's k products
are added) as a stand-alone CPU program (tests/cpp/sddmm_rule_test.cpp), built
with -fsanitize=address,undefined as tests/test_reach_rule.py builds
reach_rule.hpp's: sddmm_tree against an independently written recursive
pairwise definition for k = 1..130 in f32 and f64, bit for bit, on arrays of
exactly k terms, and W(k) / the lanes at k = 1, 2, 3, 4, 5, 31, 32, 33, 63,
64, 65, 129."""

from cpp_support import run_sanitized


def test_sddmm_rule_under_sanitizer():
    run_sanitized("sddmm_rule_test.cpp", extra_flags=["-ffp-contract=off"])
