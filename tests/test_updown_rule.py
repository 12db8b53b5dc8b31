"""The scalar rule of the kept factor's rank-k update and downdate
(csrc/updown_rule.hpp: a pivot's c and s, the "not positive definite" test, a
row's new L_ij and w_i, the skip on w_j == 0) as a stand-alone CPU program
(tests/cpp/updown_rule_test.cpp), built with -fsanitize=address,undefined as
tests/test_pcg_rule.py builds pcg_rule.hpp's: L L^T after an update and after
a downdate of the 9 x 9 grid's dense factor, a downdate that is not positive
definite at a named pivot, w_j == 0 leaving column j's bits, a rank-3 call in
column order; in f64 and f32."""

from cpp_support import run_sanitized


def test_updown_rule_under_sanitizer():
    run_sanitized("updown_rule_test.cpp")
