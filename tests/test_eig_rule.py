"""The rule of the block shift-invert Lanczos (csrc/eig_rule.hpp: the argument
checks, the p x p Cholesky with its rank rule, the symmetric eigen-solver, the
residual estimate and the stop rule) as a stand-alone CPU program
(tests/cpp/eig_rule_test.cpp), built with -fsanitize=address,undefined as
tests/test_pcg_rule.py builds pcg_rule.hpp's: the eigen-solver against analytic
eigenvalues, on a double eigenvalue and on 1 x 1; the rank rule on a full-rank
Gram matrix, on two equal columns and on a zero block; the stop rule; and the
whole loop on the host with a dense operator on the 5 x 5-grid Poisson matrix,
where block 4 must return both copies of the double eigenvalues and block 1
must not."""

from cpp_support import run_sanitized


def test_eig_rule_under_sanitizer():
    run_sanitized("eig_rule_test.cpp")
