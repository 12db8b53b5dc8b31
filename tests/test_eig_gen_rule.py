"""The generalised problem A y = lambda M y through the rule of the block
shift-invert Lanczos (csrc/eig_rule.hpp) as a stand-alone CPU program
(tests/cpp/eig_gen_rule_test.cpp), built with -fsanitize=address,undefined as
tests/test_eig_rule.py builds its own and run directly: the whole loop in the M
inner product on the host, with a dense A^-1 and a dense M, on the 9 x 9-grid
Poisson matrix and its consistent mass matrix. Block 4 must return both copies
of the double eigenvalues, against the header's own Jacobi solver on L_M^-1 A
L_M^-T; the vectors must be M-orthonormal; a step must take three products
with M; and the positive-definiteness rule (eig_mass_pd) must fire on M = -I
and on a zero block."""

from cpp_support import run_sanitized


def test_eig_gen_rule_under_sanitizer():
    run_sanitized("eig_gen_rule_test.cpp")
