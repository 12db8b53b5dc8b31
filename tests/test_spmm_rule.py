"""The host rule of the SpMV / SpMM dispatch (csrc/spmm_rule.hpp: which of
the row kernels launch_spmm launches for a shape, a scalar type, the operands'
alignment and the three A/B overrides, and when the integer split schedule
replaces it) as a stand-alone CPU program (tests/cpp/spmm_rule_test.cpp),
built with -fsanitize=address,undefined as tests/test_reach_rule.py builds
reach_rule.hpp's: every threshold from both sides (nnz = 12 rows and + 1,
rows 16384 / 16385 x longest row 48 / 49 / unknown, nnz = 24 rows and + 1 at
k = 32 f64, aligned / misaligned, k at every template edge, rows = 0, the
split's 8191 / 8192 x k 1 / 2 x floats x env), every value of
BSM_SPMV_VARIANT, BSM_SPMM_VARIANT and BSM_SPMV_ITEMS and junk ones."""

from cpp_support import run_sanitized


def test_spmm_rule_under_sanitizer():
    run_sanitized("spmm_rule_test.cpp")
