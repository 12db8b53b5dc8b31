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

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_sparse_matrix_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "spmm_rule_test.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")


def test_spmm_rule_under_sanitizer():
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "spmm_rule_test_asan_ubsan")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and any(w in r.stderr.lower() for w in ("asan", "ubsan")):
        pytest.skip("no sanitizer runtime for -fsanitize=address,undefined: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr
    san_env = {"ASAN_OPTIONS": "exitcode=66", "UBSAN_OPTIONS": "halt_on_error=1 print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, **san_env))
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " 0 failed" in r.stdout

