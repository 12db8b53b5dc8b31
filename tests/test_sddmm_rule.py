"""The host rule of the SDDMM's dot product (csrc/sddmm_rule.hpp: W(k), the
lanes per entry, and sddmm_tree, the one order in which an entry's k products
are added) as a stand-alone CPU program (tests/cpp/sddmm_rule_test.cpp), built
with -fsanitize=address,undefined as tests/test_reach_rule.py builds
reach_rule.hpp's: sddmm_tree against an independently written recursive
pairwise definition for k = 1..130 in f32 and f64, bit for bit, on arrays of
exactly k terms, and W(k) / the lanes at k = 1, 2, 3, 4, 5, 31, 32, 33, 63,
64, 65, 129."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_sparse_matrix_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "sddmm_rule_test.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")


def test_sddmm_rule_under_sanitizer():
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "sddmm_rule_test_asan_ubsan")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and any(w in r.stderr.lower() for w in ("asan", "ubsan")):
        pytest.skip("no sanitizer runtime for -fsanitize=address,undefined: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr
    san_env = {"ASAN_OPTIONS": "exitcode=66", "UBSAN_OPTIONS": "halt_on_error=1 print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, **san_env))
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " 0 failed" in r.stdout
