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

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_sparse_matrix_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "eig_gen_rule_test.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")


def test_eig_gen_rule_under_sanitizer():
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "eig_gen_rule_test_asan_ubsan")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and any(w in r.stderr.lower() for w in ("asan", "ubsan")):
        pytest.skip("no sanitizer runtime for -fsanitize=address,undefined: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr
    san_env = {"ASAN_OPTIONS": "exitcode=66", "UBSAN_OPTIONS": "halt_on_error=1 print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, **san_env))
    print(r.stdout)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " 0 failed" in r.stdout
