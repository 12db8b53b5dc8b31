"""The host helpers of the transfer pipelines (csrc/xfer_host.hpp: the
threaded chunk copy par_memcpy and the page prefaulter Prefault) as a
stand-alone CPU program (tests/cpp/xfer_host_test.cpp), built once with
-fsanitize=thread and once with -fsanitize=address,undefined: every byte
copied at every thread count around the 4 MiB threshold and at the sizes where
the parts' rounding matters, nothing written outside the ranges, no data race,
no out-of-bounds access."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_sparse_matrix_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "xfer_host_test.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")

SANITIZERS = {
    "tsan": ("thread", "ThreadSanitizer", {"TSAN_OPTIONS": "halt_on_error=1 exitcode=66"}),
    "asan_ubsan": ("address,undefined", "Sanitizer",
                   {"ASAN_OPTIONS": "exitcode=66", "UBSAN_OPTIONS": "halt_on_error=1 print_stacktrace=1"}),
}


@pytest.mark.parametrize("name", sorted(SANITIZERS))
def test_xfer_host_helpers_under_sanitizer(name):
    flag, banner, san_env = SANITIZERS[name]
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "xfer_host_test_" + name)
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=" + flag, "-fno-sanitize-recover=undefined", "-pthread", "-I",
           CSRC, SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and any(w in r.stderr.lower() for w in ("tsan", "asan", "ubsan")):
        pytest.skip("no sanitizer runtime for -fsanitize=" + flag + ": " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, **san_env))
    assert banner not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " 0 failed" in r.stdout
