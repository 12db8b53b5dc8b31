"""Building and running the stand-alone C++ programs under tests/cpp: the
drivers of the C++ mirror (include/bsm.hpp), linked against libbsm_hip.so and
the oracle, and the CPU-only rule programs, built with
-fsanitize=address,undefined. Each test file keeps what it does with its
program's output."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
ORC = os.path.join(ROOT, "oracle", "build")
CSRC = os.path.join(ROOT, "basic_sparse_matrix_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
BUILD = os.path.join(CPP, "build")


def build_mirror_program(src_name):
    """Compile tests/cpp/<src_name> against the mirror's header and both libraries; the executable's path."""
    libs = (os.path.join(LIB, "libbsm_hip.so"), os.path.join(ORC, "libbsm_oracle.so"))
    if not all(os.path.exists(p) for p in libs):
        pytest.skip("libbsm_hip.so / libbsm_oracle.so not built (run __graft_entry__.build())")
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, os.path.splitext(src_name)[0])
    cmd = [cxx, "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(CPP, src_name), "-L", LIB, "-lbsm_hip", "-L", ORC, "-lbsm_oracle", f"-Wl,-rpath,{LIB}",
           f"-Wl,-rpath,{ORC}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def expect_no_device(src_name):
    """Without a GPU the program's hot-path calls throw bsm::DeviceError: there is no CPU fallback."""
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    r = subprocess.run([build_mirror_program(src_name), "--expect-no-device"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def run_sanitized(src_name, include_dir=CSRC, extra_flags=()):
    """Compile tests/cpp/<src_name>, a CPU program with its own main, with -fsanitize=address,undefined and run it: no
    sanitizer report, exit status 0, and no failed check."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, os.path.splitext(src_name)[0] + "_asan_ubsan")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra_flags, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", include_dir, os.path.join(CPP, src_name), "-o", exe]
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
