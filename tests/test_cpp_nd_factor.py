"""bsm::NdFactor<T> of the C++ mirror (include/bsm.hpp), driven by
tests/cpp/test_nd_factor.cpp: on the GPU, the kept factor's solve against
bsm::solve_nd bit for bit (k = 2, Poisson g = 11) and the export's
conventions; without a GPU, the constructor throws bsm::DeviceError (no CPU
fallback)."""

import subprocess

import pytest

from cpp_support import build_mirror_program, expect_no_device

SRC = "test_nd_factor.cpp"


def test_cpp_nd_factor_no_cpu_fallback():
    expect_no_device(SRC)


@pytest.mark.gpu
def test_cpp_nd_factor_on_gpu():
    r = subprocess.run([build_mirror_program(SRC)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
