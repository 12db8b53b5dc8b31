"""bsm::NdFactor<T>::refactor / logdet / solve(b, NdSystem) of the C++ mirror
(include/bsm.hpp), driven by tests/cpp/test_nd_factor_ops.cpp: on the GPU,
Poisson g = 11: refactor against a fresh factor bit for bit, logdet against
the host sum over l(), L then L^T around the permutation against solve;
without a GPU, the constructor throws bsm::DeviceError (no CPU fallback)."""

import subprocess

import pytest

from cpp_support import build_mirror_program, expect_no_device

SRC = "test_nd_factor_ops.cpp"


def test_cpp_nd_factor_ops_no_cpu_fallback():
    expect_no_device(SRC)


@pytest.mark.gpu
def test_cpp_nd_factor_ops_on_gpu():
    r = subprocess.run([build_mirror_program(SRC)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
