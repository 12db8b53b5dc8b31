"""bsm::NdFactor<T>::refactor_partial / refactor_since of the C++ mirror
(include/bsm.hpp), driven by tests/cpp/test_nd_partial.cpp: compiled against
the header; on the GPU, Poisson g = 11 under BSM_ND_LEAF=8 (several levels):
named places and places found from the old matrix, each time L, a solve,
logdet and inv_diag equal to a fresh factor's entry for entry, the front
counts, the refusals; without a GPU, the constructor throws bsm::DeviceError
(no CPU fallback)."""

import os
import subprocess

import pytest

from cpp_support import build_mirror_program, expect_no_device

SRC = "test_nd_partial.cpp"


def test_cpp_nd_partial_no_cpu_fallback():
    expect_no_device(SRC)


@pytest.mark.gpu
def test_cpp_nd_partial_on_gpu(monkeypatch):
    monkeypatch.setenv("BSM_ND_LEAF", "8")
    r = subprocess.run([build_mirror_program(SRC)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
