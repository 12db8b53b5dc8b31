"""bsm::cholesky_nd_schur and NdFactor<T>::schur / schur_condense /
schur_expand / schur_index of the C++ mirror (include/bsm.hpp), driven by
tests/cpp/nd_schur.cpp: compiled against the header; on the GPU, Poisson
g = 11 under BSM_ND_LEAF=8 with the middle grid line as the set; without a
GPU, the constructor throws bsm::DeviceError (no CPU fallback)."""

import os
import subprocess

import pytest

from cpp_support import build_mirror_program, expect_no_device

SRC = "nd_schur.cpp"


def test_cpp_nd_schur_no_cpu_fallback():
    expect_no_device(SRC)


@pytest.mark.gpu
def test_cpp_nd_schur_on_gpu(monkeypatch):
    monkeypatch.setenv("BSM_ND_LEAF", "8")
    r = subprocess.run([build_mirror_program(SRC)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
