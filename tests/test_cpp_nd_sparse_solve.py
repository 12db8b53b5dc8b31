"""bsm::NdFactor<T>::solve_sparse / inv_block of the C++ mirror
(include/bsm.hpp), driven by tests/cpp/test_nd_sparse_solve.cpp: compiled
against the header; on the GPU, Poisson g = 11 under BSM_ND_LEAF=8 (several
levels): a sparse b at a few rows and at every row against the dense solve
entry for entry, inv_block against the solves of unit columns, the counts of
visited fronts, the refusals; without a GPU, the constructor throws
bsm::DeviceError (no CPU fallback)."""

import os
import subprocess

import pytest

from cpp_support import build_mirror_program, expect_no_device

SRC = "test_nd_sparse_solve.cpp"


def test_cpp_nd_sparse_solve_no_cpu_fallback():
    expect_no_device(SRC)


@pytest.mark.gpu
def test_cpp_nd_sparse_solve_on_gpu(monkeypatch):
    monkeypatch.setenv("BSM_ND_LEAF", "8")
    r = subprocess.run([build_mirror_program(SRC)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
