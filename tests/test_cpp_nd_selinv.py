"""bsm::NdFactor<T>::inv_diag / inv_entries of the C++ mirror (include/bsm.hpp),
driven by tests/cpp/test_nd_selinv.cpp: compiled against the header; on the
GPU, Poisson g = 11 under BSM_ND_LEAF=8 (several levels): the diagonal against
the solves with unit vectors, inv_entries' refusals and triangles, and the
printed diagonal against Python's NdFactor.inv_diag() bit for bit; without a
GPU, the constructor throws bsm::DeviceError (no CPU fallback)."""

import os
import subprocess

import numpy as np
import pytest

from cpp_support import build_mirror_program, expect_no_device

SRC = "test_nd_selinv.cpp"


def test_cpp_nd_selinv_no_cpu_fallback():
    expect_no_device(SRC)


@pytest.mark.gpu
def test_cpp_nd_selinv_on_gpu(monkeypatch):
    from basic_sparse_matrix_amd import Csr, cholesky_nd
    from oracle import pyoracle as orc

    monkeypatch.setenv("BSM_ND_LEAF", "8")
    r = subprocess.run([build_mirror_program(SRC)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("diag "):
            _, i, v = line.split()
            got[int(i)] = float.fromhex(v)
    g = 11
    rp, ci, v = orc.poisson2d(g)
    with cholesky_nd(Csr.from_csr_arrays((g * g, g * g), rp, ci, np.asarray(v, dtype=np.float64))) as f:
        want = f.inv_diag()
    assert sorted(got) == list(range(g * g))
    assert np.array_equal(np.array([got[i] for i in range(g * g)]).view(np.uint64), want.view(np.uint64))
