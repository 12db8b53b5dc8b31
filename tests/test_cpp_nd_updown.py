"""bsm::NdFactor<T>::update / downdate of the C++ mirror (include/bsm.hpp),
driven by tests/cpp/test_nd_updown.cpp: compiled against the header; on the
GPU, Poisson g = 11 under BSM_ND_LEAF=8 (several levels): logdet after a
rank-2 update against log det(I + W^T S^-1 W), the downdate back, the
refusals, and the printed logdet against Python's NdFactor after the same
update bit for bit; without a GPU, the constructor throws bsm::DeviceError (no
CPU fallback)."""

import os
import subprocess

import numpy as np
import pytest

from cpp_support import build_mirror_program, expect_no_device

SRC = "test_nd_updown.cpp"


def test_cpp_nd_updown_no_cpu_fallback():
    expect_no_device(SRC)


@pytest.mark.gpu
def test_cpp_nd_updown_on_gpu(monkeypatch):
    from basic_sparse_matrix_amd import Csr, cholesky_nd
    from oracle import pyoracle as orc

    monkeypatch.setenv("BSM_ND_LEAF", "8")
    r = subprocess.run([build_mirror_program(SRC)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
    got = u = t = None
    for line in r.stdout.splitlines():
        if line.startswith("logdet "):
            got = float.fromhex(line.split()[1])
        if line.startswith("perm0 "):
            f = line.split()
            u, t = int(f[3]), int(f[5])
    g = 11
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    with cholesky_nd(Csr.from_csr_arrays((n, n), rp, ci, np.asarray(v, dtype=np.float64))) as f:
        w = np.zeros((n, 2))
        w[f.perm[0], 0] = 0.5
        w[u, 1], w[t, 1] = np.sqrt(0.75), -np.sqrt(0.75)
        nzr, nzc = np.nonzero(w)
        wrp = np.concatenate([[0], np.cumsum(np.bincount(nzr, minlength=n))]).astype(np.uint64)
        f.update(Csr.from_csr_arrays((n, 2), wrp, nzc.astype(np.uint64), w[nzr, nzc]))
        want = f.logdet()
    assert np.array([got]).view(np.uint64)[0] == np.array([want]).view(np.uint64)[0]
