"""bsm::NdFactor<F>::eigsh_gen of the C++ mirror (include/bsm.hpp), driven by
tests/cpp/test_nd_eig_gen.cpp: compiled against the header; on the GPU, Poisson
g = 11 with its consistent mass matrix under BSM_ND_LEAF=8 on the f32 factor,
nev = 6, block = 4, ncv = 60, and the printed lam, resid, vectors and info
against Python's NdFactor.eigsh(m=...) bit for bit; without a GPU, the argument
errors of the two C entry points are reported as on the GPU (they need no
device) and the factorisation throws bsm::DeviceError (no CPU fallback)."""

import os
import subprocess

import numpy as np
import pytest

from cpp_support import build_mirror_program, expect_no_device

SRC = "test_nd_eig_gen.cpp"


def test_cpp_nd_eig_gen_argument_errors_and_no_cpu_fallback():
    expect_no_device(SRC)


@pytest.mark.gpu
def test_cpp_nd_eig_gen_on_gpu(monkeypatch):
    from basic_sparse_matrix_amd import Csr, cholesky_nd
    from oracle import pyoracle as orc

    monkeypatch.setenv("BSM_ND_LEAF", "8")
    r = subprocess.run([build_mirror_program(SRC)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
    g, nev = 11, 6
    n = g * g
    got = np.zeros((nev, n))
    seen = 0
    pairs = {}
    info = None
    for line in r.stdout.splitlines():
        if line.startswith("y "):
            _, j, i, v = line.split()
            got[int(j), int(i)] = float.fromhex(v)
            seen += 1
        elif line.startswith("pair "):
            _, j, lam, res = line.split()
            pairs[int(j)] = (float.fromhex(lam), float.fromhex(res))
        elif line.startswith("info "):
            info = [int(t) for t in line.split()[1:]]
    assert seen == nev * n and sorted(pairs) == list(range(nev)) and info is not None
    rp, ci, v = orc.poisson2d(g)
    A = Csr.from_csr_arrays((n, n), rp, ci, np.asarray(v, dtype=np.float64))
    m1 = (np.diag(np.full(g, 4.0)) + np.diag(np.ones(g - 1), 1) + np.diag(np.ones(g - 1), -1)) / 6.0
    md = np.kron(m1, m1)
    nzr, nzc = np.nonzero(md)
    mrp = np.concatenate([[0], np.cumsum(np.bincount(nzr, minlength=n))]).astype(np.uint64)
    M = Csr.from_csr_arrays((n, n), mrp, nzc.astype(np.uint64), md[nzr, nzc])
    with cholesky_nd(A, factor_dtype=np.float32) as f:
        lam, y, want = f.eigsh(A, nev, block=4, ncv=60, m=M)
    assert info == [want.steps, want.ncv_used, int(want.converged.sum()), int(want.exhausted), int(want.inexact)]
    for j in range(nev):
        assert np.array_equal(got[j].view(np.uint64), np.asarray(y.get_col(j)).view(np.uint64)), j
        assert np.float64(pairs[j][0]).view(np.uint64) == lam[j].view(np.uint64)
        assert np.float64(pairs[j][1]).view(np.uint64) == want.resid[j].view(np.uint64)
