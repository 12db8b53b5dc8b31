"""bsm::NdFactor<F>::solve_pcg of the C++ mirror (include/bsm.hpp), driven by
tests/cpp/test_nd_pcg.cpp: compiled against the header; on the GPU, Poisson
g = 11 under BSM_ND_LEAF=8, A / 2 on the f32 factor of A, and the printed x,
iters, berr and breakdown against Python's NdFactor.solve_pcg bit for bit;
without a GPU, the factorisation throws bsm::DeviceError (no CPU fallback)."""

import os
import subprocess

import numpy as np
import pytest

from cpp_support import build_mirror_program, expect_no_device

SRC = "test_nd_pcg.cpp"


def test_cpp_nd_pcg_no_cpu_fallback():
    expect_no_device(SRC)


@pytest.mark.gpu
def test_cpp_nd_pcg_on_gpu(monkeypatch):
    from basic_sparse_matrix_amd import Csr, Dense, cholesky_nd
    from oracle import pyoracle as orc

    monkeypatch.setenv("BSM_ND_LEAF", "8")
    r = subprocess.run([build_mirror_program(SRC)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
    g = 11
    n = g * g
    got = np.zeros((2, n))
    seen = 0
    info = {}
    for line in r.stdout.splitlines():
        if line.startswith("x "):
            _, j, i, v = line.split()
            got[int(j), int(i)] = float.fromhex(v)
            seen += 1
        elif line.startswith("info "):
            _, j, it, be, bd = line.split()
            info[int(j)] = (int(it), float.fromhex(be), int(bd))
    assert seen == 2 * n and sorted(info) == [0, 1]
    i = np.arange(n)
    cols = [1.0 + (i % 7) * 0.125, ((i * 37) % 11) - 5.0]  # the program's right-hand sides
    rp, ci, v = orc.poisson2d(g)
    v = np.asarray(v, dtype=np.float64)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    half = Csr.from_csr_arrays((n, n), rp, ci, 0.5 * v)
    with cholesky_nd(A, factor_dtype=np.float32) as f:
        x, want = f.solve_pcg(half, Dense.from_columns([np.asarray(c, dtype=np.float64) for c in cols]))
    for j in range(2):
        assert np.array_equal(got[j].view(np.uint64), np.asarray(x.get_col(j)).view(np.uint64)), j
        assert info[j][0] == want.iters[j] and info[j][2] == int(want.breakdown[j])
        assert np.float64(info[j][1]).view(np.uint64) == want.berr[j].view(np.uint64)
