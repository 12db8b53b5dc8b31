"""bsm::NdFactor<T>::update / downdate of the C++ mirror (include/bsm.hpp),
driven by tests/cpp/test_nd_updown.cpp: compiled against the header; on the
GPU, Poisson g = 11 under BSM_ND_LEAF=8 (several levels): logdet after a
rank-2 update against log det(I + W^T S^-1 W), the downdate back, the
refusals, and the printed logdet against Python's NdFactor after the same
update bit for bit; without a GPU, the constructor throws bsm::DeviceError (no
CPU fallback). The build recipe is test_cpp_nd_factor.py's."""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
ORC = os.path.join(ROOT, "oracle", "build")
SRC = os.path.join(ROOT, "tests", "cpp", "test_nd_updown.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_nd_updown")


def _build():
    if not (os.path.exists(os.path.join(LIB, "libbsm_hip.so")) and os.path.exists(os.path.join(ORC, "libbsm_oracle.so"))):
        pytest.skip("libbsm_hip.so / libbsm_oracle.so not built (run __graft_entry__.build())")
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = [cxx, "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", LIB, "-lbsm_hip", "-L", ORC, "-lbsm_oracle", f"-Wl,-rpath,{LIB}", f"-Wl,-rpath,{ORC}",
           "-Wl,-rpath-link,/opt/rocm/lib", "-o", EXE]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return EXE


def test_cpp_nd_updown_no_cpu_fallback():
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    r = subprocess.run([_build(), "--expect-no-device"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_nd_updown_on_gpu(monkeypatch):
    from basic_sparse_matrix_amd import Csr, cholesky_nd
    from oracle import pyoracle as orc

    monkeypatch.setenv("BSM_ND_LEAF", "8")
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=300, env=dict(os.environ))
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
