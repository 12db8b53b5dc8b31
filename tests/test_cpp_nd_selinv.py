"""bsm::NdFactor<T>::inv_diag / inv_entries of the C++ mirror (include/bsm.hpp),
driven by tests/cpp/test_nd_selinv.cpp: compiled against the header; on the
GPU, Poisson g = 11 under BSM_ND_LEAF=8 (several levels): the diagonal against
the solves with unit vectors, inv_entries' refusals and triangles, and the
printed diagonal against Python's NdFactor.inv_diag() bit for bit; without a
GPU, the constructor throws bsm::DeviceError (no CPU fallback). The build
recipe is test_cpp_nd_factor.py's."""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
ORC = os.path.join(ROOT, "oracle", "build")
SRC = os.path.join(ROOT, "tests", "cpp", "test_nd_selinv.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_nd_selinv")


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


def test_cpp_nd_selinv_no_cpu_fallback():
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    r = subprocess.run([_build(), "--expect-no-device"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_nd_selinv_on_gpu(monkeypatch):
    from basic_sparse_matrix_amd import Csr, cholesky_nd
    from oracle import pyoracle as orc

    monkeypatch.setenv("BSM_ND_LEAF", "8")
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=300, env=dict(os.environ))
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
