"""bsm::NdFactor<T>::refactor_partial / refactor_since of the C++ mirror
(include/bsm.hpp), driven by tests/cpp/test_nd_partial.cpp: compiled against
the header; on the GPU, Poisson g = 11 under BSM_ND_LEAF=8 (several levels):
named places and places found from the old matrix, each time L, a solve,
logdet and inv_diag equal to a fresh factor's entry for entry, the front
counts, the refusals; without a GPU, the constructor throws bsm::DeviceError
(no CPU fallback). The build recipe is test_cpp_nd_factor.py's."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
ORC = os.path.join(ROOT, "oracle", "build")
SRC = os.path.join(ROOT, "tests", "cpp", "test_nd_partial.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_nd_partial")


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


def test_cpp_nd_partial_no_cpu_fallback():
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    r = subprocess.run([_build(), "--expect-no-device"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_nd_partial_on_gpu(monkeypatch):
    monkeypatch.setenv("BSM_ND_LEAF", "8")
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
