"""The C++ host mirror (include/bsm.hpp) -- the reference is compiled Rust, so
its API is mirrored in C++ above the C-ABI -- driven by tests/cpp/test_mirror.cpp:
the reference's own unit tests restated in C++ plus seeded parity against the
C oracle. CPU: build, host-logic tests, and "no CPU fallback" (every hot-path
call raises bsm::DeviceError without a GPU). GPU: the whole program."""

import subprocess

import pytest

from cpp_support import build_mirror_program, expect_no_device

SRC = "test_mirror.cpp"


def _run(*args, timeout=300):
    return subprocess.run([build_mirror_program(SRC), *args], capture_output=True, text=True, timeout=timeout)


def test_cpp_mirror_host_logic():
    r = _run("--host")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout


def test_cpp_mirror_no_cpu_fallback():
    """Without a GPU every hot-path call of the mirror throws DeviceError."""
    expect_no_device(SRC)


@pytest.mark.gpu
def test_cpp_mirror_on_gpu():
    r = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
