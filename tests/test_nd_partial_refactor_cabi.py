"""CPU checks of the partial refactor's C-ABI (include/bsm.h):
bsm_nd_factor_refactor_partial and bsm_nd_factor_refactor_since are exported
and bound, the API version stays 1 (an addition), the header with them still
compiles as C, the argument checks that come before any device is asked for (a
null f or a, then nc > 0 with a null list) answer in that order on a zeroed
fake handle and touch nothing, and the Python method exists with its host-side
checks."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bsm_nd_factor_refactor_partial", "bsm_nd_factor_refactor_since")


def test_partial_refactor_symbols_exported_and_bound():
    assert_exported_and_bound(NAMES)


def test_partial_refactor_argument_checks_need_no_device():
    lib = _lib.load()
    fake_f = ctypes.create_string_buffer(4096)  # zeros: never read by these checks
    fake_a = ctypes.create_string_buffer(4096)
    f, a = ctypes.cast(fake_f, ctypes.c_void_p), ctypes.cast(fake_a, ctypes.c_void_p)
    rows = np.array([1, 0], dtype=np.uint64)
    cols = np.array([0, 0], dtype=np.uint64)
    info = np.full(3, 9, dtype=np.uint64)
    r, c, i = _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(info)
    part, since = lib.bsm_nd_factor_refactor_partial, lib.bsm_nd_factor_refactor_since
    # 1. a null f or a, whatever else is wrong
    for rc in (part(None, a, 2, r, c, i), part(f, None, 2, r, c, i), part(None, None, 2, None, None, i),
               part(f, None, 2, None, c, i), since(None, a, a, i), since(f, None, a, i), since(f, a, None, i)):
        assert rc == _lib.BSM_ERR_INVALID
        assert _lib.last_error() == "null argument"
    # 2. pairs named, and no list of them
    for rc in (part(f, a, 2, None, c, i), part(f, a, 2, r, None, i), part(f, a, 1, None, None, None)):
        assert rc == _lib.BSM_ERR_INVALID
        assert "rows or cols is null" in _lib.last_error()
    assert np.array_equal(info, [9, 9, 9]) and np.array_equal(rows, [1, 0]) and np.array_equal(cols, [0, 0])
    assert fake_f.raw == bytes(4096) and fake_a.raw == bytes(4096)


def test_python_method_exists_and_checks_on_the_host():
    from basic_sparse_matrix_amd import Csr, NdFactor, PartialInfo, Panic

    assert hasattr(NdFactor, "refactor_partial")
    assert "refactor(a)" in NdFactor.refactor_partial.__doc__  # the contract: refactor's bits
    assert PartialInfo(1, 2, 3) == PartialInfo(fronts=1, total_fronts=2, changed=3)
    f = NdFactor.__new__(NdFactor)  # a closed factor: the host-side checks come first
    f.handle, f.n, f.dtype, f.src_dtype = None, 2, np.dtype(np.float64), np.dtype(np.float64)
    a = Csr.from_data([[2.0, -1.0], [-1.0, 2.0]], dtype=np.float64)
    with pytest.raises(ValueError, match="exactly one"):
        f.refactor_partial(a)
    with pytest.raises(ValueError, match="exactly one"):
        f.refactor_partial(a, [0], [0], since=a)
    with pytest.raises(ValueError, match="exactly one"):
        f.refactor_partial(a, [0], since=a)
    with pytest.raises(TypeError, match="f32"):
        f.refactor_partial(Csr.from_data([[2, -1], [-1, 2]], dtype=np.int32), [0], [0])
    with pytest.raises(Panic, match="NonSquareMatrix"):
        f.refactor_partial(Csr.from_data([[2.0, -1.0]], dtype=np.float64), [0], [0])
    with pytest.raises(ValueError, match="after close"):
        f.refactor_partial(a, [0], [0])
    f.handle = 1  # never passed on: the arguments are refused first
    try:
        with pytest.raises(ValueError, match="go together"):
            f.refactor_partial(a, [0])
        with pytest.raises(ValueError, match="go together"):
            f.refactor_partial(a, cols=[0])
        with pytest.raises(ValueError, match="rows has 2 entries, cols 1"):
            f.refactor_partial(a, [0, 1], [0])
        with pytest.raises(ValueError, match="1-D"):
            f.refactor_partial(a, [[0, 1]], [0, 1])
        with pytest.raises(TypeError, match="integers"):
            f.refactor_partial(a, [0.5], [0])
        with pytest.raises(TypeError, match="integers"):
            f.refactor_partial(a, [0], [1.5])
        with pytest.raises(ValueError, match="negative"):
            f.refactor_partial(a, [0], [-1])
        with pytest.raises(TypeError, match="since must be a Csr"):
            f.refactor_partial(a, since=np.eye(2))
        with pytest.raises(TypeError, match="since is Csr<float32>"):
            f.refactor_partial(a, since=Csr.from_data([[2.0, -1.0], [-1.0, 2.0]], dtype=np.float32))
    finally:
        f.handle = None  # nothing for close() to free


def test_header_with_partial_refactor_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    uint64_t rows[1] = {0}, cols[1] = {0}, info[3] = {9, 9, 9};\n"
        "    int (*pp)(bsm_nd_factor*, const bsm_csr*, uint64_t, const uint64_t*, const uint64_t*, uint64_t*) =\n"
        "        bsm_nd_factor_refactor_partial;\n"
        "    int (*ps)(bsm_nd_factor*, const bsm_csr*, const bsm_csr*, uint64_t*) = bsm_nd_factor_refactor_since;\n"
        "    if (pp(0, 0, 1, rows, cols, info) != BSM_ERR_INVALID) return 2;\n"
        "    if (ps(0, 0, 0, info) != BSM_ERR_INVALID) return 3;\n"
        "    if (info[0] != 9 || info[2] != 9) return 4;\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "f.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile the partial refactor's declarations of bsm.h as C"
    assert os.system(str(exe)) == 0
