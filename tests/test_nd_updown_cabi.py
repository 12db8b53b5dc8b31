"""CPU checks of the kept factor's update / downdate C-ABI (include/bsm.h):
bsm_nd_factor_updown is exported and bound, the API version stays 1 (an
addition), the header with it still compiles as C, the argument checks that
come before any device is asked for (null pointers, the sign, col_ptr and the
rows' order, then k > 16, then a row >= n) answer in that order and touch
nothing, and the Python methods exist with their host-side checks."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_updown_symbol_exported_and_bound():
    assert_exported_and_bound(["bsm_nd_factor_updown"])


def test_updown_argument_checks_need_no_device():
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)  # zeros: a handle of n == 0 whose other fields are never read
    addr = ctypes.cast(fake, ctypes.c_void_p)
    up = lib.bsm_nd_factor_updown
    cp = np.array([0, 2], dtype=np.uint64)
    rows = np.array([0, 1], dtype=np.uint64)
    vals = np.array([1.0, -1.0])
    c, r, v = _lib.ptr(cp), _lib.ptr(rows), _lib.ptr(vals)
    # 1. null pointers, the sign, the order of col_ptr and of the rows
    for rc in (up(None, 1, 1, c, r, v), up(addr, 1, 1, None, r, v), up(addr, 1, 1, c, None, v),
               up(addr, 1, 1, c, r, None)):
        assert rc == _lib.BSM_ERR_INVALID
        assert "null" in _lib.last_error()
    for sign in (0, 2, -2):
        assert up(addr, sign, 1, c, r, v) == _lib.BSM_ERR_INVALID
        assert "sign" in _lib.last_error()
    for bad_rows in ([1, 0], [1, 1]):
        br = np.array(bad_rows, dtype=np.uint64)
        assert up(addr, 1, 1, c, _lib.ptr(br), v) == _lib.BSM_ERR_INVALID
        assert "strictly ascending" in _lib.last_error()
    assert up(addr, 1, 1, _lib.ptr(np.array([1, 2], dtype=np.uint64)), r, v) == _lib.BSM_ERR_INVALID
    assert "col_ptr[0]" in _lib.last_error()
    assert up(addr, 1, 2, _lib.ptr(np.array([0, 2, 1], dtype=np.uint64)), r, v) == _lib.BSM_ERR_INVALID
    assert "not ascending" in _lib.last_error()
    # ... which come before k > 16, also with 17 columns
    cp17 = np.zeros(18, dtype=np.uint64)
    assert up(addr, 0, 17, _lib.ptr(cp17), None, None) == _lib.BSM_ERR_INVALID
    # 2. k > 16, before 3. a row >= n (every row is, with n == 0)
    cp17[1:] = 1
    assert up(addr, -1, 17, _lib.ptr(cp17), r, v) == _lib.BSM_ERR_UNSUPPORTED
    assert "at most 16" in _lib.last_error()
    assert up(addr, 1, 1, c, r, v) == _lib.BSM_ERR_OUT_OF_BOUNDS
    assert "row 0" in _lib.last_error()
    assert np.array_equal(cp, [0, 2]) and np.array_equal(rows, [0, 1]) and np.array_equal(vals, [1.0, -1.0])
    assert fake.raw == bytes(4096)


def test_python_mirrors_exist_and_check_on_the_host():
    from basic_sparse_matrix_amd import Csr, MatErr, MatErrKind, NdFactor

    for name in ("update", "downdate"):
        assert hasattr(NdFactor, name), name
    assert "later in the new order" in " ".join(NdFactor.update.__doc__.lower().split())  # which columns are inside
    f = NdFactor.__new__(NdFactor)  # a closed factor: the host-side checks come first
    f.handle, f.n, f.dtype, f.src_dtype = None, 2, np.dtype(np.float32), np.dtype(np.float64)
    w = Csr.from_data([[1.0], [-1.0]])
    with pytest.raises(ValueError, match="after close"):
        f.update(w)
    with pytest.raises(ValueError, match="after close"):
        f.downdate(w)
    f.handle = 1  # never passed on: the arguments are refused first
    try:
        with pytest.raises(MatErr) as e:
            f.update(Csr.from_data([[1.0], [-1.0], [0.5]]))
        assert e.value.kind == MatErrKind.IncorrectDimensions
        with pytest.raises(TypeError, match="float64"):  # the factored matrix's dtype, not the factor's
            f.downdate(Csr.from_csr_arrays((2, 1), np.array([0, 1, 2], dtype=np.uint64), np.zeros(2, dtype=np.uint64),
                                           np.array([1.0, -1.0], dtype=np.float32)))
    finally:
        f.handle = None  # nothing for close() to free


def test_header_with_updown_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    uint64_t cp[2] = {0, 1}, rows[1] = {0};\n"
        "    double v[1] = {7.0};\n"
        "    int (*ud)(bsm_nd_factor*, int, uint64_t, const uint64_t*, const uint64_t*, const void*) =\n"
        "        bsm_nd_factor_updown;\n"
        "    if (ud(0, 1, 1, cp, rows, v) != BSM_ERR_INVALID) return 2;\n"
        "    if (ud(0, -1, 0, 0, 0, 0) != BSM_ERR_INVALID) return 3;\n"
        "    if (v[0] != 7.0 || cp[1] != 1) return 4;\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "f.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile the update's declaration of bsm.h as C"
    assert os.system(str(exe)) == 0
