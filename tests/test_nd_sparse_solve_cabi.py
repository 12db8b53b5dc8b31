"""CPU checks of the kept factor's sparse solve C-ABI (include/bsm.h):
bsm_nd_factor_solve_sparse and bsm_dev_nd_factor_solve_sparse are exported and
bound, the API version stays 1 (an addition), the header with them still
compiles as C, the argument checks that come before any device is asked for
(null pointers, col_ptr and the rows' order, rows asked for without xrows, then
a row >= n) answer in that order and touch nothing, the no-ops need no device,
and the Python methods exist with their host-side checks."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bsm_nd_factor_solve_sparse", "bsm_dev_nd_factor_solve_sparse")


def test_sparse_solve_symbols_exported_and_bound():
    assert_exported_and_bound(NAMES)


def test_sparse_solve_argument_checks_need_no_device():
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)  # zeros: a handle of n == 0 whose other fields are never read
    addr = ctypes.cast(fake, ctypes.c_void_p)
    cp = np.array([0, 2], dtype=np.uint64)
    rows = np.array([0, 1], dtype=np.uint64)
    vals = np.array([1.0, -1.0])
    xr = np.array([3, 0], dtype=np.uint64)
    x0 = np.full(2, 7.0)
    xc = _lib.ptr_array([x0])
    info = np.full(4, 9, dtype=np.uint32)
    c, r, v, q, i = _lib.ptr(cp), _lib.ptr(rows), _lib.ptr(vals), _lib.ptr(xr), _lib.ptr(info)

    def host(f=addr, k=1, c=c, r=r, v=v, nq=2, q=q, x=xc, i=i):
        return lib.bsm_nd_factor_solve_sparse(f, k, c, r, v, nq, q, x, i)

    def dev(f=addr, k=1, c=c, r=r, v=v, nq=2, q=q, x=_lib.ptr(x0), i=i):
        return lib.bsm_dev_nd_factor_solve_sparse(f, k, c, r, v, nq, q, x, i, None)

    for call in (host, dev):
        # 1. null pointers
        for rc in (call(f=None), call(c=None), call(r=None), call(v=None), call(x=None)):
            assert rc == _lib.BSM_ERR_INVALID
            assert "null" in _lib.last_error()
        # 2. the order of col_ptr and of the rows
        for bad_rows in ([1, 0], [1, 1]):
            br = np.array(bad_rows, dtype=np.uint64)
            assert call(r=_lib.ptr(br)) == _lib.BSM_ERR_INVALID
            assert "strictly ascending" in _lib.last_error()
        assert call(c=_lib.ptr(np.array([1, 2], dtype=np.uint64))) == _lib.BSM_ERR_INVALID
        assert "col_ptr[0]" in _lib.last_error()
        two = {} if call is dev else {"x": _lib.ptr_array([x0, x0])}  # k = 2: two host columns
        assert call(k=2, c=_lib.ptr(np.array([0, 2, 1], dtype=np.uint64)), **two) == _lib.BSM_ERR_INVALID
        assert "not ascending" in _lib.last_error()
        # 3. rows asked for, and no way to tell which: before 4. a row >= n (every row is, with n == 0)
        assert call(q=None) == _lib.BSM_ERR_INVALID
        assert "xrows is null" in _lib.last_error()
        assert call() == _lib.BSM_ERR_OUT_OF_BOUNDS
        assert "entry 0 is row 0" in _lib.last_error()
        empty = np.zeros(2, dtype=np.uint64)
        assert call(c=_lib.ptr(empty), r=None, v=None) == _lib.BSM_ERR_OUT_OF_BOUNDS  # b is fine, xrows is not
        assert "requested row 0 is row 3" in _lib.last_error()
        # the no-ops: no columns (nothing at all is written); no rows asked for (info is cleared)
        assert call(k=0, c=None, r=None, v=None, nq=0, q=None, x=None) == _lib.BSM_OK
        assert np.array_equal(info, [9, 9, 9, 9])
        assert call(c=_lib.ptr(empty), r=None, v=None, nq=0, x=None) == _lib.BSM_OK  # xrows non-null, nq == 0
        assert np.array_equal(info, [0, 0, 0, 0])
        info[:] = 9
        assert call(c=_lib.ptr(empty), r=None, v=None, nq=0, q=None, x=None) == _lib.BSM_OK  # every row of n == 0
        info[:] = 9
    assert np.array_equal(cp, [0, 2]) and np.array_equal(rows, [0, 1]) and np.array_equal(vals, [1.0, -1.0])
    assert np.array_equal(x0, [7.0, 7.0]) and np.array_equal(xr, [3, 0])
    assert fake.raw == bytes(4096)


def test_python_mirrors_exist_and_check_on_the_host():
    from basic_sparse_matrix_amd import Csr, MatErr, MatErrKind, NdFactor, device

    for name in ("solve_sparse", "inv_block"):
        assert hasattr(NdFactor, name), name
    assert hasattr(device, "nd_factor_solve_sparse")
    assert "np.array_equal" in NdFactor.solve_sparse.__doc__  # the contract: equality, no tolerance
    f = NdFactor.__new__(NdFactor)  # a closed factor: the host-side checks come first
    f.handle, f.n, f.dtype, f.src_dtype = None, 2, np.dtype(np.float32), np.dtype(np.float64)
    b = Csr.from_data([[1.0], [-1.0]], dtype=np.float32)
    with pytest.raises(ValueError, match="after close"):
        f.solve_sparse(b)
    with pytest.raises(ValueError, match="after close"):
        f.inv_block([0], [1])
    f.handle = 1  # never passed on: the arguments are refused first
    try:
        with pytest.raises(MatErr) as e:
            f.solve_sparse(Csr.from_data([[1.0], [-1.0], [0.5]], dtype=np.float32))
        assert e.value.kind == MatErrKind.IncorrectDimensions
        with pytest.raises(TypeError, match="float32"):  # the FACTOR's dtype, not the factored matrix's
            f.solve_sparse(Csr.from_data([[1.0], [-1.0]]))
        with pytest.raises(ValueError, match="1-D"):
            f.solve_sparse(b, [[0, 1]])
        with pytest.raises(TypeError, match="integers"):
            f.solve_sparse(b, [0.5])
        with pytest.raises(ValueError, match="negative"):
            f.solve_sparse(b, [-1])
        with pytest.raises(ValueError, match="1-D"):
            f.inv_block(0, [1])
        with pytest.raises(TypeError, match="integers"):
            f.inv_block([0], [1.5])
        with pytest.raises(ValueError, match="negative"):
            f.inv_block([0], [-1])
        # nothing to compute: no device is asked for
        x = f.solve_sparse(b, [])
        assert (x.get_dims().rows, x.get_dims().cols) == (0, 1)
        assert f.inv_block([], [0, 1]).shape == (0, 2) and f.inv_block([0, 1, 1], []).shape == (3, 0)
    finally:
        f.handle = None  # nothing for close() to free


def test_header_with_sparse_solve_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    uint64_t cp[2] = {0, 1}, rows[1] = {0}, xr[1] = {0};\n"
        "    double v[1] = {7.0}, x[1] = {5.0};\n"
        "    void* xc[1] = {x};\n"
        "    uint32_t info[4] = {9, 9, 9, 9};\n"
        "    int (*hs)(const bsm_nd_factor*, uint64_t, const uint64_t*, const uint64_t*, const void*, uint64_t,\n"
        "              const uint64_t*, void* const*, uint32_t*) = bsm_nd_factor_solve_sparse;\n"
        "    int (*ds)(const bsm_nd_factor*, uint64_t, const uint64_t*, const uint64_t*, const void*, uint64_t,\n"
        "              const uint64_t*, void*, uint32_t*, void*) = bsm_dev_nd_factor_solve_sparse;\n"
        "    if (hs(0, 1, cp, rows, v, 1, xr, xc, info) != BSM_ERR_INVALID) return 2;\n"
        "    if (ds(0, 1, cp, rows, v, 1, xr, x, info, 0) != BSM_ERR_INVALID) return 3;\n"
        "    if (v[0] != 7.0 || x[0] != 5.0 || info[0] != 9) return 4;\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "f.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile the sparse solve's declarations of bsm.h as C"
    assert os.system(str(exe)) == 0
