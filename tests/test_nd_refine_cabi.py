"""CPU checks of the mixed-precision additions to the C-ABI (include/bsm.h):
bsm_nd_factor_create_as, bsm_nd_factor_solve_refined and
bsm_dev_nd_factor_solve_refined are exported and bound, the API version stays 1
(they are additions), the header with them still compiles as C, null, bad-dtype
and bad-tol arguments are refused before any device is asked for and touch no
output, and the Python mirrors exist with their host-side checks."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bsm_nd_factor_create_as", "bsm_nd_factor_solve_refined", "bsm_dev_nd_factor_solve_refined"]


def test_refine_symbols_exported_and_bound():
    assert_exported_and_bound(NAMES)


def test_refine_bad_arguments_need_no_device():
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)  # never read: another argument is refused first
    addr = ctypes.cast(fake, ctypes.c_void_p)
    x = np.full(4, 7.0)
    berr = np.full(1, 7.0)
    iters = np.full(1, 7, dtype=np.uint32)
    cols = _lib.ptr_array([x])
    out = ctypes.c_void_p(12345)
    it, be, xp = _lib.ptr(iters), _lib.ptr(berr), _lib.ptr(x)
    nulls = (lib.bsm_nd_factor_create_as(None, _lib.BSM_F32, ctypes.byref(out)),
             lib.bsm_nd_factor_create_as(addr, _lib.BSM_F32, None),
             lib.bsm_nd_factor_solve_refined(None, addr, 1, 4, cols, cols, 5, 0.0, it, be),
             lib.bsm_nd_factor_solve_refined(addr, None, 1, 4, cols, cols, 5, 0.0, it, be),
             lib.bsm_dev_nd_factor_solve_refined(None, addr, 1, xp, xp, 5, 0.0, it, be, None),
             lib.bsm_dev_nd_factor_solve_refined(addr, None, 1, xp, xp, 5, 0.0, it, be, None))
    for rc in nulls:
        assert rc == _lib.BSM_ERR_INVALID
        assert "null" in _lib.last_error()
    for bad in (_lib.BSM_I32, _lib.BSM_U64, 6, -1, 99):  # a factor is f64 or f32
        assert lib.bsm_nd_factor_create_as(addr, bad, ctypes.byref(out)) == _lib.BSM_ERR_INVALID
        assert "factor_dtype" in _lib.last_error()
    for tol in (-1.0, -1e-300, float("nan"), float("-inf")):
        assert lib.bsm_nd_factor_solve_refined(addr, addr, 1, 4, cols, cols, 5, tol, it, be) == _lib.BSM_ERR_INVALID
        assert "tol" in _lib.last_error()
        assert lib.bsm_dev_nd_factor_solve_refined(addr, addr, 1, xp, xp, 5, tol, it, be, None) == _lib.BSM_ERR_INVALID
        assert "tol" in _lib.last_error()
    assert np.all(x == 7.0) and berr[0] == 7.0 and iters[0] == 7 and out.value == 12345


def test_python_mirrors_exist_and_check_on_the_host():
    import inspect

    from basic_sparse_matrix_amd import Csr, Dense, MatErr, NdFactor, RefineInfo, cholesky_nd, device

    assert hasattr(NdFactor, "solve_refined") and hasattr(device, "nd_factor_solve_refined")
    assert "factor_dtype" in inspect.signature(cholesky_nd).parameters
    assert [f for f in RefineInfo.__dataclass_fields__] == ["iters", "berr", "converged", "tol"]
    a = Csr.from_data([[4.0, 1.0], [1.0, 3.0]])
    b = Dense.from_columns([np.array([1.0, 2.0])])
    with pytest.raises(TypeError, match="factor_dtype"):
        cholesky_nd(a, factor_dtype=np.int32)
    f = NdFactor.__new__(NdFactor)  # a closed factor: the host-side checks come first
    f.handle, f.n, f.dtype = None, 2, np.dtype(np.float32)
    with pytest.raises(ValueError, match="after close"):
        f.solve_refined(a, b)
    with pytest.raises(ValueError, match="after close"):
        device.nd_factor_solve_refined(f, a, None)
    f.handle = 1  # never passed on: the arguments are refused first
    try:
        with pytest.raises(TypeError, match="dtype"):
            f.solve_refined(a, Dense.from_columns([np.array([1.0, 2.0], dtype=np.float32)]))
        with pytest.raises(TypeError):
            f.solve_refined(Csr.from_data([[4, 1], [1, 3]], dtype=np.int32), b)
        with pytest.raises(ValueError, match="max_iter"):
            f.solve_refined(a, b, max_iter=-1)
        for tol in (0.0, -1e-9, float("nan")):
            with pytest.raises(ValueError, match="tol"):
                f.solve_refined(a, b, tol=tol)
        with pytest.raises(MatErr):
            f.solve_refined(a, Dense.from_columns([np.array([1.0, 2.0, 3.0])]))
        with pytest.raises(MatErr):
            f.solve_refined(Csr.from_data([[4.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 0.0, 1.0]]), b)
    finally:
        f.handle = None  # nothing for close() to free


def test_default_tol_is_the_residuals_rounding_bound():
    from basic_sparse_matrix_amd import Csr
    from basic_sparse_matrix_amd.solver import refine_default_tol

    # lower triangle mirrored: rows of 2, 3, 2 entries, whatever lies above the diagonal
    a = Csr.from_data([[4.0, 9.0, 9.0], [1.0, 3.0, 0.0], [0.0, 1.0, 5.0]])
    assert refine_default_tol(a) == 5 * 2.0 ** -53


def test_header_with_refine_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    double x[2] = {7.0, 7.0}, berr[1] = {7.0};\n"
        "    uint32_t iters[1] = {7};\n"
        "    const void* bc[1];\n"
        "    void* xc[1];\n"
        "    int fake[1024] = {0};\n"
        "    const bsm_nd_factor* f = (const bsm_nd_factor*)fake; /* never read */\n"
        "    const bsm_csr* a = (const bsm_csr*)fake;\n"
        "    bsm_nd_factor* out = 0;\n"
        "    int (*mk)(const bsm_csr*, int, bsm_nd_factor**) = bsm_nd_factor_create_as;\n"
        "    int (*host)(const bsm_nd_factor*, const bsm_csr*, uint64_t, uint64_t, const void* const*, void* const*,\n"
        "                uint32_t, double, uint32_t*, double*) = bsm_nd_factor_solve_refined;\n"
        "    int (*dev)(const bsm_nd_factor*, const bsm_csr*, uint64_t, const void*, void*, uint32_t, double,\n"
        "               uint32_t*, double*, void*) = bsm_dev_nd_factor_solve_refined;\n"
        "    bc[0] = x; xc[0] = x;\n"
        "    if (mk(0, BSM_F32, &out) != BSM_ERR_INVALID) return 2;\n"
        "    if (mk(a, 17, &out) != BSM_ERR_INVALID) return 3;\n"
        "    if (host(0, a, 1, 2, bc, xc, 5, 0.0, iters, berr) != BSM_ERR_INVALID) return 4;\n"
        "    if (host(f, a, 1, 2, bc, xc, 5, -1.0, iters, berr) != BSM_ERR_INVALID) return 5;\n"
        "    if (dev(f, 0, 1, x, x, 5, 0.0, iters, berr, 0) != BSM_ERR_INVALID) return 6;\n"
        "    if (dev(f, a, 1, x, x, 5, -1.0, iters, berr, 0) != BSM_ERR_INVALID) return 7;\n"
        "    if (x[0] != 7.0 || x[1] != 7.0 || berr[0] != 7.0 || iters[0] != 7 || out != 0) return 8;\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "f.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile the refined solve's declarations of bsm.h as C"
    assert os.system(str(exe)) == 0
