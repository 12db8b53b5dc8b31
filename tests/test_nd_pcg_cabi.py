"""CPU checks of the pcg solve's additions to the C-ABI (include/bsm.h):
bsm_nd_factor_solve_pcg and bsm_dev_nd_factor_solve_pcg are exported and bound,
the API version stays 1 (they are additions), the header with them still
compiles as C, null and bad-tol arguments are refused before any device is
asked for and touch no output, and the Python mirrors exist with their
host-side checks."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bsm_nd_factor_solve_pcg", "bsm_dev_nd_factor_solve_pcg"]


def test_pcg_symbols_exported_and_bound():
    assert_exported_and_bound(NAMES)


def test_pcg_bad_arguments_need_no_device():
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)  # never read: another argument is refused first
    addr = ctypes.cast(fake, ctypes.c_void_p)
    x = np.full(4, 7.0)
    berr = np.full(1, 7.0)
    iters = np.full(1, 7, dtype=np.uint32)
    flags = np.full(1, 7, dtype=np.uint32)
    cols = _lib.ptr_array([x])
    it, be, fl, xp = _lib.ptr(iters), _lib.ptr(berr), _lib.ptr(flags), _lib.ptr(x)
    nulls = (lib.bsm_nd_factor_solve_pcg(None, addr, 1, 4, cols, cols, 50, 0.0, it, be, fl),
             lib.bsm_nd_factor_solve_pcg(addr, None, 1, 4, cols, cols, 50, 0.0, it, be, fl),
             lib.bsm_dev_nd_factor_solve_pcg(None, addr, 1, xp, xp, 50, 0.0, it, be, fl, None),
             lib.bsm_dev_nd_factor_solve_pcg(addr, None, 1, xp, xp, 50, 0.0, it, be, fl, None))
    for rc in nulls:
        assert rc == _lib.BSM_ERR_INVALID
        assert "null" in _lib.last_error()
    for tol in (-1.0, -1e-300, float("nan"), float("-inf")):
        assert lib.bsm_nd_factor_solve_pcg(addr, addr, 1, 4, cols, cols, 50, tol, it, be, fl) == _lib.BSM_ERR_INVALID
        assert "tol" in _lib.last_error()
        assert lib.bsm_dev_nd_factor_solve_pcg(addr, addr, 1, xp, xp, 50, tol, it, be, fl, None) == _lib.BSM_ERR_INVALID
        assert "tol" in _lib.last_error()
    assert np.all(x == 7.0) and berr[0] == 7.0 and iters[0] == 7 and flags[0] == 7


def test_python_mirrors_exist_and_check_on_the_host():
    import inspect

    import basic_sparse_matrix_amd as bsm
    from basic_sparse_matrix_amd import Csr, Dense, MatErr, NdFactor, PcgInfo, device

    assert "PcgInfo" in bsm.__all__
    assert [f for f in PcgInfo.__dataclass_fields__] == ["iters", "berr", "converged", "breakdown", "tol"]
    for fn in (NdFactor.solve_pcg, device.nd_factor_solve_pcg):
        p = inspect.signature(fn).parameters
        assert p["max_iter"].default == 50 and p["tol"].default is None
        assert p["max_iter"].kind == p["tol"].kind == inspect.Parameter.KEYWORD_ONLY
    a = Csr.from_data([[4.0, 1.0], [1.0, 3.0]])
    b = Dense.from_columns([np.array([1.0, 2.0])])
    f = NdFactor.__new__(NdFactor)  # a closed factor: the host-side checks come first
    f.handle, f.n, f.dtype = None, 2, np.dtype(np.float32)
    with pytest.raises(ValueError, match="after close"):
        f.solve_pcg(a, b)
    with pytest.raises(ValueError, match="after close"):
        device.nd_factor_solve_pcg(f, a, None)
    f.handle = 1  # never passed on: the arguments are refused first
    try:
        with pytest.raises(TypeError, match="dtype"):
            f.solve_pcg(a, Dense.from_columns([np.array([1.0, 2.0], dtype=np.float32)]))
        with pytest.raises(TypeError):
            f.solve_pcg(Csr.from_data([[4, 1], [1, 3]], dtype=np.int32), b)
        with pytest.raises(ValueError, match="max_iter"):
            f.solve_pcg(a, b, max_iter=-1)
        for tol in (0.0, -1e-9, float("nan")):
            with pytest.raises(ValueError, match="tol"):
                f.solve_pcg(a, b, tol=tol)
        with pytest.raises(MatErr):
            f.solve_pcg(a, Dense.from_columns([np.array([1.0, 2.0, 3.0])]))
        with pytest.raises(MatErr):
            f.solve_pcg(Csr.from_data([[4.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 0.0, 1.0]]), b)
    finally:
        f.handle = None  # nothing for close() to free


def test_header_with_pcg_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    double x[2] = {7.0, 7.0}, berr[1] = {7.0};\n"
        "    uint32_t iters[1] = {7}, flags[1] = {7};\n"
        "    const void* bc[1];\n"
        "    void* xc[1];\n"
        "    int fake[1024] = {0};\n"
        "    const bsm_nd_factor* f = (const bsm_nd_factor*)fake; /* never read */\n"
        "    const bsm_csr* a = (const bsm_csr*)fake;\n"
        "    int (*host)(const bsm_nd_factor*, const bsm_csr*, uint64_t, uint64_t, const void* const*, void* const*,\n"
        "                uint32_t, double, uint32_t*, double*, uint32_t*) = bsm_nd_factor_solve_pcg;\n"
        "    int (*dev)(const bsm_nd_factor*, const bsm_csr*, uint64_t, const void*, void*, uint32_t, double,\n"
        "               uint32_t*, double*, uint32_t*, void*) = bsm_dev_nd_factor_solve_pcg;\n"
        "    bc[0] = x; xc[0] = x;\n"
        "    if (host(0, a, 1, 2, bc, xc, 50, 0.0, iters, berr, flags) != BSM_ERR_INVALID) return 4;\n"
        "    if (host(f, a, 1, 2, bc, xc, 50, -1.0, iters, berr, flags) != BSM_ERR_INVALID) return 5;\n"
        "    if (dev(f, 0, 1, x, x, 50, 0.0, iters, berr, flags, 0) != BSM_ERR_INVALID) return 6;\n"
        "    if (dev(f, a, 1, x, x, 50, -1.0, iters, berr, 0, 0) != BSM_ERR_INVALID) return 7;\n"
        "    if (x[0] != 7.0 || x[1] != 7.0 || berr[0] != 7.0 || iters[0] != 7 || flags[0] != 7) return 8;\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "f.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile the pcg solve's declarations of bsm.h as C"
    assert os.system(str(exe)) == 0
