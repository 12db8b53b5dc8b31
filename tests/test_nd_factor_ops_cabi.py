"""CPU checks of the kept nd factor's later C-ABI (include/bsm.h):
bsm_nd_factor_refactor, bsm_nd_factor_logdet, bsm_nd_factor_solve_system and
bsm_dev_nd_factor_solve are exported and bound, the API version stays 1 (they
are additions), the header with them and BSM_ND_SYS_* still compiles as C, and
null arguments are refused before any device is asked for."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bsm_nd_factor_refactor", "bsm_nd_factor_logdet", "bsm_nd_factor_solve_system", "bsm_dev_nd_factor_solve"]


def test_ops_symbols_exported_and_bound():
    assert_exported_and_bound(NAMES)


def test_ops_null_arguments_need_no_device():
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)  # never read: the other argument is refused first
    addr = ctypes.cast(fake, ctypes.c_void_p)
    v = ctypes.c_double(7.0)
    cols = _lib.ptr_array([np.zeros(1)])
    for rc in (lib.bsm_nd_factor_refactor(None, addr), lib.bsm_nd_factor_refactor(None, None),
               lib.bsm_nd_factor_logdet(None, ctypes.byref(v)), lib.bsm_nd_factor_logdet(None, None),
               lib.bsm_nd_factor_solve_system(None, 0, 1, 1, cols, cols),
               lib.bsm_nd_factor_solve_system(None, 1, 0, 0, None, None),
               lib.bsm_dev_nd_factor_solve(None, 0, 1, addr, addr, None)):
        assert rc == _lib.BSM_ERR_INVALID
        assert "null" in _lib.last_error()
    assert v.value == 7.0


def test_python_mirrors_exist_and_check_on_the_host():
    from basic_sparse_matrix_amd import Csr, NdFactor
    from basic_sparse_matrix_amd import solver

    for name in ("refactor", "logdet"):
        assert hasattr(NdFactor, name), name
    assert solver.ND_SYSTEMS == {"A": 0, "L": 1, "Lt": 2}
    with pytest.raises(ValueError):
        solver.nd_system_code("Q")
    f = NdFactor.__new__(NdFactor)  # a closed factor: the host-side checks come first
    f.handle, f.n, f.dtype = None, 2, np.dtype(np.float64)
    with pytest.raises(TypeError):
        f.refactor(Csr.from_data([[1, 0], [0, 1]], dtype=np.int32))
    with pytest.raises(ValueError):
        f.refactor(Csr.from_data([[4.0, 1.0], [1.0, 3.0]]))
    with pytest.raises(ValueError):
        f.logdet()


def test_header_with_ops_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    double ld = 7.0;\n"
        "    int systems[3] = {BSM_ND_SYS_A, BSM_ND_SYS_L, BSM_ND_SYS_LT};\n"
        "    int (*refactor)(bsm_nd_factor*, const bsm_csr*) = bsm_nd_factor_refactor;\n"
        "    int (*logdet)(const bsm_nd_factor*, double*) = bsm_nd_factor_logdet;\n"
        "    int (*sys)(const bsm_nd_factor*, int, uint64_t, uint64_t, const void* const*, void* const*) =\n"
        "        bsm_nd_factor_solve_system;\n"
        "    int (*dev)(const bsm_nd_factor*, int, uint64_t, const void*, void*, void*) = bsm_dev_nd_factor_solve;\n"
        "    if (systems[0] != 0 || systems[1] != 1 || systems[2] != 2) return 2;\n"
        "    if (refactor(0, 0) != BSM_ERR_INVALID) return 3;\n"
        "    if (logdet(0, &ld) != BSM_ERR_INVALID || ld != 7.0) return 4;\n"
        "    if (sys(0, BSM_ND_SYS_L, 0, 0, 0, 0) != BSM_ERR_INVALID) return 5;\n"
        "    if (dev(0, BSM_ND_SYS_LT, 0, 0, 0, 0) != BSM_ERR_INVALID) return 6;\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "f.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile the factor's declarations of bsm.h as C"
    assert os.system(str(exe)) == 0
