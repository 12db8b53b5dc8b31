"""CPU checks of the selected inverse's C-ABI (include/bsm.h):
bsm_nd_factor_selinv and bsm_dev_nd_factor_inv_diag are exported and bound,
the API version stays 1 (they are additions), the header with them still
compiles as C, null arguments are refused before any device is asked for and
touch no output, and the Python methods exist with their host-side checks."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bsm_nd_factor_selinv", "bsm_dev_nd_factor_inv_diag"]


def test_selinv_symbols_exported_and_bound():
    assert_exported_and_bound(NAMES)


def test_selinv_null_arguments_need_no_device():
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)  # never read: another argument is refused first
    addr = ctypes.cast(fake, ctypes.c_void_p)
    diag, vals = np.full(4, 7.0), np.full(4, 7.0)
    idx = np.zeros(4, dtype=np.uint64)
    d, v, r = _lib.ptr(diag), _lib.ptr(vals), _lib.ptr(idx)
    for rc in (lib.bsm_nd_factor_selinv(None, d, 0, None, None, None),     # no handle
               lib.bsm_nd_factor_selinv(None, d, 4, r, r, v),
               lib.bsm_nd_factor_selinv(addr, None, 0, None, None, None),  # nothing asked for
               lib.bsm_nd_factor_selinv(addr, None, 0, r, r, v),
               lib.bsm_nd_factor_selinv(addr, d, 4, None, r, v),           # a null among rows / cols / vals
               lib.bsm_nd_factor_selinv(addr, d, 4, r, None, v),
               lib.bsm_nd_factor_selinv(addr, d, 4, r, r, None),
               lib.bsm_nd_factor_selinv(addr, None, 4, r, r, None),
               lib.bsm_dev_nd_factor_inv_diag(None, addr, None),
               lib.bsm_dev_nd_factor_inv_diag(None, None, None)):
        assert rc == _lib.BSM_ERR_INVALID
        assert "null" in _lib.last_error()
    assert np.all(diag == 7.0) and np.all(vals == 7.0) and np.all(idx == 0)


def test_python_mirrors_exist_and_check_on_the_host():
    from basic_sparse_matrix_amd import Csr, NdFactor, device

    for name in ("inv_diag", "inv_entries", "inv_on"):
        assert hasattr(NdFactor, name), name
    assert hasattr(device, "nd_factor_inv_diag")
    f = NdFactor.__new__(NdFactor)  # a closed factor: the host-side checks come first
    f.handle, f.n, f.dtype = None, 2, np.dtype(np.float64)
    with pytest.raises(ValueError, match="after close"):
        f.inv_diag()
    with pytest.raises(ValueError, match="after close"):
        f.inv_entries([0], [0])
    with pytest.raises(ValueError, match="after close"):
        f.inv_on(Csr.from_data([[4.0, 1.0], [1.0, 3.0]]))
    with pytest.raises(ValueError, match="after close"):
        device.nd_factor_inv_diag(f)
    f.handle = 1  # never passed on: the arguments are refused first
    try:
        with pytest.raises(ValueError, match="equal length"):
            f.inv_entries([0, 1], [0])
        with pytest.raises(ValueError, match="equal length"):
            f.inv_entries([[0]], [[0]])
        with pytest.raises(TypeError):
            f.inv_entries([0.5], [0.5])
        with pytest.raises(ValueError, match="negative"):
            f.inv_entries([-1], [0])
        from basic_sparse_matrix_amd import MatErr

        with pytest.raises(MatErr):
            f.inv_on(Csr.from_data([[4.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 0.0, 1.0]]))
    finally:
        f.handle = None  # nothing for close() to free


def test_header_with_selinv_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    double d[2] = {7.0, 7.0}, v[1] = {7.0};\n"
        "    uint64_t r[1] = {0};\n"
        "    int fake[64] = {0};\n"
        "    const bsm_nd_factor* f = (const bsm_nd_factor*)fake; /* never read */\n"
        "    int (*sel)(const bsm_nd_factor*, void*, uint64_t, const uint64_t*, const uint64_t*, void*) =\n"
        "        bsm_nd_factor_selinv;\n"
        "    int (*dev)(const bsm_nd_factor*, void*, void*) = bsm_dev_nd_factor_inv_diag;\n"
        "    if (sel(0, d, 0, 0, 0, 0) != BSM_ERR_INVALID) return 2;\n"
        "    if (sel(f, 0, 0, 0, 0, 0) != BSM_ERR_INVALID) return 3;\n"
        "    if (sel(f, d, 1, r, 0, v) != BSM_ERR_INVALID) return 4;\n"
        "    if (dev(0, d, 0) != BSM_ERR_INVALID) return 5;\n"
        "    if (d[0] != 7.0 || d[1] != 7.0 || v[0] != 7.0) return 6;\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "f.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile the selected inverse's declarations of bsm.h as C"
    assert os.system(str(exe)) == 0
