"""CPU checks of the kept nd factor's C-ABI (bsm_nd_factor_*, include/bsm.h):
the six entry points are exported and bound, the API version stays 1, the
header still compiles as C, and without a device the factorisation fails
loudly like every other hot-path call (no CPU fallback)."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bsm_nd_factor_create", "bsm_nd_factor_solve", "bsm_nd_factor_info", "bsm_nd_factor_perm",
         "bsm_nd_factor_export", "bsm_nd_factor_free"]


def _no_device():
    n = ctypes.c_int(0)
    _lib.load().bsm_device_count(ctypes.byref(n))
    return n.value == 0


def test_factor_symbols_exported_and_bound():
    assert_exported_and_bound(NAMES)


def test_factor_null_arguments_need_no_device():
    lib = _lib.load()
    assert lib.bsm_nd_factor_create(None, None) == _lib.BSM_ERR_INVALID
    assert "null" in _lib.last_error()
    assert lib.bsm_nd_factor_info(None, None, None, None, None) == _lib.BSM_ERR_INVALID
    assert lib.bsm_nd_factor_export(None, None, None) == _lib.BSM_ERR_INVALID
    lib.bsm_nd_factor_free(None)  # like free(NULL)


def test_header_with_factor_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    bsm_nd_factor* f = 0;\n"
        "    uint64_t n = 1, bytes = 1, nnz = 1;\n"
        "    int dt = -1;\n"
        "    int (*create)(const bsm_csr*, bsm_nd_factor**) = bsm_nd_factor_create;\n"
        "    int (*solve)(const bsm_nd_factor*, uint64_t, uint64_t, const void* const*, void* const*) =\n"
        "        bsm_nd_factor_solve;\n"
        "    int (*perm)(const bsm_nd_factor*, int64_t*) = bsm_nd_factor_perm;\n"
        "    int (*exp)(const bsm_nd_factor*, bsm_csr**, bsm_csr**) = bsm_nd_factor_export;\n"
        "    if (!create || !solve || !perm || !exp) return 2;\n"
        "    if (create(0, &f) != BSM_ERR_INVALID) return 3;\n"
        "    if (bsm_nd_factor_info(f, &n, &dt, &bytes, &nnz) != BSM_ERR_INVALID) return 4;\n"
        "    bsm_nd_factor_free(f);\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "f.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile the factor declarations of bsm.h as C"
    assert os.system(str(exe)) == 0


def test_factor_create_without_device_is_the_no_device_error():
    """The same failure, code and message, as another hot-path call
    (bsm_csr_transpose) gives on a host without a GPU. No handle can exist
    there (the upload fails the same way), so both calls get a zeroed block in
    its place: they ask for the device before they read the handle."""
    if not _no_device():
        pytest.skip("a GPU is visible")
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)
    addr = ctypes.cast(fake, ctypes.c_void_p)
    t = ctypes.c_void_p()
    rc_ref = lib.bsm_csr_transpose(addr, ctypes.byref(t))
    msg_ref = _lib.last_error()
    out = ctypes.c_void_p()
    rc = lib.bsm_nd_factor_create(addr, ctypes.byref(out))
    msg = _lib.last_error()
    assert rc_ref not in (_lib.BSM_OK, _lib.BSM_ERR_INVALID)
    assert rc == rc_ref
    assert msg.split(" (")[0] == msg_ref.split(" (")[0]  # the same HIP failure; the source line differs
    assert out.value is None and t.value is None
    rp = np.array([0, 1], dtype=np.uint64)
    ci = np.array([0], dtype=np.uint64)
    h = ctypes.c_void_p()
    rc_up = lib.bsm_csr_upload(_lib.BSM_F64, 1, 1, 1, _lib.ptr(rp), _lib.ptr(ci), _lib.ptr(np.array([4.0])),
                               ctypes.byref(h))
    assert rc_up == rc


def test_cholesky_nd_and_ndfactor_import_and_raise_without_device():
    import basic_sparse_matrix_amd as bsm
    from basic_sparse_matrix_amd import Csr, NdFactor, Panic, cholesky_nd

    assert "cholesky_nd" in bsm.__all__ and "NdFactor" in bsm.__all__
    for name in ("solve", "perm", "l", "l_star", "nbytes", "close", "__enter__", "__exit__"):
        assert hasattr(NdFactor, name), name
    # host-side checks come first, as in solve(): they need no device
    with pytest.raises(Panic):
        cholesky_nd(Csr.from_data([[1.0, 2.0]], dtype=np.float32))
    with pytest.raises(TypeError):
        cholesky_nd(Csr.from_data([[1, 0], [0, 1]], dtype=np.int32))
    if _no_device():
        with pytest.raises(_lib.DeviceUnavailable):
            cholesky_nd(Csr.from_data([[4.0, 1.0], [1.0, 3.0]]))
