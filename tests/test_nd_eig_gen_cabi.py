"""CPU checks of the generalised eigsh's additions to the C-ABI (include/bsm.h):
bsm_nd_factor_eigsh_gen and bsm_dev_nd_factor_eigsh_gen are exported and bound,
the API version stays 1 (they are additions), the header with them still
compiles as C, null, tol, nev, block and ncv arguments are refused before any
device is asked for and touch no output, with m NULL and with m a handle, and
the Python mirrors take m= with their host-side checks."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bsm_nd_factor_eigsh_gen", "bsm_dev_nd_factor_eigsh_gen"]


def test_eig_gen_symbols_exported_and_bound():
    assert_exported_and_bound(NAMES)


def test_eig_gen_bad_arguments_need_no_device():
    lib = _lib.load()
    # never read past the refused argument; all zero, so the factor it stands for is 0 x 0: nev must be 0, ncv 0
    fake = ctypes.create_string_buffer(4096)
    addr = ctypes.cast(fake, ctypes.c_void_p)
    y = np.full(4, 7.0)
    lam = np.full(2, 7.0)
    resid = np.full(2, 7.0)
    info = np.full(4, 7, dtype=np.uint32)
    cols = _lib.ptr_array([y, y])
    lp, rp, ip, yp = _lib.ptr(lam), _lib.ptr(resid), _lib.ptr(info), _lib.ptr(y)

    for m in (None, addr):
        def host(f=addr, a=addr, nev=0, block=4, ncv=0, tol=0.0, lam_p=lp, resid_p=rp):
            return lib.bsm_nd_factor_eigsh_gen(f, a, m, nev, block, ncv, tol, 0, None, lam_p, cols, resid_p, ip)

        def dev(f=addr, a=addr, nev=0, block=4, ncv=0, tol=0.0, lam_p=lp, resid_p=rp):
            return lib.bsm_dev_nd_factor_eigsh_gen(f, a, m, nev, block, ncv, tol, 0, None, lam_p, yp, resid_p, ip,
                                                   None)

        for call in (host, dev):
            for kw in ({"f": None}, {"a": None}, {"lam_p": None}, {"resid_p": None}):
                assert call(**kw) == _lib.BSM_ERR_INVALID
                assert "null" in _lib.last_error()
            for tol in (-1.0, -1e-300, float("nan"), float("-inf")):
                assert call(tol=tol) == _lib.BSM_ERR_INVALID
                assert "tol" in _lib.last_error()
            for block in (0, 33, 2 ** 40):
                assert call(block=block) == _lib.BSM_ERR_INVALID
                assert "block must" in _lib.last_error()
            assert call(nev=2) == _lib.BSM_ERR_INVALID  # on the 0 x 0 factor only nev == 0 is accepted
            assert "nev must" in _lib.last_error()
            for ncv in (4, 9):  # rounded down to 4 and 8: above n = 0
                assert call(ncv=ncv) == _lib.BSM_ERR_INVALID
                assert "ncv (" in _lib.last_error()
    assert np.all(y == 7.0) and np.all(lam == 7.0) and np.all(resid == 7.0) and np.all(info == 7)


def test_python_mirrors_take_m_and_check_it_on_the_host():
    import inspect

    from basic_sparse_matrix_amd import Csr, EigInfo, MatErr, NdFactor, device

    assert [f for f in EigInfo.__dataclass_fields__] == ["steps", "ncv_used", "resid", "converged", "exhausted",
                                                         "inexact", "tol"]
    for fn in (NdFactor.eigsh, device.nd_factor_eigsh):
        p = inspect.signature(fn).parameters["m"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    a = Csr.from_data([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 5.0]])
    good = Csr.from_data([[2.0, 0.5, 0.0], [0.5, 2.0, 0.5], [0.0, 0.5, 2.0]])
    f = NdFactor.__new__(NdFactor)  # a closed factor: the host-side checks come first
    f.handle, f.n, f.dtype = None, 3, np.dtype(np.float32)
    with pytest.raises(ValueError, match="after close"):
        f.eigsh(a, 1, m=good)
    with pytest.raises(ValueError, match="after close"):
        device.nd_factor_eigsh(f, a, 1, m=good)
    f.handle = 1  # never passed on: the arguments are refused first
    try:
        for call in (f.eigsh, lambda *args, **kw: device.nd_factor_eigsh(f, *args, **kw)):
            with pytest.raises(TypeError, match="m must have a's dtype"):
                call(a, 1, block=1, m=Csr.from_data([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0]],
                                                    dtype=np.float32))
            with pytest.raises(TypeError, match="m must have a's dtype"):
                call(a, 1, block=1, m=Csr.from_data([[2, 0, 0], [0, 2, 0], [0, 0, 2]], dtype=np.int32))
            with pytest.raises(TypeError, match="m must be a Csr"):
                call(a, 1, block=1, m=np.eye(3))
            with pytest.raises(MatErr):
                call(a, 1, block=1, m=Csr.from_data([[2.0, 0.5], [0.5, 2.0]]))
            with pytest.raises(ValueError, match="nev"):  # the argument checks without m still come first
                call(a, 0, block=1, m=good)
            with pytest.raises(TypeError):
                call(a, 1, 1, None, None, None, 0, None, True, None, good)  # m is keyword only
    finally:
        f.handle = None  # nothing for close() to free


def test_header_with_eigsh_gen_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    double y[2] = {7.0, 7.0}, lam[1] = {7.0}, resid[1] = {7.0};\n"
        "    uint32_t info[4] = {7, 7, 7, 7};\n"
        "    void* yc[1];\n"
        "    int fake[1024] = {0};\n"
        "    const bsm_nd_factor* f = (const bsm_nd_factor*)fake; /* never read past the refused argument */\n"
        "    const bsm_csr* a = (const bsm_csr*)fake;\n"
        "    int (*host)(const bsm_nd_factor*, const bsm_csr*, const bsm_csr*, uint64_t, uint64_t, uint64_t, double,\n"
        "                uint64_t, const void* const*, double*, void* const*, double*, uint32_t*) =\n"
        "        bsm_nd_factor_eigsh_gen;\n"
        "    int (*dev)(const bsm_nd_factor*, const bsm_csr*, const bsm_csr*, uint64_t, uint64_t, uint64_t, double,\n"
        "               uint64_t, const void*, double*, void*, double*, uint32_t*, void*) = bsm_dev_nd_factor_eigsh_gen;\n"
        "    yc[0] = y;\n"
        "    if (host(0, a, a, 1, 4, 0, 0.0, 0, 0, lam, yc, resid, info) != BSM_ERR_INVALID) return 4;\n"
        "    if (host(f, a, 0, 1, 4, 0, -1.0, 0, 0, lam, yc, resid, info) != BSM_ERR_INVALID) return 5;\n"
        "    if (host(f, a, a, 0, 0, 0, 0.0, 0, 0, lam, yc, resid, info) != BSM_ERR_INVALID) return 6;\n"
        "    if (dev(f, 0, a, 1, 4, 0, 0.0, 0, 0, lam, y, resid, info, 0) != BSM_ERR_INVALID) return 7;\n"
        "    if (dev(f, a, 0, 0, 4, 0, 0.0, 0, 0, 0, y, resid, info, 0) != BSM_ERR_INVALID) return 8;\n"
        "    if (dev(f, a, a, 0, 33, 0, 0.0, 0, 0, lam, y, resid, 0, 0) != BSM_ERR_INVALID) return 9;\n"
        "    if (y[0] != 7.0 || y[1] != 7.0 || lam[0] != 7.0 || resid[0] != 7.0 || info[0] != 7 || info[3] != 7)\n"
        "        return 10;\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "f.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile eigsh_gen's declarations of bsm.h as C"
    assert os.system(str(exe)) == 0
