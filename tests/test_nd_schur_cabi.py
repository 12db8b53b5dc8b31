"""CPU checks of the Schur complement's C-ABI (include/bsm.h): the entry points
are exported and bound and the API version stays 1 (additions), the header
with them still compiles as C, and the refusals that come before any device
is asked for (null pointers, a factor made without a set, an index >= n, a
repeated index, a set above the cap, ld < m) answer in that order and touch
nothing. This machine has no GPU, so a call that got past them would answer
BSM_ERR_NO_DEVICE instead."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bsm_nd_analyse_last", "bsm_nd_factor_create_schur", "bsm_nd_factor_schur_info", "bsm_nd_factor_schur",
         "bsm_dev_nd_factor_schur", "bsm_nd_factor_schur_condense", "bsm_nd_factor_schur_expand",
         "bsm_dev_nd_factor_schur_condense", "bsm_dev_nd_factor_schur_expand")
CAP = 16384


def test_schur_symbols_exported_and_bound():
    assert_exported_and_bound(NAMES)


def fake_csr(n):
    """Zeros with rows = cols = n where bsm_csr keeps them (two ints, then three uint64): the set is checked against
    n alone, before anything else of the handle is read."""
    buf = ctypes.create_string_buffer(4096)
    np.frombuffer(buf, dtype=np.uint64, count=3, offset=8)[:2] = n
    return buf


def test_create_schur_refusals_need_no_device():
    lib = _lib.load()
    a = fake_csr(CAP + 10)
    before = a.raw
    out = ctypes.c_void_p(0)

    def create(idx, a=a, dt=_lib.DTYPE_CODES[np.dtype(np.float64)], out=ctypes.byref(out), m=None):
        iv = None if idx is None else np.asarray(idx, dtype=np.uint64)
        return lib.bsm_nd_factor_create_schur(ctypes.cast(a, ctypes.c_void_p) if a is not None else None, dt,
                                              None if iv is None else _lib.ptr(iv),
                                              m if m is not None else (0 if iv is None else iv.shape[0]), out)

    for rc in (create([1, 2], a=None), create([1, 2], out=None), create(None, m=2)):
        assert rc == _lib.BSM_ERR_INVALID and "null" in _lib.last_error()
    assert create([1, 2], dt=_lib.DTYPE_CODES[np.dtype(np.int32)]) == _lib.BSM_ERR_INVALID
    assert "factor_dtype" in _lib.last_error()
    assert create([3, CAP + 10, 3]) == _lib.BSM_ERR_INVALID  # an index >= n is named before a repeat
    assert "idx[1]" in _lib.last_error()
    assert create([3, 7, 9, 7]) == _lib.BSM_ERR_INVALID
    assert "idx[3] = 7 repeats" in _lib.last_error()
    assert create(np.arange(CAP + 1)) == _lib.BSM_ERR_UNSUPPORTED
    assert "16384" in _lib.last_error()
    assert out.value is None and a.raw == before


def test_analyse_last_cap():
    lib = _lib.load()
    n = CAP + 2
    rp = np.arange(n + 1, dtype=np.uint64)  # the identity's pattern
    ci = np.arange(n, dtype=np.uint64)
    nn, sl = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for m, want in ((CAP + 1, _lib.BSM_ERR_UNSUPPORTED), (CAP, _lib.BSM_OK)):
        lv = np.arange(m, dtype=np.uint64)
        assert lib.bsm_nd_analyse_last(n, _lib.ptr(rp), _lib.ptr(ci), 64, _lib.ptr(lv), m, None, None, 0,
                                       ctypes.byref(nn), None, 0, ctypes.byref(sl)) == want


def test_schur_calls_refuse_before_any_device():
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)  # zeros: a factor of n == 0 made without a set
    f = ctypes.cast(fake, ctypes.c_void_p)
    a = ctypes.cast(fake_csr(4), ctypes.c_void_p)
    buf = np.full(4, 7.0)
    cols = _lib.ptr_array([buf])
    m = ctypes.c_uint64(9)
    assert lib.bsm_nd_factor_schur_info(None, ctypes.byref(m), None) == _lib.BSM_ERR_INVALID
    assert lib.bsm_nd_factor_schur_info(f, ctypes.byref(m), None) == _lib.BSM_OK and m.value == 0
    calls = {
        "schur": lambda f, p: lib.bsm_nd_factor_schur(f, a, p, 4),
        "dev schur": lambda f, p: lib.bsm_dev_nd_factor_schur(f, a, p, 4, None),
        "condense": lambda f, p: lib.bsm_nd_factor_schur_condense(f, cols, 1, cols),
        "dev condense": lambda f, p: lib.bsm_dev_nd_factor_schur_condense(f, p, 1, p, None),
        "expand": lambda f, p: lib.bsm_nd_factor_schur_expand(f, cols, 1, cols, cols),
        "dev expand": lambda f, p: lib.bsm_dev_nd_factor_schur_expand(f, p, 1, p, p, None),
    }
    for name, call in calls.items():
        assert call(None, _lib.ptr(buf)) == _lib.BSM_ERR_INVALID, name
        assert "null" in _lib.last_error(), name
        assert call(f, _lib.ptr(buf)) == _lib.BSM_ERR_INVALID, name  # never BSM_ERR_NO_DEVICE: the set comes first
        assert "without a Schur set" in _lib.last_error(), name
    assert lib.bsm_nd_factor_schur(f, None, _lib.ptr(buf), 4) == _lib.BSM_ERR_INVALID
    assert np.array_equal(buf, np.full(4, 7.0)) and fake.raw == bytes(4096)


def test_python_mirrors_exist_and_check_on_the_host():
    import inspect

    from basic_sparse_matrix_amd import NdFactor, cholesky_nd, device

    for name in ("schur", "schur_condense", "schur_expand", "schur_index"):
        assert hasattr(NdFactor, name), name
    for name in ("nd_factor_schur", "nd_factor_schur_condense", "nd_factor_schur_expand"):
        assert hasattr(device, name), name
    assert list(inspect.signature(cholesky_nd).parameters) == ["a", "factor_dtype", "schur"]
    f = NdFactor.__new__(NdFactor)  # a closed factor: used after close() is refused first
    f.handle, f.n, f.dtype = None, 2, np.dtype(np.float64)
    with pytest.raises(ValueError, match="after close"):
        f.schur_index


def test_header_with_schur_compiles_as_c(tmp_path):
    src = tmp_path / "f.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    uint64_t idx[2] = {0, 1}, m = 9;\n"
        "    double v[4] = {7.0, 7.0, 7.0, 7.0};\n"
        "    const void* bc[1] = {v};\n"
        "    void* xc[1] = {v};\n"
        "    bsm_nd_factor* f = 0;\n"
        "    int (*cs)(const bsm_csr*, int, const uint64_t*, uint64_t, bsm_nd_factor**) = bsm_nd_factor_create_schur;\n"
        "    int (*si)(const bsm_nd_factor*, uint64_t*, uint64_t*) = bsm_nd_factor_schur_info;\n"
        "    int (*sh)(const bsm_nd_factor*, const bsm_csr*, void*, uint64_t) = bsm_nd_factor_schur;\n"
        "    int (*sd)(const bsm_nd_factor*, const bsm_csr*, void*, uint64_t, void*) = bsm_dev_nd_factor_schur;\n"
        "    int (*co)(const bsm_nd_factor*, const void* const*, uint64_t, void* const*) = bsm_nd_factor_schur_condense;\n"
        "    int (*ex)(const bsm_nd_factor*, const void* const*, uint64_t, const void* const*, void* const*) =\n"
        "        bsm_nd_factor_schur_expand;\n"
        "    int (*dc)(const bsm_nd_factor*, const void*, uint64_t, void*, void*) = bsm_dev_nd_factor_schur_condense;\n"
        "    int (*de)(const bsm_nd_factor*, const void*, uint64_t, const void*, void*, void*) =\n"
        "        bsm_dev_nd_factor_schur_expand;\n"
        "    if (cs(0, BSM_F64, idx, 2, &f) != BSM_ERR_INVALID || f) return 2;\n"
        "    if (si(0, &m, idx) != BSM_ERR_INVALID || sh(0, 0, v, 2) != BSM_ERR_INVALID) return 3;\n"
        "    if (sd(0, 0, v, 2, 0) != BSM_ERR_INVALID || co(0, bc, 1, xc) != BSM_ERR_INVALID) return 4;\n"
        "    if (ex(0, bc, 1, bc, xc) != BSM_ERR_INVALID || dc(0, v, 1, v, 0) != BSM_ERR_INVALID) return 5;\n"
        "    if (de(0, v, 1, v, v, 0) != BSM_ERR_INVALID || v[0] != 7.0 || m != 9) return 6;\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "f.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile the Schur complement's declarations of bsm.h as C"
    assert os.system(str(exe)) == 0
