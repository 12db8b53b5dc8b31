"""CPU checks of the differentiable solve's C-ABI (include/bsm.h):
bsm_dev_sddmm, bsm_dev_nd_factor_sddmm, bsm_dev_nd_factor_refactor_values,
bsm_dev_nd_factor_inv_pattern and bsm_nd_factor_pattern_info are exported and
bound, the API version stays 1 (they are additions), the header with them and
BSM_SDDMM_* still compiles as C, null and invalid arguments are refused before
any device is asked for, and the Python wrappers (device.py, autograd.py,
NdFactor) exist and make their host-side checks on a closed factor."""

import ctypes
import os

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from nd_support import assert_exported_and_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bsm_dev_sddmm", "bsm_dev_nd_factor_sddmm", "bsm_dev_nd_factor_refactor_values",
         "bsm_dev_nd_factor_inv_pattern", "bsm_nd_factor_pattern_info"]
F64, F32, I32 = (_lib.DTYPE_CODES[np.dtype(t)] for t in (np.float64, np.float32, np.int32))


def test_grad_symbols_exported_and_bound():
    assert_exported_and_bound(NAMES)
    assert (_lib.BSM_SDDMM_ALL, _lib.BSM_SDDMM_SYM_LOWER) == (0, 1)


def test_grad_null_arguments_need_no_device():
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)  # never read: another argument is refused first
    addr = ctypes.cast(fake, ctypes.c_void_p)
    nnz, dt = ctypes.c_uint64(7), ctypes.c_int(7)
    for rc in (lib.bsm_dev_nd_factor_sddmm(None, F64, 1, 1, addr, addr, addr, None),
               lib.bsm_dev_nd_factor_refactor_values(None, F64, 1, addr, None),
               lib.bsm_dev_nd_factor_inv_pattern(None, 1, addr, None),
               lib.bsm_nd_factor_pattern_info(None, ctypes.byref(nnz), ctypes.byref(dt)),
               lib.bsm_dev_sddmm(F64, 0, 2, 2, 3, None, addr, 1, addr, addr, addr, None),
               lib.bsm_dev_sddmm(F64, 0, 2, 2, 3, addr, None, 1, addr, addr, addr, None),
               lib.bsm_dev_sddmm(F64, 1, 2, 2, 3, addr, addr, 1, None, addr, addr, None),
               lib.bsm_dev_sddmm(F32, 1, 2, 2, 3, addr, addr, 1, addr, None, addr, None),
               lib.bsm_dev_sddmm(F32, 0, 2, 2, 3, addr, addr, 1, addr, addr, None, None)):
        assert rc == _lib.BSM_ERR_INVALID
        assert "null" in _lib.last_error()
    assert (nnz.value, dt.value) == (7, 7)


def test_sddmm_invalid_arguments_need_no_device():
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)  # never read: the arguments are refused before a launch
    a = ctypes.cast(fake, ctypes.c_void_p)
    for args, word in (((F64, 0, 2, 2, 3, a, a, 0, a, a, a, None), "k == 0"),
                       ((I32, 0, 2, 2, 3, a, a, 1, a, a, a, None), "f32/f64"),
                       ((99, 0, 2, 2, 3, a, a, 1, a, a, a, None), "f32/f64"),
                       ((F64, 2, 2, 2, 3, a, a, 1, a, a, a, None), "mode"),
                       ((F64, -1, 2, 2, 3, a, a, 1, a, a, a, None), "mode"),
                       ((F32, 1, 2, 3, 3, a, a, 1, a, a, a, None), "square")):
        assert lib.bsm_dev_sddmm(*args) == _lib.BSM_ERR_INVALID, args
        assert word in _lib.last_error(), (_lib.last_error(), word)
    # nothing to do: no launch, no device, null arrays accepted
    assert lib.bsm_dev_sddmm(F64, 0, 0, 5, 0, None, None, 3, None, None, None, None) == _lib.BSM_OK
    assert lib.bsm_dev_sddmm(F64, 1, 4, 4, 0, a, None, 3, a, a, None, None) == _lib.BSM_OK


def _closed_factor(dtype=np.float64, src=np.float64):
    from basic_sparse_matrix_amd import NdFactor

    f = NdFactor.__new__(NdFactor)  # a closed factor: the host-side checks come first
    f.handle, f.n, f.dtype, f.src_dtype = None, 3, np.dtype(dtype), np.dtype(src)
    f._pattern_nnz, f._epoch, f._vals_key, f._vals_ref, f._grad_weights = 5, 0, None, None, None
    return f


def test_python_wrappers_exist_and_check_on_the_host():
    import torch

    from basic_sparse_matrix_amd import NdFactor, autograd, device

    for name in ("pattern_nnz", "refactor_values", "_bump_epoch"):
        assert hasattr(NdFactor, name), name
    for name in ("sddmm", "nd_factor_sddmm", "nd_factor_refactor_values", "nd_factor_inv_pattern"):
        assert callable(getattr(device, name)), name
    assert callable(autograd.nd_solve) and callable(autograd.nd_logdet)
    import basic_sparse_matrix_amd

    assert not hasattr(basic_sparse_matrix_amd, "nd_solve")  # autograd is not pulled in by the package
    f = _closed_factor()
    assert f.pattern_nnz == 5 and f.src_dtype == np.float64
    z64 = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    z32 = lambda *s: torch.zeros(*s, dtype=torch.float32)  # noqa: E731
    rp, col = torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int32)

    # wrong dtype
    with pytest.raises(TypeError):
        device.nd_factor_refactor_values(f, z32(5))
    with pytest.raises(TypeError):
        f.refactor_values(z32(5))
    with pytest.raises(TypeError):
        device.nd_factor_inv_pattern(f, out=z32(5))
    with pytest.raises(TypeError):
        device.nd_factor_sddmm(f, z64(3, 2), z32(3, 2))
    with pytest.raises(TypeError):
        device.sddmm(rp, col, z64(3, 2), z32(3, 2))
    with pytest.raises(TypeError):
        device.sddmm(rp.to(torch.int32), col, z64(3, 2), z64(3, 2))
    with pytest.raises(TypeError):
        autograd.nd_solve(f, z32(5), z64(3))
    with pytest.raises(TypeError):
        autograd.nd_logdet(f, z32(5))
    # an f32 factor of an f64 matrix is not differentiable in this version
    with pytest.raises(TypeError):
        autograd.nd_solve(_closed_factor(np.float32, np.float64), z64(5), z32(3))
    with pytest.raises(TypeError):
        autograd.nd_logdet(_closed_factor(np.float32, np.float64), z64(5))
    # wrong length, k == 0, another mode: each by the message of the check it names (the tensors are on the CPU,
    # which the wrappers would refuse too, but only after the shapes)
    with pytest.raises(ValueError, match=r"vals must be contiguous, \(5,\), got \(4,\)"):
        device.nd_factor_refactor_values(f, z64(4))
    with pytest.raises(ValueError, match=r"out must be contiguous, \(5,\), got \(6,\)"):
        device.nd_factor_inv_pattern(f, out=z64(6))
    with pytest.raises(ValueError, match=r"u must be \(3,\) or \(3, k\), got \(4, 2\)"):
        device.nd_factor_sddmm(f, z64(4, 2), z64(4, 2))
    with pytest.raises(ValueError, match=r"out must be \(5,\), got \(4,\)"):
        device.nd_factor_sddmm(f, z64(3, 2), z64(3, 2), out=z64(4))
    with pytest.raises(ValueError, match="u has 2 columns, v 3"):
        device.nd_factor_sddmm(f, z64(3, 2), z64(3, 3))
    with pytest.raises(ValueError, match="k == 0"):
        device.nd_factor_sddmm(f, z64(3, 0), z64(3, 0))
    with pytest.raises(ValueError, match="k == 0"):
        device.sddmm(rp, col, z64(3, 0), z64(3, 0))
    with pytest.raises(ValueError, match="mode must be one of"):
        device.sddmm(rp, col, z64(3, 2), z64(3, 2), mode="x")
    with pytest.raises(ValueError, match=r"vals must be contiguous, \(5,\), got \(4,\)"):
        autograd.nd_solve(f, z64(4), z64(3))
    with pytest.raises(ValueError, match=r"vals must be contiguous, \(5,\), got \(5, 1\)"):
        autograd.nd_logdet(f, z64(5, 1))
    # well-shaped CPU tensors get as far as the device check, and no further
    with pytest.raises(ValueError, match="not on the device"):
        device.nd_factor_refactor_values(f, z64(5))
    with pytest.raises(ValueError, match="not on the device"):
        device.nd_factor_sddmm(f, z64(3, 2), z64(3, 2), out=z64(5))
    assert f._epoch == 0  # nothing got as far as the factor


def test_header_with_grad_calls_compiles_as_c(tmp_path):
    src = tmp_path / "g.c"
    src.write_text(
        '#include "bsm.h"\n'
        "int main(void) {\n"
        "    uint64_t nnz = 7;\n"
        "    int dt = 7;\n"
        "    int modes[2] = {BSM_SDDMM_ALL, BSM_SDDMM_SYM_LOWER};\n"
        "    int (*sd)(int, int, uint64_t, uint64_t, uint64_t, const int64_t*, const int32_t*, uint64_t, const void*,\n"
        "              const void*, void*, void*) = bsm_dev_sddmm;\n"
        "    int (*fsd)(const bsm_nd_factor*, int, uint64_t, uint64_t, const void*, const void*, void*, void*) =\n"
        "        bsm_dev_nd_factor_sddmm;\n"
        "    int (*rv)(bsm_nd_factor*, int, uint64_t, const void*, void*) = bsm_dev_nd_factor_refactor_values;\n"
        "    int (*ip)(const bsm_nd_factor*, uint64_t, void*, void*) = bsm_dev_nd_factor_inv_pattern;\n"
        "    int (*pi)(const bsm_nd_factor*, uint64_t*, int*) = bsm_nd_factor_pattern_info;\n"
        "    if (modes[0] != 0 || modes[1] != 1) return 2;\n"
        "    if (sd(BSM_F64, BSM_SDDMM_ALL, 2, 2, 3, 0, 0, 0, 0, 0, 0, 0) != BSM_ERR_INVALID) return 3;\n"
        "    if (sd(BSM_F64, BSM_SDDMM_ALL, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0) != BSM_OK) return 4;\n"
        "    if (fsd(0, BSM_F64, 0, 1, 0, 0, 0, 0) != BSM_ERR_INVALID) return 5;\n"
        "    if (rv(0, BSM_F64, 0, 0, 0) != BSM_ERR_INVALID) return 6;\n"
        "    if (ip(0, 0, 0, 0) != BSM_ERR_INVALID) return 7;\n"
        "    if (pi(0, &nnz, &dt) != BSM_ERR_INVALID || nnz != 7 || dt != 7) return 8;\n"
        "    return bsm_api_version() == 1 ? 0 : 1;\n"
        "}\n")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "basic_sparse_matrix_amd", "lib")
    exe = tmp_path / "g.out"
    r = os.system(f"gcc -std=c99 -Wall -Werror -I{inc} {src} -L{libdir} -lbsm_hip -Wl,-rpath,{libdir} -o {exe} "
                  "2>/dev/null")
    assert r == 0, "gcc failed to compile the differentiable solve's declarations of bsm.h as C"
    assert os.system(str(exe)) == 0
