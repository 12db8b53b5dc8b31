"""GPU tests of the differentiable use of a kept nd factor: refactor_values
(the numeric factor again from device values), inv_pattern (S^-1 on the kept
pattern, on the device), and autograd.nd_solve / nd_logdet with their guards.

The systems are nd_support.py's; the second values (A2 = D A D), the
not-positive-definite variant and snapshot() are
tests/test_gpu_nd_factor_ops.py's, with its tolerances
TOL = {f64: 1e-10, f32: 2e-3}. The gradients are compared with the dense f64
formulas, evaluated with numpy on the CPU from the dense S (the stored entries
with col <= row, mirrored), G the upstream gradient and Λ = S^-1 G:

  solve   d/db = Λ;  d/dvals[p = (i, j)] = -(Λ_i . x_j + Λ_j . x_i) for j < i,
          -(Λ_i . x_i) for j == i, 0 for j > i
  logdet  2 (S^-1)[i, j] for j < i, (S^-1)[i, i] for j == i, 0 for j > i

by the relative 2-norm error of grad_vals and of grad_b."""

import ctypes
import functools

import numpy as np
import pytest

from basic_sparse_matrix_amd import Csr, Dense, _lib, cholesky_nd
from nd_support import assert_same, coords, rel_err, same_bits, sym_dense, system
# the value sets (A2 = D A D, the not-positive-definite one) and what a factor answers are that feature's
from test_gpu_nd_factor_ops import TOL, _values, invalid, matrix, setup, snapshot

pytestmark = pytest.mark.gpu

SYSTEMS = ["g5-leaf1", "g11-leaf8", "g11-onefront", "blocks", "random"]
F64, F32 = np.float64, np.float32
# (the matrix's dtype, the factor's)
KINDS = {"f64": (F64, F64), "f32": (F32, F32), "f32-of-f64": (F64, F32)}


def dev(a):
    import torch

    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def everything(f, b):
    return snapshot(f, b) + [np.float64(f.logdet())]


def pattern(name):
    """(n, rows, cols) of the stored entries, in storage order."""
    return (system(name)[0], *coords(name))


# ---- refactor_values --------------------------------------------------------


@pytest.mark.parametrize("plain", ["0", "1"], ids=["pipeline", "plain"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", SYSTEMS)
def test_refactor_values_has_the_bits_of_refactor(monkeypatch, name, kind, plain):
    monkeypatch.setenv("BSM_ND_PLAIN", plain)
    src, fdt = KINDS[kind]
    _, b = setup(monkeypatch, name, fdt)
    v2 = dev(_values(name)[1].astype(src))
    with cholesky_nd(matrix(name, src), factor_dtype=fdt) as f, cholesky_nd(matrix(name, src), factor_dtype=fdt) as g, \
            cholesky_nd(matrix(name, src, 1), factor_dtype=fdt) as fresh:
        assert f.pattern_nnz == v2.shape[0] and f.src_dtype == np.dtype(src) and f.dtype == np.dtype(fdt)
        before = everything(f, b)
        e0 = f._epoch
        f.refactor_values(v2)
        assert f._epoch == e0 + 1
        g.refactor(matrix(name, src, 1))
        got = everything(f, b)
        assert_same(got, everything(g, b))
        assert_same(got, everything(fresh, b))
        assert not same_bits(got[0], before[0])
        f.refactor_values(dev(_values(name)[0].astype(src)))  # and back
        assert_same(everything(f, b), before)


@pytest.mark.parametrize("kind", ["f64", "f32-of-f64"])
def test_refactor_values_not_positive_definite(monkeypatch, kind):
    name = "g11-leaf8"
    src, fdt = KINDS[kind]
    _, b = setup(monkeypatch, name, fdt)
    with cholesky_nd(matrix(name, src), factor_dtype=fdt) as f, \
            cholesky_nd(matrix(name, src, 1), factor_dtype=fdt) as fresh:
        with pytest.raises(_lib.BsmError, match="positive definite") as want:
            fresh.refactor(matrix(name, src, 2))
        e0 = f._epoch
        with pytest.raises(_lib.BsmError, match="positive definite") as err:
            f.refactor_values(dev(_values(name)[2].astype(src)))
        assert (err.value.code, err.value.msg) == (want.value.code, want.value.msg)
        assert err.value.code == _lib.BSM_ERR_UNSUPPORTED
        assert f._epoch == e0 + 1 and f._vals_key is None  # counted although it failed
        for call in (f.logdet, f.l, lambda: f.solve(Dense.from_columns(b[:1]))):
            with invalid("holds no values; refactor first"):
                call()
        fresh.refactor(matrix(name, src, 1))
        f.refactor_values(dev(_values(name)[1].astype(src)))  # a good call revives it
        assert_same(everything(f, b), everything(fresh, b))


def test_refactor_values_refusals_leave_the_factor_untouched(monkeypatch):
    import torch

    name = "g11-leaf8"
    _, b = setup(monkeypatch, name, F64)
    lib = _lib.require_device()
    v2 = dev(_values(name)[1])
    s = torch.cuda.current_stream().cuda_stream
    c64, c32 = _lib.DTYPE_CODES[np.dtype(F64)], _lib.DTYPE_CODES[np.dtype(F32)]
    with cholesky_nd(matrix(name, F64)) as f:
        base = everything(f, b)
        e0 = f._epoch
        nnz = f.pattern_nnz
        with pytest.raises(ValueError):
            f.refactor_values(v2[:-1])
        with pytest.raises(ValueError):
            f.refactor_values(torch.cat([v2, v2])[::2])
        with pytest.raises(TypeError):
            f.refactor_values(v2.float())
        with pytest.raises(ValueError):
            f.refactor_values(v2.cpu())
        assert f._epoch == e0
        for args, word in (((f._h(), c64, nnz - 1, v2.data_ptr(), s), "nnz differs"),
                           ((f._h(), c64, nnz + 1, v2.data_ptr(), s), "nnz differs"),
                           ((f._h(), c32, nnz, v2.data_ptr(), s), "dtype differs"),
                           ((f._h(), c64, nnz, None, s), "null")):
            assert lib.bsm_dev_nd_factor_refactor_values(*args) == _lib.BSM_ERR_INVALID
            assert word in _lib.last_error()
        out = torch.full((nnz,), float("nan"), dtype=torch.float64, device="cuda")
        for args, word in (((f._h(), nnz - 1, out.data_ptr(), s), "nnz differs"), ((f._h(), nnz, None, s), "null")):
            assert lib.bsm_dev_nd_factor_inv_pattern(*args) == _lib.BSM_ERR_INVALID
            assert word in _lib.last_error()
        o = out.data_ptr()
        for args, word in (((f._h(), c64, nnz + 1, 1, o, o, o, s), "nnz differs"),
                           ((f._h(), c64, nnz, 0, o, o, o, s), "k == 0"),
                           ((f._h(), 77, nnz, 1, o, o, o, s), "f32/f64"),
                           ((f._h(), c64, nnz, 1, o, None, o, s), "null")):
            assert lib.bsm_dev_nd_factor_sddmm(*args) == _lib.BSM_ERR_INVALID
            assert word in _lib.last_error()
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
        cnt, sd = ctypes.c_uint64(), ctypes.c_int()
        assert lib.bsm_nd_factor_pattern_info(f._h(), ctypes.byref(cnt), ctypes.byref(sd)) == _lib.BSM_OK
        assert (cnt.value, sd.value) == (nnz, c64)
        assert_same(everything(f, b), base)


def test_refactor_values_after_update_equals_a_fresh_factor(monkeypatch):
    """update() leaves the fronts' update blocks stale; refactor_values writes every one of them again."""
    name = "g11-leaf8"
    n, b = setup(monkeypatch, name, F64)
    w = Csr.from_csr_arrays((n, 1), np.concatenate([np.zeros(n // 2 + 1), np.ones(n - n // 2)]).astype(np.uint64),
                            np.zeros(1, dtype=np.uint64), np.array([0.5]))
    with cholesky_nd(matrix(name, F64)) as f, cholesky_nd(matrix(name, F64, 1)) as fresh:
        base = everything(f, b)
        f.update(w)
        assert not same_bits(everything(f, b)[0], base[0])
        with pytest.raises(_lib.BsmError, match="stale"):
            f.refactor_partial(matrix(name, F64, 1), [0], [0])
        f.refactor_values(dev(_values(name)[1]))
        assert_same(everything(f, b), everything(fresh, b))
        f.refactor_partial(matrix(name, F64, 1), [0], [0])  # allowed again: every update block was rewritten
        assert_same(everything(f, b), everything(fresh, b))


# ---- inv_pattern ------------------------------------------------------------


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_inv_pattern_has_the_bits_of_inv_on(monkeypatch, name, dtype):
    import torch

    from basic_sparse_matrix_amd import device

    setup(monkeypatch, name, dtype)
    n, rows, cols = pattern(name)
    A = matrix(name, dtype)
    with cholesky_nd(A) as f:
        want = np.asarray(f.inv_on(A).v)
        buf = torch.full((f.pattern_nnz + 8,), float("nan"), dtype=device.TORCH_DT[np.dtype(dtype)], device="cuda")
        got = device.nd_factor_inv_pattern(f, out=buf[:f.pattern_nnz])
        assert same_bits(got.cpu().numpy(), want)
        assert torch.isnan(buf[f.pattern_nnz:]).all()
        assert same_bits(device.nd_factor_inv_pattern(f).cpu().numpy(), want)
        # both triangles are stored: (i, j) and (j, i) carry the same bits
        assert (cols > rows).any() and (cols < rows).any()
        z = np.zeros((n, n), dtype=dtype)
        z[rows, cols] = want
        assert same_bits(z, np.ascontiguousarray(z.T))
        assert rel_err(want, np.linalg.inv(sym_of(name, dtype))[rows, cols]) <= TOL[dtype]


# ---- gradients --------------------------------------------------------------


def sym_of(name, dtype, which=0):
    """The dense S (f64) of the value set as the dtype stores it: col <= row, mirrored."""
    return sym_dense(name, _values(name)[which].astype(dtype))


@functools.lru_cache(maxsize=None)
def inverse(name, dtype):
    return np.linalg.inv(sym_of(name, dtype, 1))


def rhs(name, k, dtype, seed):
    n = system(name)[0]
    r = np.random.default_rng(seed).standard_normal((n, k) if k > 1 else (n,))
    return r.astype(dtype)


def solve_grads(name, dtype, b, g):
    """(grad_vals, grad_b) of sum(g * S^-1 b) by the dense formulas, f64."""
    n, rows, cols = pattern(name)
    zi = inverse(name, dtype)
    b2, g2 = (np.asarray(t, dtype=np.float64).reshape(n, -1) for t in (b, g))
    x, lam = zi @ b2, zi @ g2
    gv = -(np.einsum("pc,pc->p", lam[rows], x[cols]) + np.einsum("pc,pc->p", lam[cols], x[rows]))
    gv[rows == cols] = -np.einsum("pc,pc->p", lam[rows], x[cols])[rows == cols]
    gv[cols > rows] = 0.0
    return gv, lam.reshape(np.shape(b))


def logdet_grads(name, dtype):
    n, rows, cols = pattern(name)
    zi = inverse(name, dtype)
    return np.where(cols < rows, 2.0, np.where(cols == rows, 1.0, 0.0)) * zi[rows, cols]


def leaf(a):
    return dev(a).requires_grad_(True)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_gradients_against_the_dense_formulas(monkeypatch, name, dtype):
    import torch

    from basic_sparse_matrix_amd import autograd

    setup(monkeypatch, name, dtype)
    n, rows, cols = pattern(name)
    upper = cols > rows
    assert upper.any()
    v2 = _values(name)[1].astype(dtype)
    ld_want = logdet_grads(name, dtype)
    with cholesky_nd(matrix(name, dtype)) as f:
        # nd_logdet alone
        vals = leaf(v2)
        ld = autograd.nd_logdet(f, vals)
        assert ld.dtype == torch.float64 and ld.dim() == 0 and ld.is_cuda
        assert abs(ld.item() - np.linalg.slogdet(sym_of(name, dtype, 1))[1]) <= TOL[dtype] * max(1.0, abs(ld.item()))
        ld.backward()
        got = vals.grad.cpu().numpy()
        assert got.dtype == np.dtype(dtype)
        print(f"{name} {np.dtype(dtype).name} logdet grad_vals {rel_err(got, ld_want):.3e}")
        assert rel_err(got, ld_want) <= TOL[dtype]
        assert (got[upper] == 0).all()
        for k in (1, 3, 33):
            b, g = rhs(name, k, dtype, 40 + k), rhs(name, k, dtype, 50 + k)
            gv_want, gb_want = solve_grads(name, dtype, b, g)
            # nd_solve alone
            vals, bt = leaf(v2), leaf(b)
            x = autograd.nd_solve(f, vals, bt)
            assert x.shape == bt.shape
            assert rel_err(x.detach().cpu().numpy(), inverse(name, dtype) @ b.astype(np.float64)) <= TOL[dtype]
            (dev(g) * x).sum().backward()
            ev, eb = rel_err(vals.grad.cpu().numpy(), gv_want), rel_err(bt.grad.cpu().numpy(), gb_want)
            print(f"{name} {np.dtype(dtype).name} k={k} solve grad_vals {ev:.3e} grad_b {eb:.3e}")
            assert ev <= TOL[dtype] and eb <= TOL[dtype]
            assert (vals.grad[dev(upper)] == 0).all()
            # the sum, the factor of the first call used again by the second
            vals, bt = leaf(v2), leaf(b)
            x = autograd.nd_solve(f, vals, bt)
            loss = (dev(g) * x).sum() + 0.7 * autograd.nd_logdet(f, vals, refactor=False)
            loss.backward()
            ev = rel_err(vals.grad.cpu().numpy(), gv_want + 0.7 * ld_want)
            eb = rel_err(bt.grad.cpu().numpy(), gb_want)
            print(f"{name} {np.dtype(dtype).name} k={k} sum grad_vals {ev:.3e} grad_b {eb:.3e}")
            assert ev <= TOL[dtype] and eb <= TOL[dtype]
            assert (vals.grad[dev(upper)] == 0).all()


def test_gradcheck(monkeypatch):
    """torch's own check, its default eps / atol / rtol, n = 25. gradcheck runs one forward, then some hundred
    perturbed forwards, then the first forward's backward: with one shared factor that backward is (rightly)
    refused as stale, so every forward gets a factor of its own, which its graph keeps alive."""
    import torch

    from basic_sparse_matrix_amd import autograd

    name = "g5-leaf1"
    setup(monkeypatch, name, F64)
    A = matrix(name, F64)
    vals, b = leaf(_values(name)[1]), leaf(rhs(name, 2, F64, 9))
    made = []

    def factor():
        made.append(cholesky_nd(A))
        return made[-1]

    try:
        assert torch.autograd.gradcheck(lambda v, r: autograd.nd_solve(factor(), v, r), (vals, b))
        assert torch.autograd.gradcheck(lambda v: autograd.nd_logdet(factor(), v), (vals,))
    finally:
        for f in made:
            f.close()
    with cholesky_nd(A) as f:  # and the refusal that makes this necessary
        with pytest.raises(RuntimeError, match="rewritten between forward and backward"):
            torch.autograd.gradcheck(lambda v: autograd.nd_logdet(f, v), (vals,))


# ---- guards -----------------------------------------------------------------


def test_backward_after_a_rewrite_is_refused(monkeypatch):
    from basic_sparse_matrix_amd import autograd

    name = "g5-leaf1"
    setup(monkeypatch, name, F64)
    with cholesky_nd(matrix(name, F64)) as f:
        vals, b = leaf(_values(name)[0]), leaf(rhs(name, 1, F64, 1))
        x = autograd.nd_solve(f, vals, b)
        ld = autograd.nd_logdet(f, vals, refactor=False)
        f.refactor(matrix(name, F64, 1))
        with pytest.raises(RuntimeError, match="rewritten between forward and backward"):
            x.sum().backward()
        with pytest.raises(RuntimeError, match="rewritten between forward and backward"):
            ld.backward()
        assert vals.grad is None and b.grad is None


def test_refactor_false_needs_the_factor_of_these_values(monkeypatch):
    import torch

    from basic_sparse_matrix_amd import autograd

    name = "g5-leaf1"
    setup(monkeypatch, name, F64)
    with cholesky_nd(matrix(name, F64)) as f:
        vals, other, b = leaf(_values(name)[0]), leaf(_values(name)[1]), leaf(rhs(name, 1, F64, 1))
        with pytest.raises(ValueError, match="refactor=False"):  # cholesky_nd recorded no tensor
            autograd.nd_solve(f, vals, b, refactor=False)
        f.refactor_values(vals.detach())  # the same storage and version as vals
        autograd.nd_solve(f, vals, b, refactor=False)
        autograd.nd_logdet(f, vals, refactor=False)
        with pytest.raises(ValueError, match="refactor=False"):
            autograd.nd_solve(f, other, b, refactor=False)
        with pytest.raises(ValueError, match="refactor=False"):
            autograd.nd_logdet(f, other, refactor=False)
        with torch.no_grad():
            vals.mul_(1.0)  # an in-place edit, whatever it writes
        with pytest.raises(ValueError, match="refactor=False"):
            autograd.nd_solve(f, vals, b, refactor=False)
        autograd.nd_solve(f, vals, b)
        autograd.nd_logdet(f, vals, refactor=False)
        f.refactor(matrix(name, F64))  # the factor is rewritten: the record is void
        with pytest.raises(ValueError, match="refactor=False"):
            autograd.nd_logdet(f, vals, refactor=False)


def test_the_record_keeps_its_address(monkeypatch):
    """The factor holds the recorded values: freed by the caller, their address cannot pass to a new tensor of
    other values that refactor=False would then take for them. A rewrite or close() lets go of them."""
    import torch

    from basic_sparse_matrix_amd import autograd

    name = "g5-leaf1"
    setup(monkeypatch, name, F64)
    with cholesky_nd(matrix(name, F64)) as f:
        vals, b = dev(_values(name)[0]), dev(rhs(name, 1, F64, 1))
        autograd.nd_solve(f, vals, b)
        ptr = vals.data_ptr()
        assert f._vals_key[0] == ptr and f._vals_ref.data_ptr() == ptr
        del vals
        other = dev(_values(name)[1])  # the same size: the allocator would hand out a freed block again
        assert other.data_ptr() != ptr
        with pytest.raises(ValueError, match="refactor=False"):
            autograd.nd_logdet(f, other, refactor=False)
        f.refactor(matrix(name, F64))
        assert f._vals_key is None and f._vals_ref is None
        autograd.nd_logdet(f, leaf(_values(name)[0])).backward()
        assert f._grad_weights is not None and f._vals_ref is not None
    assert f._grad_weights is None and f._vals_ref is None and f._vals_key is None


def test_wrapper_checks_on_device_tensors(monkeypatch):
    """nd_factor_sddmm's and inv_pattern's own shape, k and contiguity checks, with tensors that ARE on the device."""
    import torch

    from basic_sparse_matrix_amd import device

    name = "g5-leaf1"
    n, _ = setup(monkeypatch, name, F64)
    with cholesky_nd(matrix(name, F64)) as f:
        nnz = f.pattern_nnz
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")  # noqa: E731
        with pytest.raises(ValueError, match="k == 0"):
            device.nd_factor_sddmm(f, z(n, 0), z(n, 0))
        with pytest.raises(ValueError, match="u must be"):
            device.nd_factor_sddmm(f, z(n + 1, 2), z(n + 1, 2))
        with pytest.raises(ValueError, match="v must be"):
            device.nd_factor_sddmm(f, z(n, 2), z(n, 2, 1))
        with pytest.raises(ValueError, match="u has 2 columns, v 1"):
            device.nd_factor_sddmm(f, z(n, 2), z(n))
        with pytest.raises(ValueError, match="out must be"):
            device.nd_factor_sddmm(f, z(n, 2), z(n, 2), out=z(nnz + 1))
        with pytest.raises(ValueError, match="must be contiguous"):
            device.nd_factor_sddmm(f, z(n, 4)[:, ::2], z(n, 2))
        with pytest.raises(TypeError):
            device.nd_factor_sddmm(f, z(n, 2), z(n, 2).float())
        with pytest.raises(ValueError, match="out must be contiguous"):
            device.nd_factor_inv_pattern(f, out=z(2 * nnz)[::2])
        with pytest.raises(TypeError):
            device.nd_factor_inv_pattern(f, out=z(nnz).float())
        got = device.nd_factor_sddmm(f, z(n) + 1.0, z(n) + 3.0)  # (n,) counts as k = 1
        _, rows, cols = pattern(name)
        assert np.array_equal(got.cpu().numpy(), np.where(cols < rows, 6.0, np.where(cols == rows, 3.0, 0.0)))


def test_grad_of_b_alone_leaves_the_sddmm_out(monkeypatch):
    from basic_sparse_matrix_amd import autograd, device

    name = "g11-leaf8"
    setup(monkeypatch, name, F64)
    calls = []
    real = device.nd_factor_sddmm
    monkeypatch.setattr(device, "nd_factor_sddmm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with cholesky_nd(matrix(name, F64)) as f:
        b_np, g = rhs(name, 3, F64, 3), rhs(name, 3, F64, 4)
        vals, b = dev(_values(name)[1]), leaf(b_np)
        (dev(g) * autograd.nd_solve(f, vals, b)).sum().backward()
        assert not calls and vals.grad is None
        assert rel_err(b.grad.cpu().numpy(), solve_grads(name, F64, b_np, g)[1]) <= TOL[F64]
        vals = leaf(_values(name)[1])
        (dev(g) * autograd.nd_solve(f, vals, b.detach())).sum().backward()
        assert calls == [1] and vals.grad is not None


def test_f32_factor_of_an_f64_matrix_is_refused(monkeypatch):
    from basic_sparse_matrix_amd import autograd

    name = "g5-leaf1"
    setup(monkeypatch, name, F32)
    with cholesky_nd(matrix(name, F64), factor_dtype=F32) as f:
        with pytest.raises(TypeError, match="not differentiable in this version"):
            autograd.nd_solve(f, leaf(_values(name)[0]), dev(rhs(name, 1, F32, 1)))
        with pytest.raises(TypeError, match="not differentiable in this version"):
            autograd.nd_logdet(f, leaf(_values(name)[0]))
