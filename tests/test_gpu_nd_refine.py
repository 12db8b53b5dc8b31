"""GPU tests of the mixed-precision use of a kept nd factor: a factor whose
dtype is chosen (cholesky_nd(a, factor_dtype=...), bsm_nd_factor_create_as)
and iterative refinement on it (NdFactor.solve_refined,
device.nd_factor_solve_refined).

The systems are nd_support.py's, the smallest
that hit one-pivot fronts (g5-leaf1), several levels (g11-leaf8), multi-tile
fronts (g40-leaf256), fronts without pivots (blocks) and an irregular tree
(random); the right-hand sides are orc.gen_x_cols(2001, n, 3).

Bounds. The default tol is (m + 2) 2^-53, m the longest row of the mirrored
matrix S: the rounding bound of the f64 residual. berr is held to it; omega
recomputed here from a longdouble residual is held to twice it (the device's
own residual carries that rounding); the forward errors to the nd files' f64
TOL = 1e-10, and for f32 data to 2^-23 of max |x| (the rounding of x itself,
2^-24, and as much again for the refined f64 iterate's own error)."""

import functools

import numpy as np
import pytest

from basic_sparse_matrix_amd import Csr, Dense, _lib, cholesky_nd
from nd_support import (assert_same, cols_of, coords, csr_parts, default_tol, matrix, omega_np, rel_err, rhs, rhs_cols,
                        same_bits, setup, sym_dense, system)

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 2e-3}
POISSON = ["g5-leaf1", "g11-leaf8", "g40-leaf256"]
SYSTEMS = POISSON + ["blocks", "random"]
F32, F64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def _truth(name, dtype):
    """(S, tol, the f64 solutions of S x = b) for the system's values and right-hand sides rounded to dtype."""
    S = sym_dense(name, system(name)[3].astype(dtype))
    B = np.stack([c.astype(dtype).astype(np.float64) for c in rhs_cols(name)], axis=1)
    return S, default_tol(S), np.linalg.solve(S, B)


def result_parts(x, info):
    return cols_of(x) + [info.iters, info.berr]


# ---- a factor whose dtype is chosen ----------------------------------------------


@pytest.mark.parametrize("name", SYSTEMS)
def test_f32_factor_refines_an_f64_system_to_f64_accuracy(monkeypatch, name):
    setup(monkeypatch, name)
    S, tol, xt = _truth(name, F64)
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        assert f.dtype == np.dtype(F32)
        x, info = f.solve_refined(A, rhs(name, F64))
    assert x.dtype == np.dtype(F64) and info.tol == tol
    for j, xj in enumerate(cols_of(x)):
        w = omega_np(S, xj, rhs_cols(name)[j])
        e = rel_err(xj, xt[:, j])
        print(f"{name} column {j}: iters {info.iters[j]} berr {info.berr[j]:.3e} omega {w:.3e} rel_err {e:.3e}")
        assert info.converged[j] and info.iters[j] <= 3
        assert info.berr[j] <= tol
        assert w <= 2 * tol
        assert e <= TOL[F64]


@pytest.mark.parametrize("name", ["g11-leaf8", "g40-leaf256", "random"])
def test_f32_factor_of_f64_values_has_the_bits_of_the_f32_matrixs(monkeypatch, name):
    setup(monkeypatch, name)
    with cholesky_nd(matrix(name, F64), factor_dtype=F32) as f, cholesky_nd(matrix(name, F32)) as g:
        assert f.dtype == g.dtype == np.dtype(F32)
        assert_same(csr_parts(f.l()), csr_parts(g.l()))
    with cholesky_nd(matrix(name, F64), factor_dtype=F64) as f, cholesky_nd(matrix(name, F64)) as g:
        assert_same(csr_parts(f.l()), csr_parts(g.l()))  # the matrix's own dtype: plain create


def test_f32_factor_has_half_the_bytes(monkeypatch):
    setup(monkeypatch, "g40-leaf256")
    A = matrix("g40-leaf256", F64)
    with cholesky_nd(A, factor_dtype=F32) as f, cholesky_nd(A) as g:
        assert f.nbytes > 0 and 2 * f.nbytes == g.nbytes


def test_refactor_converts_and_keeps_the_source_dtype(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    n, _, _, v, _ = system(name)
    r, c = coords(name)
    d = 1.0 + np.random.default_rng(11).random(n)
    v2 = d[r] * v * d[c]  # A2 = D A D
    b = rhs(name, F32)
    with cholesky_nd(matrix(name, F64), factor_dtype=F32) as f, \
            cholesky_nd(matrix(name, F64, v2), factor_dtype=F32) as fresh:
        f.refactor(matrix(name, F64, v2))
        want = csr_parts(fresh.l()) + cols_of(fresh.solve(b))
        assert_same(csr_parts(f.l()) + cols_of(f.solve(b)), want)
        with pytest.raises(_lib.BsmError, match="dtype differs.*f64 was factored.*f32"):
            f.refactor(matrix(name, F32, v2))
        assert_same(csr_parts(f.l()) + cols_of(f.solve(b)), want)  # untouched


# ---- the refined solve ---------------------------------------------------------------


@pytest.mark.parametrize("name", POISSON)
def test_f32_system_is_solved_to_the_rounding_of_x(monkeypatch, name):
    setup(monkeypatch, name)
    _, _, xt = _truth(name, F32)
    A = matrix(name, F32)
    with cholesky_nd(A) as f:
        x, info = f.solve_refined(A, rhs(name, F32))
        plain = f.solve(rhs(name, F32))
    assert x.dtype == np.dtype(F32)
    for j, xj in enumerate(cols_of(x)):
        e = np.abs(xj.astype(np.float64) - xt[:, j]).max() / np.abs(xt[:, j]).max()
        ep = rel_err(plain.get_col(j), xt[:, j])
        print(f"{name} column {j}: iters {info.iters[j]} berr {info.berr[j]:.3e} max err {e:.3e} (plain solve {ep:.3e})")
        assert info.converged[j]
        assert e <= 2.0 ** -23
        assert ep < TOL[F32]


@pytest.mark.parametrize("name", SYSTEMS)
def test_f64_factor_converges_in_one_correction(monkeypatch, name):
    setup(monkeypatch, name)
    S, tol, xt = _truth(name, F64)
    A = matrix(name, F64)
    with cholesky_nd(A) as f:
        x, info = f.solve_refined(A, rhs(name, F64))
    print(name, info)
    assert info.converged.all() and (info.iters <= 1).all() and (info.berr <= tol).all()
    for j, xj in enumerate(cols_of(x)):
        assert rel_err(xj, xt[:, j]) <= TOL[F64]


@pytest.mark.parametrize("name,dtype", [("g11-leaf8", F64), ("g40-leaf256", F32), ("g5-leaf1", F32)])
def test_no_correction_is_the_plain_solve(monkeypatch, name, dtype):
    setup(monkeypatch, name)
    S, _, _ = _truth(name, dtype)
    A = matrix(name, dtype)
    b = rhs(name, dtype)
    with cholesky_nd(A) as f:
        x, info = f.solve_refined(A, b, max_iter=0)
        assert_same(cols_of(x), cols_of(f.solve(b)))
    assert (info.iters == 0).all()
    for j, xj in enumerate(cols_of(x)):
        w = omega_np(S, xj, b.get_col(j).astype(np.float64))
        print(f"{name} {np.dtype(dtype).name} column {j}: berr {info.berr[j]:.6e} numpy {w:.6e}")
        if dtype == F32:  # omega ~ 1e-7, far above the f64 residual's rounding
            assert abs(info.berr[j] - w) <= 1e-6 * w


@pytest.mark.parametrize("name", ["g40-leaf256", "random"])
def test_columns_are_independent_and_calls_repeat(monkeypatch, name):
    setup(monkeypatch, name)
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        x3, i3 = f.solve_refined(A, rhs(name, F64))
        again = f.solve_refined(A, rhs(name, F64))
        assert_same(result_parts(x3, i3), result_parts(*again))
        for j in range(3):
            x1, i1 = f.solve_refined(A, Dense.from_columns([rhs_cols(name)[j]]))
            assert same_bits(x1.get_col(0), x3.get_col(j)), j
            assert i1.iters[0] == i3.iters[j] and same_bits(i1.berr[:1], i3.berr[j:j + 1]), j


def test_stale_factor(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    n, _, _, v, _ = system(name)
    r, c = coords(name)
    v2 = v + 0.01 * (r == c)  # A + 0.01 I on A's factor
    S = sym_dense(name, v2)
    A2 = matrix(name, F64, v2)
    b = rhs(name, F64)
    xt = np.linalg.solve(S, np.stack(rhs_cols(name), axis=1))
    with cholesky_nd(matrix(name, F64)) as f:
        x, info = f.solve_refined(A2, b, max_iter=30)
        print(info)
        assert info.converged.all() and (info.iters >= 5).all() and (info.iters <= 20).all()
        for j, xj in enumerate(cols_of(x)):
            assert rel_err(xj, xt[:, j]) <= TOL[F64]
        upto = [f.solve_refined(A2, b, max_iter=i) for i in range(4)]
    x3, i3 = upto[3]
    assert not i3.converged.any() and (i3.iters == 3).all()
    for j in range(3):
        seen = [omega_np(S, np.asarray(xi.get_col(j)), rhs_cols(name)[j]) for xi, _ in upto]
        print(f"column {j}: berr {i3.berr[j]:.6e}, the four iterates' omega {seen}")
        assert abs(i3.berr[j] - min(seen)) <= 1e-6 * min(seen)
        assert i3.berr[j] < upto[0][1].berr[j]


def test_divergence_keeps_the_best_iterate(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    A3 = matrix(name, F64, 3.0 * system(name)[3])
    b = rhs(name, F64)
    with cholesky_nd(matrix(name, F64)) as f:
        x0, i0 = f.solve_refined(A3, b, max_iter=0)
        x, info = f.solve_refined(A3, b)
    assert (info.iters == 1).all() and not info.converged.any()
    assert_same(cols_of(x), cols_of(x0))
    assert same_bits(info.berr, i0.berr)


def test_the_upper_triangle_is_ignored(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    r, c = coords(name)
    v = system(name)[3]
    junk = np.where(c > r, 1e6 * (1.0 + np.arange(v.size)), v)
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        want = result_parts(*f.solve_refined(A, rhs(name, F64)))
        assert_same(result_parts(*f.solve_refined(matrix(name, F64, junk), rhs(name, F64))), want)


def test_edge_cases(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    n = system(name)[0]
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        # a zero column beside a real one
        x, info = f.solve_refined(A, Dense.from_columns([rhs_cols(name)[0], np.zeros(n)]))
        assert not np.asarray(x.get_col(1)).any() and info.berr[1] == 0.0 and info.iters[1] == 0 and info.converged[1]
        x1, i1 = f.solve_refined(A, Dense.from_columns([rhs_cols(name)[0]]))
        assert same_bits(x.get_col(0), x1.get_col(0)) and info.iters[0] == i1.iters[0]
        x0, i0 = f.solve_refined(A, Dense(0, n, []))  # k = 0
        assert x0.get_dims().cols == 0 and i0.iters.size == 0 and i0.berr.size == 0
        bad = system(name)[3].copy()
        r, c = coords(name)
        e = int(np.nonzero((r == n // 2) & (c == n // 2))[0][0])
        bad[e] = -bad[e]
        with pytest.raises(_lib.BsmError):
            f.refactor(matrix(name, F64, bad))  # not positive definite: the handle holds no factor
        with pytest.raises(_lib.BsmError, match="refactor first"):
            f.solve_refined(A, rhs(name, F64))
    E = Csr.from_csr_arrays((0, 0), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0))
    with cholesky_nd(E, factor_dtype=F32) as f:  # n = 0
        x, info = f.solve_refined(E, Dense.from_columns([np.zeros(0)]))
        assert x.get_dims().cols == 1 and x.get_col(0).size == 0 and info.iters[0] == 0 and info.berr[0] == 0.0


@pytest.mark.parametrize("env", [{"BSM_ND_FWD_TILES": "1", "BSM_ND_BWD_TILES": "1"}, {"BSM_ND_PLAIN": "1"}],
                         ids=["tiles", "plain"])
def test_device_call_has_the_host_calls_bits(monkeypatch, env):
    import torch

    from basic_sparse_matrix_amd import device

    name = "g40-leaf256"
    setup(monkeypatch, name)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        want = result_parts(*f.solve_refined(A, rhs(name, F64)))
        b = torch.from_numpy(np.stack(rhs_cols(name), axis=1)).cuda().contiguous()
        out, info = device.nd_factor_solve_refined(f, A, b)
        got = out.cpu().numpy()
        assert_same([np.ascontiguousarray(got[:, j]) for j in range(3)] + [info.iters, info.berr], want)
        same, info2 = device.nd_factor_solve_refined(f, A, b, out=b)  # in place
        assert same is b
        assert_same([np.ascontiguousarray(b.cpu().numpy()[:, j]) for j in range(3)] + [info2.iters, info2.berr], want)
        b1 = torch.from_numpy(rhs_cols(name)[1].copy()).cuda()  # (n,): one column
        out1, info1 = device.nd_factor_solve_refined(f, A, b1)
        assert same_bits(out1.cpu().numpy(), want[1]) and info1.iters[0] == want[3][1]
