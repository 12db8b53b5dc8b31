"""GPU tests of preconditioned conjugate gradients on a kept nd factor
(NdFactor.solve_pcg, device.nd_factor_solve_pcg, bsm_nd_factor_solve_pcg).

The systems are nd_support.py's, as in test_gpu_nd_refine.py: one-pivot fronts
(g5-leaf1), several levels (g11-leaf8), multi-tile fronts (g40-leaf256), fronts
without pivots (blocks) and an irregular tree (random); the right-hand sides
are orc.gen_x_cols(2001, n, 3).

Bounds. The default tol is (m + 2) 2^-53, m the longest row of the mirrored
matrix S: the rounding bound of the f64 residual. berr (the backward error of
the TRUE residual of the returned x) is held to it; omega recomputed here from
a longdouble residual to twice it (the device's own residual carries that
rounding); the forward error to the nd files' f64 TOL = 1e-10. The step counts
are held to this file's own numpy emulation of the loop, with
np.linalg.cholesky in the factor's dtype as M, plus 2: the nd factor sums in
another order than the dense one, so an f32 preconditioner's rounding differs,
and two steps is the slack the emulation shows between its own f64 and f32
runs of 3A."""

import functools

import numpy as np
import pytest

from basic_sparse_matrix_amd import Csr, Dense, MatErr, PcgInfo, _lib, cholesky_nd
from nd_support import (_scale, assert_same, cols_of, coords, default_tol, matrix, omega_np, rel_err, rhs, rhs_cols,
                        same_bits, setup, sym_dense, system)

pytestmark = pytest.mark.gpu

TOL = 1e-10
SYSTEMS = ["g5-leaf1", "g11-leaf8", "g40-leaf256", "blocks", "random"]
F32, F64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def _truth(name, variant="A"):
    """(values, S, tol, the f64 solutions of S x = b) of a variant of the system's matrix."""
    v = variant_values(name, variant)
    S = sym_dense(name, v)
    return v, S, default_tol(S), np.linalg.solve(S, np.stack(rhs_cols(name), axis=1))


def variant_values(name, variant):
    n, _, _, v, _ = system(name)
    r, c = coords(name)
    if variant == "A":
        return v
    if variant == "3A":
        return 3.0 * v
    if variant == "A/2":
        return 0.5 * v
    if variant == "diag40":  # A + 40 e_i e_i^T at three nodes: a rank-3 change
        return v + 40.0 * ((r == c) & np.isin(r, [1, n // 2, n - 2]))
    if variant == "A+0.01I":
        return v + 0.01 * (r == c)
    if variant == "-A":
        return -v
    raise KeyError(variant)


def result_parts(x, info):
    return cols_of(x) + [info.iters, info.berr, info.breakdown]


def assert_solved(name, variant, x, info, what):
    """The bounds of a converged solve: berr <= tol, longdouble omega <= 2 tol, rel_err <= 1e-10."""
    _, S, tol, xt = _truth(name, variant)
    assert isinstance(info, PcgInfo) and info.tol == tol and x.dtype == np.dtype(F64)
    for j, xj in enumerate(cols_of(x)):
        w = omega_np(S, xj, rhs_cols(name)[j])
        e = rel_err(xj, xt[:, j])
        print(f"{what} {name} {variant} column {j}: iters {info.iters[j]} berr {info.berr[j]:.3e} "
              f"omega {w:.3e} rel_err {e:.3e}")
        assert info.converged[j] and not info.breakdown[j]
        assert info.berr[j] <= tol
        assert w <= 2 * tol
        assert e <= TOL


# ---- the loop, emulated: np.linalg.cholesky in the factor's dtype stands for M -----------


@functools.lru_cache(maxsize=None)
def emulated_iters(name, variant, fdtype, max_iter=30):
    """The CG steps each column takes in a numpy run of the library's loop."""
    from scipy.linalg import solve_triangular

    _, S, tol, _ = _truth(name, variant)
    Lf = np.linalg.cholesky(sym_dense(name, system(name)[3]).astype(fdtype))
    snorm = np.abs(S).sum(axis=1).max()

    def minv(v):
        s = _scale(v)
        w = (v / s).astype(fdtype)
        y = solve_triangular(Lf, w, lower=True)
        return s * solve_triangular(Lf.T, y, lower=False).astype(np.float64)

    out = []
    for b in rhs_cols(name):
        bn = np.abs(b).max()

        def omega(r, x):
            return np.abs(r).max() / (snorm * np.abs(x).max() + bn)

        x = minv(b)
        r = b - S @ x
        it = 0
        if omega(r, x) > tol:
            z = minv(r)
            p = z.copy()
            rho = r @ z
            for it in range(1, max_iter + 1):
                q = S @ p
                alpha = rho / (p @ q)
                x = x + alpha * p
                r = r - alpha * q
                restart = False
                if omega(r, x) <= tol:
                    r = b - S @ x
                    if omega(r, x) <= tol:
                        break
                    restart = True
                z = minv(r)
                beta = 0.0 if restart else -alpha * (q @ z) / rho
                rho = r @ z
                p = z + beta * p
        out.append(it)
    return np.array(out)


# ---- convergence ---------------------------------------------------------------------------


@pytest.mark.parametrize("name", SYSTEMS)
def test_f32_factor_solves_an_f64_system_to_f64_accuracy(monkeypatch, name):
    setup(monkeypatch, name)
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        x, info = f.solve_pcg(A, rhs(name, F64))
    assert_solved(name, "A", x, info, "f32 factor")


@pytest.mark.parametrize("name", SYSTEMS)
def test_f64_factor_on_its_own_matrix_takes_at_most_one_step(monkeypatch, name):
    setup(monkeypatch, name)
    A = matrix(name, F64)
    with cholesky_nd(A) as f:
        x, info = f.solve_pcg(A, rhs(name, F64))
    assert_solved(name, "A", x, info, "f64 factor")
    assert (info.iters <= 1).all()


@pytest.mark.parametrize("fdtype", [F64, F32], ids=["f64-factor", "f32-factor"])
def test_what_refinement_cannot_do(monkeypatch, fdtype):
    """3A, A/2 and a rank-3 change of the diagonal on the factor of A: CG
    converges within the emulation's steps + 2, refinement reports failure on
    3A and on the diagonal change."""
    name = "g11-leaf8"
    setup(monkeypatch, name)
    with cholesky_nd(matrix(name, F64), factor_dtype=fdtype) as f:
        for variant in ("3A", "A/2", "diag40"):
            A2 = matrix(name, F64, variant_values(name, variant))
            x, info = f.solve_pcg(A2, rhs(name, F64), max_iter=30)
            assert_solved(name, variant, x, info, np.dtype(fdtype).name)
            emu = emulated_iters(name, variant, fdtype)
            print(f"{variant}: device iters {info.iters}, emulation {emu}")
            assert (info.iters <= emu + 2).all()
            if variant != "A/2":
                _, refined = f.solve_refined(A2, rhs(name, F64), max_iter=30)
                print(f"{variant}: solve_refined iters {refined.iters} berr {refined.berr}")
                assert not refined.converged.any()


def test_stale_factor_takes_fewer_steps_than_refinement(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    A2 = matrix(name, F64, variant_values(name, "A+0.01I"))
    with cholesky_nd(matrix(name, F64)) as f:
        x, info = f.solve_pcg(A2, rhs(name, F64))
        _, refined = f.solve_refined(A2, rhs(name, F64), max_iter=30)
    assert_solved(name, "A+0.01I", x, info, "stale")
    print(f"pcg iters {info.iters}, solve_refined iters {refined.iters}")
    assert refined.converged.all()
    assert (info.iters < refined.iters).all()


# ---- bits ----------------------------------------------------------------------------------


@pytest.mark.parametrize("name,dtype,fdtype", [("g11-leaf8", F64, F64), ("g40-leaf256", F32, F32),
                                               ("g5-leaf1", F32, F32), ("g11-leaf8", F64, F32)])
def test_no_step_is_the_refined_solves_first_iterate(monkeypatch, name, dtype, fdtype):
    setup(monkeypatch, name)
    A = matrix(name, dtype)
    b = rhs(name, dtype)
    with cholesky_nd(A, factor_dtype=fdtype) as f:
        x, info = f.solve_pcg(A, b, max_iter=0)
        xr, ir = f.solve_refined(A, b, max_iter=0)
    assert x.dtype == np.dtype(dtype) and (info.iters == 0).all() and not info.breakdown.any()
    assert_same(cols_of(x) + [info.berr], cols_of(xr) + [ir.berr])


@pytest.mark.parametrize("name", ["g40-leaf256", "random"])
def test_columns_are_independent_and_calls_repeat(monkeypatch, name):
    """A/2 on the f32 factor of A, so that several steps run."""
    setup(monkeypatch, name)
    n = system(name)[0]
    A2 = matrix(name, F64, variant_values(name, "A/2"))
    with cholesky_nd(matrix(name, F64), factor_dtype=F32) as f:
        x3, i3 = f.solve_pcg(A2, rhs(name, F64))
        print(name, i3)
        assert i3.converged.all() and (i3.iters >= 2).all()
        assert_same(result_parts(x3, i3), result_parts(*f.solve_pcg(A2, rhs(name, F64))))
        for j in range(3):
            x1, i1 = f.solve_pcg(A2, Dense.from_columns([rhs_cols(name)[j]]))
            assert same_bits(x1.get_col(0), x3.get_col(j)), j
            assert i1.iters[0] == i3.iters[j] and same_bits(i1.berr[:1], i3.berr[j:j + 1]), j
        xz, iz = f.solve_pcg(A2, Dense.from_columns([np.zeros(n), rhs_cols(name)[0]]))  # beside a zero column
        assert not np.asarray(xz.get_col(0)).any() and iz.iters[0] == 0 and iz.berr[0] == 0.0 and iz.converged[0]
        assert same_bits(xz.get_col(1), x3.get_col(0)) and iz.iters[1] == i3.iters[0]
        assert same_bits(iz.berr[1:], i3.berr[:1])


@pytest.mark.parametrize("name", ["g40-leaf256", "random"])
def test_a_column_beside_one_that_converges_at_x0(monkeypatch, name):
    """No right-hand side but 0 converges at x_0 on A/2, or on any S with an f32
    factor (x_0 carries the f32 solve's 1e-7). So this case has the f64 factor
    of A and the rank-3 diagonal change: b = A y with y zero at the changed
    nodes is solved by x_0 = A^-1 b up to the solve's own error at those nodes
    (cond(A) 2^-53, hence tol = 1e-12 for both columns), while the other
    column takes steps."""
    setup(monkeypatch, name)
    n = system(name)[0]
    v = variant_values(name, "diag40")
    y = np.array(rhs_cols(name)[2])
    y[[1, n // 2, n - 2]] = 0.0
    b0 = sym_dense(name, system(name)[3]) @ y
    A2 = matrix(name, F64, v)
    with cholesky_nd(matrix(name, F64)) as f:
        x, info = f.solve_pcg(A2, Dense.from_columns([b0, rhs_cols(name)[0]]), tol=1e-12)
        x1, i1 = f.solve_pcg(A2, Dense.from_columns([rhs_cols(name)[0]]), tol=1e-12)
        xs, js = f.solve_pcg(A2, Dense.from_columns([rhs_cols(name)[0], b0]), tol=1e-12)
    print(name, info, i1)
    assert info.converged.all() and info.iters[0] == 0 and info.iters[1] >= 2
    assert same_bits(x.get_col(1), x1.get_col(0)) and info.iters[1] == i1.iters[0]
    assert same_bits(info.berr[1:], i1.berr)
    assert_same(cols_of(xs)[::-1] + [js.iters[::-1], js.berr[::-1]], cols_of(x) + [info.iters, info.berr])


def test_breakdown_on_a_negative_definite_system(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    Aneg = matrix(name, F64, variant_values(name, "-A"))
    with cholesky_nd(matrix(name, F64)) as f:
        x, info = f.solve_pcg(Aneg, rhs(name, F64))
    print(info)
    assert info.breakdown.all() and not info.converged.any() and (info.iters <= 1).all()
    assert all(np.isfinite(c).all() for c in cols_of(x))


def test_the_upper_triangle_is_ignored(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    r, c = coords(name)
    v = variant_values(name, "A/2")
    junk = np.where(c > r, 1e6 * (1.0 + np.arange(v.size)), v)
    with cholesky_nd(matrix(name, F64), factor_dtype=F32) as f:
        want = result_parts(*f.solve_pcg(matrix(name, F64, v), rhs(name, F64)))
        assert_same(result_parts(*f.solve_pcg(matrix(name, F64, junk), rhs(name, F64))), want)


def test_edge_cases(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    n = system(name)[0]
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        # a zero column beside a real one
        x, info = f.solve_pcg(A, Dense.from_columns([rhs_cols(name)[0], np.zeros(n)]))
        assert not np.asarray(x.get_col(1)).any() and info.berr[1] == 0.0 and info.iters[1] == 0
        assert info.converged[1] and not info.breakdown[1]
        x1, i1 = f.solve_pcg(A, Dense.from_columns([rhs_cols(name)[0]]))
        assert same_bits(x.get_col(0), x1.get_col(0)) and info.iters[0] == i1.iters[0]
        x0, i0 = f.solve_pcg(A, Dense(0, n, []))  # k = 0
        assert x0.get_dims().cols == 0 and i0.iters.size == 0 and i0.berr.size == 0 and i0.breakdown.size == 0
        with pytest.raises(MatErr, match="IncorrectDimensions"):
            f.solve_pcg(A, Dense.from_columns([np.zeros(n + 1)]))
        with pytest.raises(MatErr, match="IncorrectDimensions"):
            f.solve_pcg(matrix("g5-leaf1", F64), rhs(name, F64))
        with pytest.raises(TypeError):
            f.solve_pcg(A, rhs(name, F32))
        with pytest.raises(TypeError):
            f.solve_pcg(matrix(name, np.int32, np.ones(system(name)[3].size)), rhs(name, F64))
        bad = system(name)[3].copy()
        r, c = coords(name)
        e = int(np.nonzero((r == n // 2) & (c == n // 2))[0][0])
        bad[e] = -bad[e]
        with pytest.raises(_lib.BsmError):
            f.refactor(matrix(name, F64, bad))  # not positive definite: the handle holds no factor
        with pytest.raises(_lib.BsmError, match="refactor first"):
            f.solve_pcg(A, rhs(name, F64))
    E = Csr.from_csr_arrays((0, 0), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0))
    with cholesky_nd(E, factor_dtype=F32) as f:  # n = 0
        x, info = f.solve_pcg(E, Dense.from_columns([np.zeros(0)]))
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
    A2 = matrix(name, F64, variant_values(name, "A/2"))
    with cholesky_nd(matrix(name, F64), factor_dtype=F32) as f:
        want = result_parts(*f.solve_pcg(A2, rhs(name, F64)))
        assert (want[3] >= 2).all()  # steps were made
        b = torch.from_numpy(np.stack(rhs_cols(name), axis=1)).cuda().contiguous()
        out, info = device.nd_factor_solve_pcg(f, A2, b)
        got = out.cpu().numpy()
        assert_same([np.ascontiguousarray(got[:, j]) for j in range(3)] + [info.iters, info.berr, info.breakdown], want)
        same, info2 = device.nd_factor_solve_pcg(f, A2, b, out=b)  # in place
        assert same is b
        assert_same([np.ascontiguousarray(b.cpu().numpy()[:, j]) for j in range(3)]
                    + [info2.iters, info2.berr, info2.breakdown], want)
        b1 = torch.from_numpy(rhs_cols(name)[1].copy()).cuda()  # (n,): one column
        out1, info1 = device.nd_factor_solve_pcg(f, A2, b1)
        assert same_bits(out1.cpu().numpy(), want[1]) and info1.iters[0] == want[3][1]
        assert same_bits(info1.berr, want[4][1:2])
