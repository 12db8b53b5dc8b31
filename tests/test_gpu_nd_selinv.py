"""GPU tests of the kept nd factor's selected inverse (NdFactor.inv_diag /
inv_entries / inv_on, device.nd_factor_inv_diag): Z = A^-1 on the pattern of
L + L^T by the Takahashi recursion over the fronts.

The systems are nd_support.py's, the ones test_gpu_nd_factor_ops.py runs: the
smallest that reach each structure: one-pivot fronts with 63 padding pivots (g5-leaf1), a single
dense front of two pivot tiles (g11-onefront), several levels with a parent
more than one level above a child (g40-leaf64), leaves of several pivot tiles
(g40-leaf256), fronts with np = 0 (blocks), an irregular tree (random); f64 on
all of them, f32 on the Poisson ones. n <= 1600, so numpy.linalg.inv of the
dense matrix in f64 is the reference.

Accuracy is held against a yardstick measured in the same test: with
err(X) = max|X - Zref| / max|Zref| over the compared entries, the selected
inverse may be at most 8 times as far from Zref as the kept factor's own
f.solve(I) over all n unit columns is on the same entries. Both algorithms
are backward stable with errors of a few ulps of the scale; a CPU emulation
(scalar Takahashi against two triangular solves) gave ratios 0.5 - 1.25 on
these matrices in both dtypes, and 8 covers the other elimination order and
the MFMA accumulation without hiding a wrong tile. Measured on MI355X
(selinv / solve, worst of the three entry sets): see DESIGN.md §4.9e."""

import functools
import threading

import numpy as np
import pytest

import nd_support
from basic_sparse_matrix_amd import Csr, Dense, MatErr, MatErrKind, _lib, cholesky_nd
from nd_support import assert_same, cols_of, coords, dense_of, same_bits, setup, system

pytestmark = pytest.mark.gpu

POISSON = ["g5-leaf1", "g11-leaf8", "g11-onefront", "g40-leaf64", "g40-leaf256"]
SYSTEMS = POISSON + ["blocks", "random"]
CASES = [(s, np.float64) for s in SYSTEMS] + [(s, np.float32) for s in POISSON]
CASE_IDS = [f"{s}-{np.dtype(d).name}" for s, d in CASES]
FEW = [("g5-leaf1", np.float32), ("g11-onefront", np.float64), ("g40-leaf256", np.float64), ("blocks", np.float64)]
FEW_IDS = [f"{s}-{np.dtype(d).name}" for s, d in FEW]
MARGIN = 8.0


@functools.lru_cache(maxsize=None)
def _second_values(name):
    """A2 = D A D's values, d = 1 + rng.random(n): SPD with A; and A's with one diagonal entry negated."""
    n, _, _, v, _ = system(name)
    rows, cols = coords(name)
    d = 1.0 + np.random.default_rng(11).random(n)
    bad = v.copy()
    e = int(np.nonzero((rows == n // 2) & (cols == n // 2))[0][0])
    bad[e] = -bad[e]
    return d[rows] * v * d[cols], bad


@functools.lru_cache(maxsize=None)
def _zref(name, dtype):
    """inv(A) in f64 of the matrix as the factor sees it (its values rounded to dtype). Never modified."""
    n, rp, ci, v, _ = system(name)
    z = np.linalg.inv(dense_of(rp, ci, v.astype(dtype), n))
    z.setflags(write=False)
    return z


def matrix(name, dtype, which=0):
    return nd_support.matrix(name, dtype, None if which == 0 else _second_values(name)[which - 1])


def l_pairs(f):
    """Every stored position of L (new order) as pairs in A's order."""
    l = f.l()
    p = f.perm
    lrp = np.asarray(l.row_index).astype(np.int64)
    rows = np.repeat(np.arange(f.n), np.diff(lrp))
    return p[rows], p[np.asarray(l.col_index).astype(np.int64)]


def everything(f, name):
    """inv_diag, inv_on(A)'s values and the whole pattern of L through inv_entries."""
    li, lj = l_pairs(f)
    return [f.inv_diag(), np.asarray(f.inv_on(matrix(name, f.dtype)).v).copy(), f.inv_entries(li, lj)]


# ---- accuracy -------------------------------------------------------------------


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_accuracy_against_the_factors_own_solves(monkeypatch, name, dtype):
    setup(monkeypatch, name)
    n = system(name)[0]
    zref = _zref(name, dtype)
    scale = np.abs(zref).max()
    with cholesky_nd(matrix(name, dtype)) as f:
        eye = np.eye(n, dtype=dtype)
        xs = np.stack(cols_of(f.solve(Dense.from_columns([np.ascontiguousarray(eye[:, j]) for j in range(n)]))),
                      axis=1).astype(np.float64)  # xs[:, j] = A^-1 e_j
        d = f.inv_diag()
        assert d.dtype == np.dtype(dtype) and d.shape == (n,)
        ai, aj = coords(name)
        on = f.inv_on(matrix(name, dtype))
        assert on.dtype == np.dtype(dtype) and on.is_finalised
        assert np.array_equal(np.asarray(on.row_index), system(name)[1])
        assert np.array_equal(np.asarray(on.col_index), system(name)[2])
        li, lj = l_pairs(f)
        le = f.inv_entries(li, lj)
        assert le.dtype == np.dtype(dtype) and le.shape == li.shape
        idx = np.arange(n)
        for what, got, (i, j) in (("inv_diag", d, (idx, idx)), ("inv_on", np.asarray(on.v), (ai, aj)),
                                  ("inv_entries(L)", le, (li, lj))):
            err = np.abs(got.astype(np.float64) - zref[i, j]).max() / scale
            yard = np.abs(xs[i, j] - zref[i, j]).max() / scale
            print(f"{name} {np.dtype(dtype).name} {what}: selinv {err:.3e}, solve {yard:.3e}, "
                  f"ratio {err / yard if yard else float('inf'):.2f}")
            assert np.all(np.isfinite(got))
            assert err <= MARGIN * yard, what


# ---- the pattern ----------------------------------------------------------------


def test_one_dense_front_answers_every_pair(monkeypatch):
    name, dtype = "g11-onefront", np.float64
    setup(monkeypatch, name)
    n = system(name)[0]
    zref = _zref(name, dtype)
    i, j = (x.ravel() for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    with cholesky_nd(matrix(name, dtype)) as f:
        z = f.inv_entries(i, j).reshape(n, n)
    assert same_bits(z, np.ascontiguousarray(z.T))  # (i, j) and (j, i): the same bits
    assert np.abs(z - zref).max() / np.abs(zref).max() < 1e-12


def test_pairs_outside_the_pattern_and_out_of_bounds(monkeypatch):
    name, dtype = "g11-leaf8", np.float64
    setup(monkeypatch, name)
    n = system(name)[0]
    with cholesky_nd(matrix(name, dtype)) as f:
        li, lj = l_pairs(f)
        stored = np.zeros((n, n), dtype=bool)
        stored[li, lj] = stored[lj, li] = True
        oi, oj = (x[:3] for x in np.nonzero(~stored))
        assert oi.size == 3  # several levels: L + L^T is not full
        rows, cols = np.concatenate([li[:5], oi]), np.concatenate([lj[:5], oj])
        with pytest.raises(_lib.BsmError, match=rf"3 of 8 pairs.*first is pair 5, \({oi[0]}, {oj[0]}\)") as e:
            f.inv_entries(rows, cols)
        assert e.value.code == _lib.BSM_ERR_INVALID
        # the C call leaves its outputs alone
        lib = _lib.require_device()
        diag, vals = np.full(n, 7.0), np.full(8, 7.0)
        r64, c64 = rows.astype(np.uint64), cols.astype(np.uint64)
        rc = lib.bsm_nd_factor_selinv(f._h(), _lib.ptr(diag), 8, _lib.ptr(r64), _lib.ptr(c64), _lib.ptr(vals))
        assert rc == _lib.BSM_ERR_INVALID and np.all(diag == 7.0) and np.all(vals == 7.0)
        c64[0] = n
        rc = lib.bsm_nd_factor_selinv(f._h(), _lib.ptr(diag), 8, _lib.ptr(r64), _lib.ptr(c64), _lib.ptr(vals))
        assert rc == _lib.BSM_ERR_OUT_OF_BOUNDS and np.all(diag == 7.0) and np.all(vals == 7.0)
        with pytest.raises(MatErr) as oob:
            f.inv_entries([0, n], [0, 0])
        assert oob.value.kind == MatErrKind.OutOfBounds
        with pytest.raises(ValueError):
            f.inv_entries([0, 1], [0])
        with pytest.raises(ValueError):
            f.inv_entries([[0]], [[0]])
        with pytest.raises(MatErr) as dims:
            f.inv_on(matrix("g5-leaf1", dtype))
        assert dims.value.kind == MatErrKind.IncorrectDimensions
        # both triangles, and none asked for
        assert same_bits(f.inv_entries(li, lj), f.inv_entries(lj, li))
        assert f.inv_entries([], []).shape == (0,)


def test_inv_on_takes_the_pattern_of_its_argument(monkeypatch):
    """The pattern is a's own (here the diagonal alone, stored zeros included), not the factored matrix's."""
    name, dtype = "blocks", np.float64
    setup(monkeypatch, name)
    n = system(name)[0]
    with cholesky_nd(matrix(name, dtype)) as f:
        d = f.inv_diag()
        eye = Csr.from_csr_arrays((n, n), np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint64),
                                  np.zeros(n))
        on = f.inv_on(eye)
        assert on.get_nnz() == n and same_bits(np.asarray(on.v), d)
        assert np.allclose(d[-9:], 1.0 / 3.0, rtol=1e-14)  # the 3 I block


# ---- bits -----------------------------------------------------------------------


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_same_bits_on_every_call_and_route(monkeypatch, name, dtype):
    import torch

    from basic_sparse_matrix_amd import device

    setup(monkeypatch, name)
    n = system(name)[0]
    with cholesky_nd(matrix(name, dtype)) as f:
        base = everything(f, name)
        assert_same(everything(f, name), base)
        idx = np.arange(n)
        assert same_bits(f.inv_entries(idx, idx), base[0])
        t = device.nd_factor_inv_diag(f)
        assert t.shape == (n,) and t.is_cuda
        assert same_bits(t.cpu().numpy(), base[0])
        out = torch.zeros(n, dtype=t.dtype, device="cuda")
        assert device.nd_factor_inv_diag(f, out, stream=torch.cuda.current_stream()) is out
        assert same_bits(out.cpu().numpy(), base[0])
        f.refactor(matrix(name, dtype, 1))
        assert not same_bits(f.inv_diag(), base[0])
        f.refactor(matrix(name, dtype))
        assert_same(everything(f, name), base)
    monkeypatch.setenv("BSM_ND_PLAIN", "1")
    with cholesky_nd(matrix(name, dtype)) as plain:
        assert_same(everything(plain, name), base)


def test_device_diag_checks(monkeypatch):
    import torch

    from basic_sparse_matrix_amd import device

    name, dtype = "g5-leaf1", np.float64
    setup(monkeypatch, name)
    n = system(name)[0]
    with cholesky_nd(matrix(name, dtype)) as f:
        with pytest.raises(TypeError):
            device.nd_factor_inv_diag(f, torch.zeros(n, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            device.nd_factor_inv_diag(f, torch.zeros(n - 1, dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            device.nd_factor_inv_diag(f, torch.zeros(n, dtype=torch.float64))
        with pytest.raises(ValueError):
            device.nd_factor_inv_diag(f, torch.zeros((n, 2), dtype=torch.float64, device="cuda")[:, 0])


@pytest.mark.parametrize("name,dtype", FEW, ids=FEW_IDS)
def test_nothing_undefined_is_read(monkeypatch, name, dtype):
    """BSM_ND_POISON=1: the fronts (before the factor), Z and the panels start as NaN."""
    setup(monkeypatch, name)
    with cholesky_nd(matrix(name, dtype)) as f:
        base = everything(f, name)
    monkeypatch.setenv("BSM_ND_POISON", "1")
    with cholesky_nd(matrix(name, dtype)) as f:
        got = everything(f, name)
    for g in got:
        assert np.all(np.isfinite(g))
    assert_same(got, base)


# ---- the factor is only read ----------------------------------------------------


@pytest.mark.parametrize("name,dtype", FEW, ids=FEW_IDS)
def test_the_factor_is_untouched(monkeypatch, name, dtype):
    setup(monkeypatch, name)
    n = system(name)[0]
    rng = np.random.default_rng(3)
    b = [rng.standard_normal(n).astype(dtype) for _ in range(3)]

    def snapshot(f):
        out = []
        for k in (1, 3):
            out += cols_of(f.solve(Dense.from_columns(b[:k])))
        l = f.l()
        out += [np.asarray(l.row_index).copy(), np.asarray(l.col_index).copy(), np.asarray(l.v).copy()]
        return out + [np.array([f.logdet()]), np.array([f.nbytes])]

    with cholesky_nd(matrix(name, dtype)) as f:
        before = snapshot(f)
        everything(f, name)
        assert_same(snapshot(f), before)


def test_a_handle_without_values_refuses(monkeypatch):
    import torch

    from basic_sparse_matrix_amd import device

    name, dtype = "g40-leaf64", np.float64
    setup(monkeypatch, name)
    n = system(name)[0]
    A = matrix(name, dtype)
    with cholesky_nd(A) as f:
        base = f.inv_diag()
        with pytest.raises(_lib.BsmError, match="positive definite"):
            f.refactor(matrix(name, dtype, 2))
        out = torch.zeros(n, dtype=torch.float64, device="cuda")
        for call in (f.inv_diag, lambda: f.inv_entries([0], [0]), lambda: f.inv_on(A),
                     lambda: device.nd_factor_inv_diag(f, out)):
            with pytest.raises(_lib.BsmError, match="holds no values; refactor first") as e:
                call()
            assert e.value.code == _lib.BSM_ERR_INVALID
        f.refactor(A)
        assert same_bits(f.inv_diag(), base)


def test_empty_factor():
    e = Csr.from_csr_arrays((0, 0), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0))
    with cholesky_nd(e) as f:
        assert f.inv_diag().shape == (0,)
        assert f.inv_entries([], []).shape == (0,)
        assert f.inv_on(e).get_nnz() == 0
        with pytest.raises(MatErr):
            f.inv_entries([0], [0])


# ---- threads --------------------------------------------------------------------


def test_a_second_thread_solves_while_the_selected_inverse_runs(monkeypatch):
    """One solve on another thread: the handle's mutex puts it before or after the selected inverse."""
    name, dtype = "g40-leaf64", np.float64
    setup(monkeypatch, name)
    n = system(name)[0]
    B = Dense.from_columns([np.random.default_rng(5).standard_normal(n)])
    with cholesky_nd(matrix(name, dtype)) as f:
        ref, base = cols_of(f.solve(B)), f.inv_diag()
        out, errs = [], []

        def solver():
            try:
                out.append(cols_of(f.solve(B)))
            except Exception as e:  # noqa: BLE001 -- reported below
                errs.append(repr(e))

        t = threading.Thread(target=solver)
        t.start()
        d = f.inv_diag()
        t.join()
        assert not errs, errs
        assert_same(out[0], ref)
        assert same_bits(d, base)
