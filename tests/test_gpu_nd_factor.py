"""GPU tests of the kept nd factor (cholesky_nd / NdFactor, bsm_nd_factor_*):
factor P A P^T once, solve many times on the kept factor, export L and L^T
as ordinary Csr. The factor's bits are those of solve(order="nd") and its
solves run the same forward and backward passes, so a factor solve equals the
fused solve bit for bit (for one column: the fused solve with BSM_ND_FOLD=0,
which runs the separate forward pass too). In nd_solve_passes every (front,
column) pair is one workgroup or one wave-task of its own, reading only its
column of the right-hand sides and of the solve vectors, so column j of a
multi-column solve does not depend on k; test_solve_bits_equal_fused_solve
checks that as well (k = 2 against k = 3).

Shapes: the smallest that still exercise each structure (one-pivot fronts
with 63 padding pivots, several levels, one dense front of two pivot tiles,
a multi-level tree, leaves of several pivot tiles, fronts without pivots, an
irregular tree)."""

import functools
import gc

import numpy as np
import pytest

import nd_support
from basic_sparse_matrix_amd import (Csr, Dense, Panic, backward_substitution, cholesky_nd, forward_substitution,
                                     solve)
from nd_support import csr_arrays, dense_of, matrix, rel_err, rhs_cols, same_bits, system

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 2e-3}

POISSON = ["g5-leaf1", "g11-leaf8", "g11-onefront", "g40-leaf64", "g40-leaf256"]
SYSTEMS = POISSON + ["blocks", "random"]
CASES = [(s, np.float64) for s in SYSTEMS] + [(s, np.float32) for s in POISSON]
CASE_IDS = [f"{s}-{np.dtype(d).name}" for s, d in CASES]


def dense_of_csr(m):
    return dense_of(m.row_index, m.col_index, m.v, m.dims.rows)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle's f64 solution of the three right-hand columns, once per system: the band restatement, and the
    literal one for the random matrix."""
    from oracle import pyoracle as orc

    n, rp, ci, v, _ = system(name)
    return orc.solve(n, rp, ci, v, rhs_cols(name), band=name != "random")


def setup(monkeypatch, name, dtype):
    nd_support.setup(monkeypatch, name)
    b = [c.astype(dtype) for c in rhs_cols(name)]
    return system(name)[0], matrix(name, dtype), b, _reference(name)


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_solve_bits_equal_fused_solve(monkeypatch, name, dtype):
    """cholesky_nd(A).solve(B) == solve(A, B, order="nd"), column by column,
    np.array_equal, for k = 2 and 3; for k = 1 against the fused solve with
    BSM_ND_FOLD=0. Column j does not depend on k."""
    n, A, b, _ = setup(monkeypatch, name, dtype)
    with cholesky_nd(A) as f:
        assert f.n == n and f.dtype == np.dtype(dtype) and f.nbytes > 0
        xs = {}
        for k in (2, 3):
            xf = f.solve(Dense.from_columns(b[:k]))
            xs[k] = xf
            fused = solve(A, Dense.from_columns(b[:k]), order="nd")
            for j in range(k):
                assert np.array_equal(np.asarray(xf.get_col(j)), np.asarray(fused.get_col(j))), (k, j)
                assert same_bits(xf.get_col(j), fused.get_col(j)), (k, j)
        for j in range(2):
            assert same_bits(xs[2].get_col(j), xs[3].get_col(j)), j
        monkeypatch.setenv("BSM_ND_FOLD", "0")
        x1 = f.solve(Dense.from_columns(b[:1]))
        fused1 = solve(A, Dense.from_columns(b[:1]), order="nd")
        assert np.array_equal(np.asarray(x1.get_col(0)), np.asarray(fused1.get_col(0)))
        assert same_bits(x1.get_col(0), xs[3].get_col(0))


def test_reuse_survives_other_solves_free_and_cache_clear(monkeypatch):
    """One factor, three different B in turn, a solve of another matrix with
    the same pattern in between (it overwrites the plan's kept fronts); then
    A's handle is freed and the plan cache cleared: the factor still gives
    the fused solve's bits."""
    from basic_sparse_matrix_amd import _lib
    from oracle import pyoracle as orc

    n, A, _, _ = setup(monkeypatch, "g40-leaf64", np.float64)
    _, rp, ci, v, _ = system("g40-leaf64")
    f = cholesky_nd(A)
    last = None
    for seed in (2101, 2102, 2103):
        B = orc.gen_x_cols(seed, n, 2)
        want = solve(A, Dense.from_columns(B), order="nd")
        other = Csr.from_csr_arrays((n, n), rp, ci, 1.5 * v)  # the same pattern, other values
        solve(other, Dense.from_columns(orc.gen_x_cols(seed + 50, n, 2)), order="nd")
        got = f.solve(Dense.from_columns(B))
        for j in range(2):
            assert np.array_equal(np.asarray(got.get_col(j)), np.asarray(want.get_col(j))), (seed, j)
        last = (B, [np.asarray(want.get_col(j)).copy() for j in range(2)])
    del A, other, want
    gc.collect()  # bsm_csr_free of A's handle
    _lib.nd_cache_clear()
    assert _lib.nd_cache_info()["entries"] == 0
    got = f.solve(Dense.from_columns(last[0]))
    for j in range(2):
        assert np.array_equal(np.asarray(got.get_col(j)), last[1][j]), j
    f.close()
    f.close()  # idempotent
    with pytest.raises(ValueError):
        f.solve(Dense.from_columns(last[0]))


def test_concurrent_solves_on_one_factor(monkeypatch):
    """Three threads solve on one handle (ctypes releases the GIL, so the
    calls overlap; the handle's mutex runs them one after the other): every
    call gives the single-thread bits."""
    import threading

    _, A, b, _ = setup(monkeypatch, "g40-leaf64", np.float64)
    with cholesky_nd(A) as f:
        ref = [np.asarray(f.solve(Dense.from_columns(b[:2])).get_col(j)).copy() for j in range(2)]
        out, errs = [], []

        def work():
            try:
                for _ in range(3):
                    x = f.solve(Dense.from_columns(b[:2]))
                    out.append([np.asarray(x.get_col(j)).copy() for j in range(2)])
            except Exception as e:  # noqa: BLE001 -- reported below
                errs.append(repr(e))

        ts = [threading.Thread(target=work) for _ in range(3)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    assert not errs, errs
    assert len(out) == 9
    for x in out:
        for j in range(2):
            assert same_bits(x[j], ref[j]), j


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_solve_accuracy_vs_oracle(monkeypatch, name, dtype):
    """Each column against the oracle's f64 solution (the band restatement;
    the literal one for the random matrix), at the project's own bars."""
    _, A, b, ex = setup(monkeypatch, name, dtype)
    with cholesky_nd(A) as f:
        x = f.solve(Dense.from_columns(b))
    for j in range(3):
        e = rel_err(x.get_col(j), ex[j])
        print(f"{name} {np.dtype(dtype).name} column {j}: rel err {e:.3e}")
        assert e < TOL[dtype], j


def check_reconstruction(A, f, L, dtype):
    """|| L L^T - P A P^T ||_F / || P A P^T ||_F < TOL (the classical
    backward-error bound, (n + 1) u, is far below it at these n)."""
    p = f.perm
    Ap = dense_of_csr(A)[np.ix_(p, p)]
    e = np.linalg.norm(L @ L.T - Ap) / np.linalg.norm(Ap)
    print(f"reconstruction: {e:.3e}")
    assert e < TOL[dtype]
    return Ap


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_export_is_the_factor(orc, monkeypatch, name, dtype):
    n, A, _, _ = setup(monkeypatch, name, dtype)
    with cholesky_nd(A) as f:
        assert f.nnz_l == 0
        l = f.l()
        assert f.nnz_l == l.get_nnz() > 0
        L = dense_of_csr(l)
        Ap = check_reconstruction(A, f, L, dtype)
    if dtype == np.float64 and n <= 400 and name != "blocks":
        # densified, not by pattern: an exact zero on one side can be a
        # rounding-level value on the other
        lr, lc, lv = orc.cholesky(n, n, *csr_arrays(Ap), band=False)
        Lo = dense_of(lr, lc, lv, n)
        e = np.linalg.norm(L - Lo) / np.linalg.norm(Lo)
        print(f"{name}: L against the literal oracle's: {e:.3e}")
        assert e < TOL[dtype]


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_export_conventions(monkeypatch, name, dtype):
    n, A, _, _ = setup(monkeypatch, name, dtype)
    with cholesky_nd(A) as f:
        l, ls, p = f.l(), f.l_star(), f.perm
    assert np.array_equal(np.sort(p), np.arange(n))
    for m in (l, ls):
        assert m.is_finalised and m.dims.rows == n and m.dims.cols == n and m.dtype == np.dtype(dtype)
    rp, ci, v = (np.asarray(x) for x in (l.row_index, l.col_index, l.v))
    sp, si, sv = (np.asarray(x) for x in (ls.row_index, ls.col_index, ls.v))
    assert not np.any(v == 0) and not np.any(sv == 0)
    for i in range(n):
        c = ci[int(rp[i]):int(rp[i + 1])].astype(np.int64)
        assert c.size and c[-1] == i and np.all(np.diff(c) > 0), i  # ascending, the diagonal last
        assert v[int(rp[i + 1]) - 1] > 0, i
        c = si[int(sp[i]):int(sp[i + 1])].astype(np.int64)
        assert c.size and c[0] == i and np.all(np.diff(c) > 0), i  # the diagonal first, ascending
        assert sv[int(sp[i])] > 0, i
    assert ls == l.transpose()


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_export_feeds_the_reference_triangular_solves(monkeypatch, name, dtype):
    """backward_substitution(l_star, forward_substitution(l, P b)), the
    reference-order device kernels, un-permuted, against factor.solve(b)."""
    n, A, b, _ = setup(monkeypatch, name, dtype)
    with cholesky_nd(A) as f:
        l, ls, p = f.l(), f.l_star(), f.perm
        want = f.solve(Dense.from_columns(b[:2]))
    pb = Dense.from_columns([np.ascontiguousarray(c[p]) for c in b[:2]])
    xp = backward_substitution(ls, forward_substitution(l, pb))
    for j in range(2):
        x = np.zeros(n, dtype=dtype)
        x[p] = np.asarray(xp.get_col(j))
        e = rel_err(x, want.get_col(j))
        print(f"{name} {np.dtype(dtype).name} column {j}: {e:.3e}")
        assert e < TOL[dtype], j


@pytest.mark.parametrize("name", ["g5-leaf1", "blocks"])
def test_export_never_reads_padding(monkeypatch, name):
    """BSM_ND_POISON=1: the fronts start as NaN, and the default pipeline
    writes neither the padding rows and columns nor a pivot tile above its
    diagonal; the export holds no NaN and still reconstructs P A P^T."""
    monkeypatch.setenv("BSM_ND_POISON", "1")
    n, A, b, ex = setup(monkeypatch, name, np.float64)
    with cholesky_nd(A) as f:
        l, ls = f.l(), f.l_star()
        assert np.all(np.isfinite(np.asarray(l.v))) and np.all(np.isfinite(np.asarray(ls.v)))
        check_reconstruction(A, f, dense_of_csr(l), np.float64)
        assert ls == l.transpose()
        x = f.solve(Dense.from_columns(b[:1]))
    assert rel_err(x.get_col(0), ex[0]) < TOL[np.float64]


def test_errors_and_empty_shapes():
    with pytest.raises(Panic):
        cholesky_nd(Csr.from_data([[1.0, 2.0]], dtype=np.float32))
    with pytest.raises(Exception, match="positive definite"):
        cholesky_nd(Csr.from_data([[1.0, 2.0], [2.0, 1.0]], dtype=np.float64))
    a = Csr.from_data([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 2.0]], dtype=np.float64)
    with cholesky_nd(a) as f:
        with pytest.raises(Panic):
            f.solve(Dense.from_columns([np.ones(2)]))
        with pytest.raises(Panic):
            f.solve(Dense.from_columns([np.ones(4)]))
        with pytest.raises(TypeError):
            f.solve(Dense.from_columns([np.ones(3, dtype=np.float32)]))
        x0 = f.solve(Dense(0, 3, []))  # k = 0
        assert x0.get_dims().cols == 0 and x0.data == []
        x = np.asarray(f.solve(Dense.from_columns([np.array([1.0, 2.0, 3.0])])).get_col(0))
        assert np.allclose(dense_of_csr(a) @ x, [1.0, 2.0, 3.0], rtol=1e-12, atol=1e-12)
    e = Csr.from_csr_arrays((0, 0), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0))
    with cholesky_nd(e) as f:  # n = 0: a valid empty factor
        assert f.n == 0 and f.nbytes == 0 and f.perm.size == 0
        x = f.solve(Dense.from_columns([np.zeros(0)]))
        assert x.get_dims().cols == 1 and x.get_col(0).size == 0
        for m in (f.l(), f.l_star()):
            assert m.get_nnz() == 0 and m.dims.rows == 0 and m.dims.cols == 0
