"""GPU tests of what a kept nd factor (cholesky_nd / NdFactor) can do beyond
solve and export: refactor in place (new values on the same pattern), the
log-determinant, the L and L^T solves on their own, and right-hand sides that
are already on the device (device.nd_factor_solve).

The systems are those of test_gpu_nd_factor.py, the smallest that still hit
each structure (one-pivot fronts with 63 padding pivots, several levels, one
front of two pivot tiles, a multi-level tree, leaves of several pivot tiles,
fronts without pivots, an irregular tree); f64 on all of them, f32 on the
Poisson ones; the tolerances are that file's.

Second values for a pattern: A2 = D A D with d = 1 + rng.random(n), which is
SPD with A. The variant that is not positive definite has one diagonal entry
negated."""

import functools
import gc
import threading

import numpy as np
import pytest

import nd_support
from basic_sparse_matrix_amd import (Csr, Dense, _lib, backward_substitution, cholesky_nd, forward_substitution)
from nd_support import (assert_same, cols_of, coords, csr_arrays, csr_parts, dense_of, rel_err, rhs_cols, same_bits,
                        system)

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 2e-3}

POISSON = ["g5-leaf1", "g11-leaf8", "g11-onefront", "g40-leaf64", "g40-leaf256"]
SYSTEMS = POISSON + ["blocks", "random"]
CASES = [(s, np.float64) for s in SYSTEMS] + [(s, np.float32) for s in POISSON]
CASE_IDS = [f"{s}-{np.dtype(d).name}" for s, d in CASES]
# a subset for the checks that repeat one property under other switches
FEW = [("g5-leaf1", np.float32), ("g11-onefront", np.float64), ("g40-leaf256", np.float64), ("blocks", np.float64)]
FEW_IDS = [f"{s}-{np.dtype(d).name}" for s, d in FEW]


@functools.lru_cache(maxsize=None)
def _values(name):
    """The three value sets of a pattern, f64: A's, A2 = D A D's, and A's with one diagonal entry negated."""
    n, _, _, v, _ = system(name)
    rows, cols = coords(name)
    d = 1.0 + np.random.default_rng(11).random(n)
    v2 = d[rows] * v * d[cols]
    bad = v.copy()
    e = int(np.nonzero((rows == n // 2) & (cols == n // 2))[0][0])
    bad[e] = -bad[e]
    return v, v2, bad


def setup(monkeypatch, name, dtype):
    nd_support.setup(monkeypatch, name)
    return system(name)[0], [c.astype(dtype) for c in rhs_cols(name)]


def matrix(name, dtype, which=0):
    """A fresh Csr (a fresh device handle) of the pattern with value set `which`."""
    return nd_support.matrix(name, dtype, _values(name)[which])


def snapshot(f, b):
    """Everything a factor answers: the solves for k = 1, 2, 3, L, L^T, perm."""
    out = []
    for k in (1, 2, 3):
        out += cols_of(f.solve(Dense.from_columns(b[:k])))
    out += csr_parts(f.l()) + csr_parts(f.l_star()) + [f.perm]
    return out


def invalid(match):
    return pytest.raises(_lib.BsmError, match=match)


# ---- refactor -------------------------------------------------------------------


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_refactor_has_the_bits_of_a_fresh_factor(monkeypatch, name, dtype):
    _, b = setup(monkeypatch, name, dtype)
    A, A2 = matrix(name, dtype), matrix(name, dtype, 1)
    with cholesky_nd(A) as f, cholesky_nd(matrix(name, dtype, 1)) as fresh:
        base = snapshot(f, b)
        nbytes = f.nbytes
        assert f.nnz_l > 0
        f.refactor(A2)  # a handle without a plan: the factor's own pattern copy is compared
        assert f.nnz_l == 0
        assert_same(snapshot(f, b), snapshot(fresh, b))
        assert f.nbytes == nbytes
        f.refactor(A)  # the handle the factor's plan came from
        assert_same(snapshot(f, b), base)
        assert f.nbytes == nbytes


def test_refactor_plain_pipeline(monkeypatch):
    monkeypatch.setenv("BSM_ND_PLAIN", "1")
    name, dtype = "g40-leaf64", np.float64
    _, b = setup(monkeypatch, name, dtype)
    with cholesky_nd(matrix(name, dtype)) as f, cholesky_nd(matrix(name, dtype, 1)) as fresh:
        base = snapshot(f, b)
        f.refactor(matrix(name, dtype, 1))
        assert_same(snapshot(f, b), snapshot(fresh, b))
        f.refactor(matrix(name, dtype))
        assert_same(snapshot(f, b), base)


def test_refactor_does_not_depend_on_what_the_fronts_held(monkeypatch):
    """BSM_ND_POISON=1 fills the fronts with NaN before the numeric factor, of a refactorisation too."""
    name, dtype = "g5-leaf1", np.float64
    _, b = setup(monkeypatch, name, dtype)
    with cholesky_nd(matrix(name, dtype)) as f, cholesky_nd(matrix(name, dtype, 1)) as fresh:
        monkeypatch.setenv("BSM_ND_POISON", "1")
        f.refactor(matrix(name, dtype, 1))
        assert_same(snapshot(f, b), snapshot(fresh, b))


def test_refactor_after_cache_clear_and_free_of_a(monkeypatch):
    """The plan cache cleared and A's handle freed: what the new matrix is
    compared against is the factor's own copy of the pattern."""
    name, dtype = "g40-leaf64", np.float64
    _, b = setup(monkeypatch, name, dtype)
    with cholesky_nd(matrix(name, dtype, 1)) as fresh:
        want = snapshot(fresh, b)
    A = matrix(name, dtype)
    f = cholesky_nd(A)
    del A
    gc.collect()
    _lib.nd_cache_clear()
    assert _lib.nd_cache_info()["entries"] == 0
    f.refactor(matrix(name, dtype, 1))
    assert_same(snapshot(f, b), want)
    n, rp, ci, _, _ = system(name)
    moved = ci.copy()
    moved[1] += 1  # row 0 of the grid: columns 0, 1, g -> 0, 2, g
    with invalid("col differs"):
        f.refactor(Csr.from_csr_arrays((n, n), rp, moved, _values(name)[0]))
    assert_same(snapshot(f, b), want)
    f.close()


@pytest.mark.parametrize("switch", ["BSM_ND_SHARED", "BSM_ND_CACHE"])
def test_refactor_with_the_caches_off(monkeypatch, switch):
    """No cross-handle cache entry (and, with BSM_ND_CACHE=0, no plan on the
    handle either): create makes the pattern copy itself, and refactor
    compares against it."""
    monkeypatch.setenv(switch, "0")
    name, dtype = "g11-leaf8", np.float64
    n, b = setup(monkeypatch, name, dtype)
    _, rp, ci, _, _ = system(name)
    A = matrix(name, dtype)
    with cholesky_nd(A) as f, cholesky_nd(A) as second, cholesky_nd(matrix(name, dtype, 1)) as fresh:
        base, want = snapshot(f, b), snapshot(fresh, b)
        f.refactor(matrix(name, dtype, 1))
        assert_same(snapshot(f, b), want)
        assert_same(snapshot(second, b), base)  # another factor of the same matrix is not touched
        moved = ci.copy()
        moved[1] += 1
        with invalid("col differs"):
            f.refactor(Csr.from_csr_arrays((n, n), rp, moved, _values(name)[0]))
        f.refactor(A)
        assert_same(snapshot(f, b), base)


def test_refactor_keeps_the_plan_of_create(monkeypatch):
    """BSM_ND_LEAF changed between create and refactor: the factor's plan still rules."""
    name, dtype = "g40-leaf64", np.float64
    _, b = setup(monkeypatch, name, dtype)
    with cholesky_nd(matrix(name, dtype)) as f, cholesky_nd(matrix(name, dtype, 1)) as fresh:
        want = snapshot(fresh, b)  # made under the original leaf
        monkeypatch.setenv("BSM_ND_LEAF", "256")
        monkeypatch.setenv("BSM_ND_PLAIN", "1")
        f.refactor(matrix(name, dtype, 1))
        got = snapshot(f, b)
    assert_same(got, want)
    with cholesky_nd(matrix(name, dtype, 1)) as other:  # the other leaf gives another order: the check can fail
        assert not np.array_equal(other.perm, want[-1])


def test_refactor_rejections_leave_the_factor_untouched(monkeypatch):
    from oracle import pyoracle as orc

    name, dtype = "g11-leaf8", np.float64
    n, b = setup(monkeypatch, name, dtype)
    _, rp, ci, v, _ = system(name)
    with cholesky_nd(matrix(name, dtype)) as f:
        base = snapshot(f, b)
        with invalid("dtype differs"):
            f.refactor(matrix(name, np.float32))
        rp10, ci10, v10 = orc.poisson2d(10)
        with invalid("n differs"):
            f.refactor(Csr.from_csr_arrays((100, 100), rp10, ci10, np.asarray(v10, dtype=dtype)))
        moved = ci.copy()
        moved[1] += 1  # row 0: columns 0, 1, 11 -> 0, 2, 11; the same n and nnz
        with invalid("col differs"):
            f.refactor(Csr.from_csr_arrays((n, n), rp, moved, v))
        a = dense_of(rp, ci, v, n)
        a[0, 2] = a[2, 0] = -0.25  # two more entries
        with invalid("nnz differs"):
            f.refactor(Csr.from_csr_arrays((n, n), *csr_arrays(a)))
        a = dense_of(rp, ci, v, n)
        assert a[5, 7] == 0.0 and a[6, 7] != 0.0
        a[5, 7], a[6, 7] = -0.25, 0.0  # the same nnz, an entry moved from row 6 to row 5: row_ptr differs
        shifted = csr_arrays(a)
        assert shifted[1].size == ci.size and not np.array_equal(shifted[0], rp)
        with invalid("row_ptr differs"):
            f.refactor(Csr.from_csr_arrays((n, n), *shifted))
        assert_same(snapshot(f, b), base)
        with pytest.raises(TypeError):
            f.refactor(Csr.from_data([[1, 0], [0, 1]], dtype=np.int32))


@pytest.mark.parametrize("name,dtype", [("g40-leaf64", np.float64), ("g5-leaf1", np.float32)],
                         ids=["g40-leaf64-float64", "g5-leaf1-float32"])
def test_refactor_not_positive_definite_empties_the_factor(monkeypatch, name, dtype):
    import torch

    from basic_sparse_matrix_amd import device

    n, b = setup(monkeypatch, name, dtype)
    _, rp, ci, _, _ = system(name)
    bad = _values(name)[2]
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(dense_of(rp, ci, bad, n))
    with pytest.raises(_lib.BsmError, match="positive definite") as fresh_err:
        cholesky_nd(matrix(name, dtype, 2))
    A = matrix(name, dtype)
    with cholesky_nd(A) as f:
        base = snapshot(f, b)
        perm, nbytes = f.perm, f.nbytes
        with pytest.raises(_lib.BsmError, match="positive definite") as err:
            f.refactor(matrix(name, dtype, 2))
        assert err.value.code == fresh_err.value.code == _lib.BSM_ERR_UNSUPPORTED
        assert err.value.msg == fresh_err.value.msg
        B = Dense.from_columns(b[:1])
        tb = torch.tensor(np.ascontiguousarray(b[0]), device="cuda")
        for call in (lambda: f.solve(B), lambda: f.solve(B, system="L"), lambda: f.solve(B, system="Lt"), f.l,
                     f.l_star, f.logdet, lambda: device.nd_factor_solve(f, tb)):
            with invalid("holds no values; refactor first") as e:
                call()
            assert e.value.code == _lib.BSM_ERR_INVALID
        assert np.array_equal(f.perm, perm) and f.nbytes == nbytes and f.n == n
        f.refactor(A)
        assert_same(snapshot(f, b), base)


# ---- logdet ---------------------------------------------------------------------


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_logdet(monkeypatch, name, dtype):
    n, _ = setup(monkeypatch, name, dtype)
    _, rp, ci, _, _ = system(name)
    v, v2, _ = (x.astype(dtype) for x in _values(name))
    sign, ref = np.linalg.slogdet(dense_of(rp, ci, v, n))
    assert sign == 1.0
    with cholesky_nd(matrix(name, dtype)) as f, cholesky_nd(matrix(name, dtype, 1)) as fresh:
        ld = f.logdet()
        assert isinstance(ld, float)
        e = abs(ld - ref) / abs(ref)
        print(f"{name} {np.dtype(dtype).name}: logdet {ld!r}, slogdet {ref!r}, rel err {e:.3e}")
        assert e < TOL[dtype]
        l = f.l()
        lrp, lv = np.asarray(l.row_index).astype(np.int64), np.asarray(l.v)
        host = 2.0 * np.sum(np.log(lv[lrp[1:] - 1].astype(np.float64)))  # the diagonal is last in each row
        e = abs(ld - host) / abs(host)
        print(f"{name} {np.dtype(dtype).name}: against the exported diagonal {e:.3e}")
        assert e < 1e-12
        assert same_bits(np.array([f.logdet()]), np.array([ld]))
        f.refactor(matrix(name, dtype, 1))
        assert same_bits(np.array([f.logdet()]), np.array([fresh.logdet()]))
        sign2, ref2 = np.linalg.slogdet(dense_of(rp, ci, v2, n))
        assert sign2 == 1.0 and abs(f.logdet() - ref2) / abs(ref2) < TOL[dtype]


def test_empty_factor():
    e = Csr.from_csr_arrays((0, 0), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0))
    with cholesky_nd(e) as f:
        assert f.logdet() == 0.0
        f.refactor(e)
        for system in ("A", "L", "Lt"):
            x = f.solve(Dense.from_columns([np.zeros(0)]), system=system)
            assert x.get_dims().cols == 1 and x.get_col(0).size == 0


# ---- the L and L^T systems ------------------------------------------------------


def two_pass(f, b, k, p):
    """(y, xp, x): L y = P b, L^T xp = y, x = P^T xp."""
    pb = Dense.from_columns([np.ascontiguousarray(c[p]) for c in b[:k]])
    y = f.solve(pb, system="L")
    xp = f.solve(y, system="Lt")
    x = []
    for c in cols_of(xp):
        o = np.zeros_like(c)
        o[p] = c
        x.append(o)
    return pb, y, xp, x


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_systems(monkeypatch, name, dtype):
    _, b = setup(monkeypatch, name, dtype)
    with cholesky_nd(matrix(name, dtype)) as f:
        p = f.perm
        ys, xps = {}, {}
        for k in (1, 2, 3):
            want = cols_of(f.solve(Dense.from_columns(b[:k])))
            pb, y, xp, x = two_pass(f, b, k, p)
            ys[k], xps[k] = cols_of(y), cols_of(xp)
            if k == 2:
                continue
            for j in range(k):  # A = scatter . LT . L . gather, bit for bit
                assert same_bits(x[j], want[j]), (k, j)
            yref = forward_substitution(f.l(), pb)
            xref = backward_substitution(f.l_star(), y)
            for j in range(k):
                ey, ex = rel_err(y.get_col(j), yref.get_col(j)), rel_err(xp.get_col(j), xref.get_col(j))
                print(f"{name} {np.dtype(dtype).name} k {k} column {j}: L {ey:.3e}, Lt {ex:.3e}")
                assert ey < TOL[dtype] and ex < TOL[dtype], (k, j)
        for j in range(2):  # column j does not depend on k
            assert same_bits(ys[3][j], ys[2][j]) and same_bits(xps[3][j], xps[2][j]), j
        assert same_bits(ys[3][0], ys[1][0]) and same_bits(xps[3][0], xps[1][0])
        with pytest.raises(ValueError):
            f.solve(Dense.from_columns(b[:1]), system="Q")


@pytest.mark.parametrize("name,dtype", FEW, ids=FEW_IDS)
def test_systems_on_both_kernel_families(monkeypatch, name, dtype):
    """BSM_ND_FWD_TILES / BSM_ND_BWD_TILES = 0: one workgroup per (front,
    column); = 1: by tiles on every level (what the default takes at these
    sizes). The same bits either way, for each pass alone as for both."""
    _, b = setup(monkeypatch, name, dtype)
    with cholesky_nd(matrix(name, dtype)) as f:
        p = f.perm
        got = {}
        for mode in ("0", "1"):
            monkeypatch.setenv("BSM_ND_FWD_TILES", mode)
            monkeypatch.setenv("BSM_ND_BWD_TILES", mode)
            for k in (1, 3):
                want = cols_of(f.solve(Dense.from_columns(b[:k])))
                _, y, xp, x = two_pass(f, b, k, p)
                for j in range(k):
                    assert same_bits(x[j], want[j]), (mode, k, j)
                got[mode, k] = cols_of(y) + cols_of(xp)
        for k in (1, 3):
            assert_same(got["0", k], got["1", k])


# ---- right-hand sides on the device ---------------------------------------------


@pytest.mark.parametrize("name,dtype", FEW, ids=FEW_IDS)
def test_device_solve(monkeypatch, name, dtype):
    import torch

    from basic_sparse_matrix_amd import device

    n, b = setup(monkeypatch, name, dtype)
    with cholesky_nd(matrix(name, dtype)) as f:
        for system in ("A", "L", "Lt"):
            for k in (1, 3):
                want = cols_of(f.solve(Dense.from_columns(b[:k]), system=system))
                tb = torch.tensor(np.ascontiguousarray(np.stack(b[:k], axis=1)), device="cuda")  # row-major n x k
                x = device.nd_factor_solve(f, tb, system=system)
                assert x.shape == (n, k) and x.data_ptr() != tb.data_ptr()
                assert same_bits(tb.cpu().numpy(), np.stack(b[:k], axis=1))  # b is left alone
                xh = x.cpu().numpy()
                for j in range(k):
                    assert same_bits(xh[:, j], want[j]), (system, k, j)
                r = device.nd_factor_solve(f, tb, out=tb, system=system)  # in place
                assert r is tb
                for j in range(k):
                    assert same_bits(tb.cpu().numpy()[:, j], want[j]), (system, k, j)
            t1 = torch.tensor(np.ascontiguousarray(b[0]), device="cuda")  # 1-D
            x1 = device.nd_factor_solve(f, t1, system=system, stream=torch.cuda.current_stream())
            assert x1.shape == (n,)
            assert same_bits(x1.cpu().numpy(), cols_of(f.solve(Dense.from_columns(b[:1]), system=system))[0])
        other = torch.float32 if dtype == np.float64 else torch.float64
        with pytest.raises(TypeError):
            device.nd_factor_solve(f, torch.zeros(n, dtype=other, device="cuda"))
        good = torch.tensor(np.ascontiguousarray(b[0]), device="cuda")
        with pytest.raises(ValueError):
            device.nd_factor_solve(f, good[: n - 1].contiguous())
        with pytest.raises(ValueError):
            device.nd_factor_solve(f, good.cpu())
        with pytest.raises(ValueError):
            device.nd_factor_solve(f, good, out=torch.zeros((n, 2), dtype=good.dtype, device="cuda"))
        with pytest.raises(ValueError):
            device.nd_factor_solve(f, good, system="Q")


# ---- threads --------------------------------------------------------------------


def test_refactor_while_another_thread_solves(monkeypatch):
    """One thread solves about 20 times while another refactors once: the
    handle's mutex puts every solve before or after the refactorisation, so
    each result has the bits of factor(A)'s or of factor(A2)'s solve."""
    name, dtype = "g40-leaf64", np.float64
    _, b = setup(monkeypatch, name, dtype)
    B = Dense.from_columns(b[:2])
    A2 = matrix(name, dtype, 1)
    with cholesky_nd(matrix(name, dtype, 1)) as fresh:
        ref2 = cols_of(fresh.solve(B))
    with cholesky_nd(matrix(name, dtype)) as f:
        ref1 = cols_of(f.solve(B))
        assert not same_bits(ref1[0], ref2[0])
        out, errs = [], []
        started = threading.Event()

        def solver():
            try:
                for _ in range(20):
                    out.append(cols_of(f.solve(B)))
                    started.set()
            except Exception as e:  # noqa: BLE001 -- reported below
                errs.append(repr(e))
            finally:
                started.set()

        def refactorer():
            try:
                started.wait()
                f.refactor(A2)
            except Exception as e:  # noqa: BLE001 -- reported below
                errs.append(repr(e))

        ts = [threading.Thread(target=solver), threading.Thread(target=refactorer)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        assert len(out) == 20
        seen_second = False
        for x in out:
            first = all(same_bits(x[j], ref1[j]) for j in range(2))
            second = all(same_bits(x[j], ref2[j]) for j in range(2))
            assert first or second
            assert not (seen_second and first)  # no solve sees the old factor after the new one
            seen_second = seen_second or second
        assert_same(cols_of(f.solve(B)), ref2)
