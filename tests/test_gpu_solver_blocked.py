"""GPU tests of solve(..., order="blocked") (bsm_solve_blocked): the
reference's solve (src/lib.rs:11-24) with the triangular solves reassociated
into 64-row blocks. Not bit-exact by design; the bar is BASELINE.json's
floating-point tolerance: 1e-6 relative on f64 against the reference-order
result (the band oracle, itself pinned to the reference's goldens). The tests
use tighter bounds where the systems are well conditioned, so a wrong block
(an off-by-one in the band masks, a missing far block) cannot hide."""

import functools

import numpy as np
import pytest

import band_support as bs
from basic_sparse_matrix_amd import Csr, Dense, Panic, solve
from basic_sparse_matrix_amd._lib import BsmError
from golden.golden_io import matrix, scalars
from nd_support import assert_same, cols_of, csr_arrays, rel_err

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 2e-3}


def test_blocked_solve_golden(golden):
    """solve_test (lib.rs:74-138): [0.625, -0.1, 2.6999998, 0.5] within f32 rounding."""
    g = golden["solve_test"]
    b = Dense.from_data([scalars(c, np.float32) for c in g["b_cols"]], dtype=np.float32)
    a = Csr.from_data(matrix(g["rows"], np.float32), dtype=np.float32)
    x = solve(a, b, order="blocked").get_col(0)
    assert np.allclose(x, [0.625, -0.1, 2.6999998, 0.5], rtol=1e-6, atol=1e-6)


def test_blocked_solve_non_square_panics():
    with pytest.raises(Panic):
        solve(Csr.from_data([[1.0, 2.0]], dtype=np.float32), Dense.from_data([[1.0]], dtype=np.float32),
              order="blocked")


def test_blocked_solve_bad_order():
    with pytest.raises(ValueError):
        solve(Csr.from_data([[1.0]], dtype=np.float64), Dense.from_data([[1.0]], dtype=np.float64), order="x")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("g,k", [(1, 1), (5, 2), (8, 1), (11, 3), (40, 2), (70, 1), (130, 2)])
def test_blocked_poisson_vs_oracle(orc, dtype, g, k):
    """2D Poisson g x g (bandwidth g): n from 1 to 16,900, one to three RHS
    columns; n not a multiple of 64 and bandwidths below, at and above the
    block size, so partial last blocks, empty far ranges and far blocks that
    straddle the band edge all occur."""
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    v = v.astype(dtype)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    b = orc.gen_x_cols(1004, n, k, dtype=dtype)
    ex = orc.solve(n, rp, ci, v, b, band=True)
    x = solve(A, Dense.from_columns(b), order="blocked")
    if dtype == np.float64:
        for j in range(k):
            assert rel_err(x.get_col(j), ex[j]) < TOL[dtype], j
    else:  # f32: error ~ cond(A) * 6e-8 (cond <= ~1e4 here) against the f64 solution
        x64 = orc.solve(n, rp, ci, v.astype(np.float64), [c.astype(np.float64) for c in b], band=True)
        for j in range(k):
            assert rel_err(x.get_col(j), x64[j]) < 2e-3, j


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_blocked_wide_band_vs_oracle(orc, dtype):
    """Bandwidth 1060 > 1024 (17 far blocks per 64-row block)."""
    n, g = 2400, 1060
    rows, cols, vals = [], [], []
    for i in range(n):
        for j, val in ((i - g, -1.0), (i - 1, -1.0), (i, 4.5), (i + 1, -1.0), (i + g, -1.0)):
            if 0 <= j < n:
                rows.append(i), cols.append(j), vals.append(val)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.uint64)
    ci = np.asarray(cols, dtype=np.uint64)
    v = np.asarray(vals, dtype=dtype)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    b = orc.gen_x_cols(1003, n, 1, dtype=dtype)
    x = solve(A, Dense.from_columns(b), order="blocked").get_col(0)
    ex = orc.solve(n, rp, ci, v, b, band=True)[0]
    assert rel_err(x, ex) < TOL[dtype]


def test_blocked_random_spd_vs_oracle(orc):
    """Random sparse SPD (irregular envelope, dense-ish rows) against the
    literal oracle."""
    rng = np.random.default_rng(7)
    n = 300
    a = np.zeros((n, n))
    mask = rng.random((n, n)) < 0.02
    vals = rng.uniform(-1.0, 1.0, (n, n))
    a[mask] = vals[mask]
    a = np.tril(a, -1)
    a = a + a.T
    a[np.arange(n), np.arange(n)] = np.abs(a).sum(axis=1) + 1.0 + rng.random(n)
    nzr, nzc = np.nonzero(a != 0)
    rp = np.concatenate([[0], np.cumsum(np.bincount(nzr, minlength=n))]).astype(np.uint64)
    ci, v = nzc.astype(np.uint64), a[nzr, nzc]
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    b = orc.gen_x_cols(1005, n, 2)
    ex = orc.solve(n, rp, ci, v, b, band=False)
    x = solve(A, Dense.from_columns(b), order="blocked")
    for j in range(2):
        assert rel_err(x.get_col(j), ex[j]) < 1e-12


# the blocked factor (blk_chol) / the reference-order band factor (band_chol5)
# under the blocked solves (BSM_BLK_CHOL=0)
@pytest.mark.parametrize("blk_chol", ["1", "0"])
def test_blocked_poisson_250_f64_vs_reference_order(orc, monkeypatch, blk_chol):
    """62,500 unknowns, bandwidth 250: blocked vs reference order on the GPU."""
    monkeypatch.setenv("BSM_BLK_CHOL", blk_chol)
    g = 250
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    b = orc.gen_x_cols(1002, n, 1)
    xr = solve(A, Dense.from_columns(b)).get_col(0)
    xb = solve(A, Dense.from_columns(b), order="blocked").get_col(0)
    assert rel_err(xb, xr) < 1e-10


@pytest.mark.slow
def test_c5_blocked_poisson_1m_f64_properties(orc, golden_c5):
    """C5 (N = 1M, bandwidth 1000) through the blocked solves: within 1e-6
    relative (BASELINE.json) of the band oracle's exact x (sampled from
    tests/golden/c5_poisson_1000.json) and of x_true, residual tiny."""
    g = 1000
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    x_true = orc.gen_x_cols(1002, n, 1)[0]
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    b = np.zeros(n)
    np.add.at(b, rows, v * x_true[ci.astype(np.int64)])
    x = solve(A, Dense.from_columns([b]), order="blocked").get_col(0)
    exact = np.asarray([int(h, 16) for h in golden_c5["x_sample_bits"]], dtype=np.uint64).view(np.float64)
    assert rel_err(x[::golden_c5["x_stride"]], exact) < 1e-6
    assert rel_err(x, x_true) < 1e-6
    r = np.zeros(n)
    np.add.at(r, rows, v * x[ci.astype(np.int64)])
    assert np.linalg.norm(r - b) / np.linalg.norm(b) < 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("g,k", [(9, 1), (40, 2), (70, 1), (130, 2), (250, 1)])
def test_blocked_progressive_handoff_deterministic(orc, dtype, g, k):
    """The blocked factor's progressive hand-off (tile K publishes Linv_K by
    16-row blocks, tile K + 1 forms its sub-diagonal tile block by block):
    two runs give the same bits (every element's MFMA sequence is fixed, so
    any stale hand-off would show), within the tolerance of the band oracle."""
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    v = v.astype(dtype)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    b = orc.gen_x_cols(1007, n, k, dtype=dtype)
    xs = []
    for _ in range(2):
        x = solve(A, Dense.from_columns(b), order="blocked")
        xs.append([np.asarray(x.get_col(j)).copy() for j in range(k)])
    ref = orc.solve(n, rp, ci, v.astype(np.float64), [c.astype(np.float64) for c in b], band=True)
    for j in range(k):
        assert np.array_equal(xs[0][j].view(np.uint8), xs[1][j].view(np.uint8)), j
        assert rel_err(xs[0][j], ref[j]) < TOL[dtype], j


# ----------------------------------------------------- non-stationary bands
# band_support.py's systems: every row has its own scale, so the block that a
# ticket reads (Linv_I, MF_I / MB_I, a far tile) differs from its neighbours
# in every digit, where a Poisson factor's blocks agree to many. (n, b) put
# the 64-row tile edge in both: b = 0 (DM = 1, no sub-diagonal tile), 1,
# 63 / 64 / 65, 127 / 128 / 129, n = 63, 64, 65, 128, 129, and the 16-row
# panel edge of blk_diag_panels (b = 15, 16, 17).
#
# Truth: for f32 the oracle's f64 reference-order solve of the f32-rounded
# system; for f64 a band Cholesky solve in np.longdouble (band_support.py).
# e_ref is the reference-order oracle's own error in the tested dtype against
# that truth, relative, in the Frobenius norm over the k columns.
BAND_SYSTEMS = bs.blocked_systems()
F64, F32 = np.float64, np.float32


def rel_fro(x_cols, truth_cols):
    t = np.stack(truth_cols)
    d = np.stack([np.asarray(c, dtype=t.dtype) for c in x_cols]) - t
    return float(np.sqrt((d * d).sum()) / np.sqrt((t * t).sum()))


@functools.lru_cache(maxsize=None)
def band_case(kind, n, b, fill, dtype, kmax=4):
    """(rp, ci, v, rhs columns, truth columns, the reference-order oracle's
    columns) of one system in one dtype; the k = 1 tests take column 0."""
    from oracle import pyoracle as orc

    a = bs.system(kind, n, b, fill).astype(dtype)
    rp, ci, v = csr_arrays(a)
    rhs = orc.gen_x_cols(1013, n, kmax, dtype=dtype)
    if dtype == F32:
        truth = orc.solve(n, rp, ci, v.astype(F64), [c.astype(F64) for c in rhs], band=True)
    else:
        truth = list(bs.solve_longdouble(a, b, np.stack(rhs, axis=1)).T)
    return rp, ci, v, rhs, truth, orc.solve(n, rp, ci, v, rhs, band=True)


def blocked_error(case, n, k):
    """(error of the blocked solve, e_ref), both against the truth, on the first k columns."""
    rp, ci, v, rhs, truth, ref = case
    x = cols_of(solve(Csr.from_csr_arrays((n, n), rp, ci, v), Dense.from_columns(rhs[:k]), order="blocked"))
    assert len(x) == k
    return rel_fro(x, truth[:k]), rel_fro(ref[:k], truth[:k])


BAND_CASES = [pytest.param(*s, dt, k, id=f"{s[0]}-{s[1]}-{s[2]}-{np.dtype(dt).name}-k{k}")
              for s in BAND_SYSTEMS for dt in (F64, F32) for k in (1, 4)]


@pytest.mark.parametrize("kind,n,b,fill,dtype,k", BAND_CASES)
def test_blocked_band_vs_truth(kind, n, b, fill, dtype, k):
    """The default blocked factor (blk_chol) under blk_prep / blk_trsv.

    f64: TOL[f64] = 1e-10, the file's own number: blk_diag_panels takes its
    pivots from the hardware rsqrt estimate plus one Newton step, a floor
    above eps that is not derived here. Worst observed on these 23 systems
    (MI355X): 1.1e-15, 7.3 e_ref, at (200, 127) with k = 1 (e_ref 1.1e-16 ..
    2.2e-16).

    f32: 8 e_ref (e_ref 5e-8 .. 1e-7 on these systems; 1e-8 and 3e-8 for the
    single column of n = 1 and n = 2). Reassociation changes
    the constants of the rounding bound, not its order; the explicit inverse
    diagonal blocks may add up to kappa(L_II) <= sqrt(kappa_2(A)) <= 8
    (test_band_systems.py: kappa_2 <= 64), and the f32 tiles are carried in
    f64 MFMA, which only helps. Worst observed: 1.8e-7, 2.6 e_ref, at
    (128, 64) with k = 1; no case came near the bar."""
    err, e_ref = blocked_error(band_case(kind, n, b, fill, dtype), n, k)
    print(f"blocked default {kind} n={n} b={b} {np.dtype(dtype).name} k={k}: err {err:.3e} e_ref {e_ref:.3e} "
          f"ratio {err / max(e_ref, 1e-300):.2f}")
    if dtype == F64:
        assert err < TOL[F64]
    else:
        assert err <= 8 * e_ref


BAND_CASES_F64 = [pytest.param(*s, k, id=f"{s[0]}-{s[1]}-{s[2]}-k{k}") for s in BAND_SYSTEMS for k in (1, 4)]


@pytest.mark.parametrize("kind,n,b,fill,k", BAND_CASES_F64)
def test_blocked_band_reference_factor_f64_vs_truth(monkeypatch, kind, n, b, fill, k):
    """BSM_BLK_CHOL=0: the reference-order factor (exact pivots) under
    blk_prep / blk_trsv, so only the two solves are reassociated and a wrong
    coupling block cannot hide under the rsqrt floor of the blocked factor:
    8 e_ref against the longdouble truth (e_ref 1.1e-16 .. 2.2e-16). Worst
    observed: 3.1e-16; the largest ratio is 2.1 e_ref, at (129, 65) with k = 1."""
    monkeypatch.setenv("BSM_BLK_CHOL", "0")
    err, e_ref = blocked_error(band_case(kind, n, b, fill, F64), n, k)
    print(f"blocked BSM_BLK_CHOL=0 {kind} n={n} b={b} f64 k={k}: err {err:.3e} e_ref {e_ref:.3e} "
          f"ratio {err / max(e_ref, 1e-300):.2f}")
    assert err <= 8 * e_ref


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("n,b", [(129, 65), (321, 193)])
def test_blocked_band_deterministic(dtype, n, b):
    """Two runs give the same bits (as test_blocked_progressive_handoff_deterministic
    asks of the Poisson systems): with blocks that all differ, a stale
    hand-off would not be a small change."""
    rp, ci, v, rhs, _, _ = band_case("band", n, b, bs.blocked_fill(b), dtype)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    runs = [cols_of(solve(A, Dense.from_columns(rhs), order="blocked")) for _ in range(2)]
    assert_same(runs[0], runs[1])


@pytest.mark.parametrize("blk_chol", ["1", "0"])
def test_blocked_band_more_tickets_than_workgroups(monkeypatch, blk_chol):
    """n = 4096, b = 70, k = 64: 64 blocks x 64 columns = 4096 blk_trsv
    tickets, more than any resident grid (asserted against 16 workgroups per
    CU, twice what 256 threads allow), so every workgroup takes many tickets
    in turn and waits on flags that earlier tickets of other workgroups raise.
    The same bars: 1e-10 with the default factor, 8 e_ref with the
    reference-order one. Observed: 6.4e-16 (4.3 e_ref) with the default
    factor, 2.3e-16 (1.5 e_ref) with the reference-order one."""
    import torch

    n, b = bs.BLOCKED_TICKETS
    k = 64
    assert (n + 63) // 64 * k >= 16 * torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.setenv("BSM_BLK_CHOL", blk_chol)
    err, e_ref = blocked_error(band_case("band", n, b, 1.0, F64, k), n, k)
    print(f"blocked tickets BSM_BLK_CHOL={blk_chol} n={n} b={b} f64 k={k}: err {err:.3e} e_ref {e_ref:.3e} "
          f"ratio {err / max(e_ref, 1e-300):.2f}")
    assert err < TOL[F64]
    if blk_chol == "0":
        assert err <= 8 * e_ref


@pytest.mark.parametrize("dtype", [F64, F32])
def test_blocked_band_refusals(dtype):
    """The blocked path has no general fall-back: a matrix that is not
    positive definite and one with a row's columns out of order raise
    BsmError, and the next solve in the same process is right. A bad pivot
    cannot stall blk_chol: blk_diag_panels only records it (pd, then
    ST_NOT_PD after its last barrier) and no branch, flag or barrier there or
    in blk_chol depends on a value, so the NaNs run through to the end; the
    unsorted row is refused by band_setup before any launch."""
    n, b = 129, 65
    rp, ci, v, rhs, _, _ = band_case("band", n, b, bs.blocked_fill(b), dtype)
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    bad = v.copy()
    bad[(rows == 70) & (ci == 70)] *= -1
    with pytest.raises(BsmError, match="not positive definite"):
        solve(Csr.from_csr_arrays((n, n), rp, ci, bad), Dense.from_columns(rhs), order="blocked")
    s, e = int(rp[70]), int(rp[71])
    assert e - s >= 3
    perm = np.arange(len(v))
    perm[[s, s + 2]] = perm[[s + 2, s]]
    with pytest.raises(BsmError, match="strictly increasing columns"):
        solve(Csr.from_csr_arrays((n, n), rp, ci[perm], v[perm]), Dense.from_columns(rhs), order="blocked")
    err, e_ref = blocked_error(band_case("band", n, b, bs.blocked_fill(b), dtype), n, 4)
    assert err < TOL[F64] if dtype == F64 else err <= 8 * e_ref
