"""GPU parity of Csr::cholesky_decomp (src/sparse.rs:682-714) and the solver
chain solve / forward_substitution / backward_substitution (src/lib.rs:11-65).

Bar: bit-exact against the reference's f32 golden vectors and against the CPU
oracle (literal O(N^3) restatement for small N, band restatement -- itself
checked equal to the literal one in test_oracle_props.py -- for larger N).
C5 (2D Poisson, N = 1M) is checked through size-independent properties:
A x = b residual and agreement with the known x_true, f64, tolerance 1e-6
relative as BASELINE.json states.
"""

import numpy as np
import pytest

from basic_sparse_matrix_amd import Csr, Dense, MatErr, MatErrKind, Panic, backward_substitution, \
    forward_substitution, solve
from golden.golden_io import f32, matrix, scalars
from nd_support import csr_arrays

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def assert_csr_exact(got: Csr, rp, ci, v):
    assert np.array_equal(np.asarray(got.row_index, np.uint64), np.asarray(rp, np.uint64))
    assert np.array_equal(np.asarray(got.col_index, np.uint64), np.asarray(ci, np.uint64))
    assert np.array_equal(bits(got.v), bits(np.asarray(v, dtype=got.dtype)))


# ----------------------------------------------------- reference goldens
def test_cholesky_decomposition_0(golden):
    g = golden["cholesky_decomposition_0"]
    m = Csr.from_data(matrix(g["rows"], np.float32), dtype=np.float32)
    lower = m.cholesky_decomp()
    upper = lower.transpose()
    assert lower == Csr.from_data(matrix(g["l_rows"], np.float32), dtype=np.float32)  # sparse.rs:1058
    assert upper == Csr.from_data(matrix(g["u_rows"], np.float32), dtype=np.float32)  # sparse.rs:1059


def test_cholesky_decomposition_1(golden):
    g = golden["cholesky_decomposition_1"]
    m = Csr.from_data(matrix(g["rows"], np.float32), dtype=np.float32)
    assert m.cholesky_decomp() == Csr.from_data(matrix(g["l_rows"], np.float32), dtype=np.float32)


def test_cholesky_non_square():
    with pytest.raises(MatErr) as e:
        Csr.from_data([[1.0, 2.0, 3.0]], dtype=np.float32).cholesky_decomp()
    assert e.value.kind == MatErrKind.NonSquareMatrix


def test_forward_substitution_golden(golden):
    g = golden["forward_substitution_test_0"]
    b = Dense.from_data([scalars(c, np.float32) for c in g["b_cols"]], dtype=np.float32)
    l = Csr.from_data(matrix(g["l_rows"], np.float32), dtype=np.float32)
    y = forward_substitution(l, b)
    assert bits(y.get_col(0)).tolist() == bits(np.asarray([f32(s) for s in g["y_cols"][0]], np.float32)).tolist()


def test_backward_substitution_golden(golden):
    g = golden["backward_substitution_test_0"]
    y = Dense.from_data([scalars(c, np.float32) for c in g["y_cols"]], dtype=np.float32)
    u = Csr.from_data(matrix(g["u_rows"], np.float32), dtype=np.float32)
    x = backward_substitution(u, y)
    assert bits(x.get_col(0)).tolist() == bits(np.asarray([f32(s) for s in g["x_cols"][0]], np.float32)).tolist()


def test_solve_golden(golden):
    g = golden["solve_test"]
    b = Dense.from_data([scalars(c, np.float32) for c in g["b_cols"]], dtype=np.float32)
    a = Csr.from_data(matrix(g["rows"], np.float32), dtype=np.float32)
    x = solve(a, b)
    x_ref = Dense.from_data([[f32(s) for s in g["x_cols"][0]]], dtype=np.float32)
    assert x == x_ref  # lib.rs:136, including 2.6999998
    assert bits(x.get_col(0)).tolist() == bits(x_ref.get_col(0)).tolist()


def test_solve_non_square_panics():
    with pytest.raises(Panic):
        solve(Csr.from_data([[1.0, 2.0]], dtype=np.float32), Dense.from_data([[1.0]], dtype=np.float32))


# ----------------------------------------------------- randomized parity
def random_spd(rng, n, density, dtype):
    """Symmetric, strictly diagonally dominant (hence SPD) sparse matrix."""
    a = np.zeros((n, n))
    mask = rng.random((n, n)) < density
    vals = rng.uniform(-1.0, 1.0, (n, n))
    a[mask] = vals[mask]
    a = np.tril(a, -1)
    a = a + a.T
    a[np.arange(n), np.arange(n)] = np.abs(a).sum(axis=1) + 1.0 + rng.random(n)
    return a.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,density", [(1, 1.0), (7, 0.5), (33, 0.2), (64, 0.05), (150, 0.1), (300, 0.02)])
def test_cholesky_random_vs_literal_oracle(orc, dtype, n, density):
    rng = np.random.default_rng(n)
    a = random_spd(rng, n, density, dtype)
    rp, ci, v = csr_arrays(a)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    L = A.cholesky_decomp()
    assert_csr_exact(L, *orc.cholesky(n, n, rp, ci, v, band=False))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("g", [3, 16, 40])
def test_poisson_cholesky_and_solve_vs_oracle(orc, dtype, g):
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    v = v.astype(dtype)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    band = g > 16
    L = A.cholesky_decomp()
    assert_csr_exact(L, *orc.cholesky(n, n, rp, ci, v, band=band))
    b = orc.gen_x_cols(1002, n, 2, dtype=dtype)
    x = solve(A, Dense.from_columns(b))
    ex = orc.solve(n, rp, ci, v, b, band=band)
    for j in range(2):
        assert bits(x.get_col(j)).tolist() == bits(ex[j]).tolist()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_csr_triangular_solves_vs_oracle(orc, dtype):
    """forward/backward_substitution on general (non-band) sorted CSR factors."""
    rng = np.random.default_rng(5)
    n = 700
    a = random_spd(rng, n, 0.01, dtype)
    rp, ci, v = csr_arrays(a)
    lrp, lci, lv = orc.cholesky(n, n, rp, ci, v, band=True)
    urp, uci, uv = orc.transpose(n, n, lrp, lci, lv)
    L = Csr.from_csr_arrays((n, n), lrp, lci, lv)
    U = Csr.from_csr_arrays((n, n), urp, uci, uv)
    b = orc.gen_x_cols(9, n, 3, dtype=dtype)
    y = forward_substitution(L, Dense.from_columns(b))
    ey = orc.forward_substitution(n, lrp, lci, lv, b)
    for j in range(3):
        assert bits(y.get_col(j)).tolist() == bits(ey[j]).tolist()
    x = backward_substitution(U, y)
    ex = orc.backward_substitution(n, urp, uci, uv, ey)
    for j in range(3):
        assert bits(x.get_col(j)).tolist() == bits(ex[j]).tolist()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("g", [5, 17, 40, 63, 100, 130, 260])
def test_poisson_cholesky_bandwidths_vs_oracle(orc, dtype, g):
    """band_chol5 gives the band oracle's factor bit for bit at every slot
    count M (bandwidths 5 .. 260: M = 1, 2, 4, 8), including bandwidths that
    are not a multiple of the 16-row tiles and last row-blocks that are cut
    short. M = 16 is pinned by the C5 fixture (below), M = 17 by the
    bandwidth-1060 solve."""
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    v = v.astype(dtype)
    expect = orc.cholesky(n, n, rp, ci, v, band=True)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    assert_csr_exact(A.cholesky_decomp(), *expect)


@pytest.mark.parametrize("delay", [8, -8])
@pytest.mark.parametrize("dtype,g", [(np.float64, 100), (np.float32, 63)])
def test_chol5_completion_with_late_waves_vs_oracle(orc, monkeypatch, dtype, g, delay):
    """a row-block is complete only when wave 0's factor AND
    the store waves' last-tile stores have landed. BSM_CHOL5_DELAY makes one
    side late in every row-block (d > 0: the store waves sleep ~d x 8k cycles
    before storing; d < 0: wave 0 before its drain), so a completion raised by
    the early side alone would let the next row-blocks read stale rows. The
    factor must still equal the band oracle bit for bit."""
    monkeypatch.setenv("BSM_CHOL5_DELAY", str(delay))
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    v = v.astype(dtype)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    assert_csr_exact(A.cholesky_decomp(), *orc.cholesky(n, n, rp, ci, v, band=True))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forward_helper_prefixes_vs_oracle(orc, dtype):
    """Bandwidth 200 > FW3_NEAR: the default forward solve takes the far
    prefixes of the rows' sums from helper workgroups; with 3 RHS columns
    (three solver/helper groups) and with one the solution equals the band
    oracle bit for bit."""
    g = 200
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    v = v.astype(dtype)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    b = orc.gen_x_cols(1004, n, 3, dtype=dtype)
    ex = orc.solve(n, rp, ci, v, b, band=True)
    x = solve(A, Dense.from_columns(b))
    for j in range(3):
        assert bits(x.get_col(j)).tolist() == bits(ex[j]).tolist()
    x1 = solve(A, Dense.from_columns(b[:1]))
    assert bits(x1.get_col(0)).tolist() == bits(ex[0]).tolist()


def test_poisson_250_bit_exact_solve_f64(orc):
    """62,500 unknowns, bandwidth 250: GPU solve == band oracle bit for bit."""
    g = 250
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    b = orc.gen_x_cols(1002, n, 1)
    x = solve(A, Dense.from_columns(b))
    ex = orc.solve(n, rp, ci, v, b, band=True)[0]
    assert bits(x.get_col(0)).tolist() == bits(ex).tolist()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wide_band_solve_vs_oracle(orc, dtype):
    """Bandwidth 1060 (> 1024: band_chol5's 17th accumulator slot and the
    32-term lane segments of the backward chain; bands up to 1073) on a
    short banded SPD system, bit-exact vs the band oracle."""
    n, g = 2400, 1060
    rows, cols, vals = [], [], []
    for i in range(n):
        for j, v in ((i - g, -1.0), (i - 1, -1.0), (i, 4.5), (i + 1, -1.0), (i + g, -1.0)):
            if 0 <= j < n:
                rows.append(i), cols.append(j), vals.append(v)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.uint64)
    ci = np.asarray(cols, dtype=np.uint64)
    v = np.asarray(vals, dtype=dtype)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    b = orc.gen_x_cols(1003, n, 1, dtype=dtype)
    x = solve(A, Dense.from_columns(b))
    ex = orc.solve(n, rp, ci, v, b, band=True)[0]
    assert bits(x.get_col(0)).tolist() == bits(ex).tolist()


def sha256_bits(a) -> str:
    import hashlib

    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def c5_system(orc):
    """C5: 1000 x 1000 grid (N = 1M, bandwidth 1000), b = A x_true with
    x_true from seed 1002, summed per row in entry order (as
    scripts/make_c5_fixture.py forms it)."""
    g = 1000
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    x_true = orc.gen_x_cols(1002, n, 1)[0]
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    b = np.zeros(n)
    np.add.at(b, rows, v * x_true[ci.astype(np.int64)])
    return n, rp, ci, v, rows, x_true, b


@pytest.mark.slow
def test_c5_poisson_1m_f64_bit_exact_vs_fixture(orc, golden_c5):
    """C5 at full size, pinned bit for bit: solve() equals the band oracle's
    x (tests/golden/c5_poisson_1000.json, made once in the build container by
    scripts/make_c5_fixture.py: ~17 min of CPU). Also the size-independent
    properties: x_true to 1e-6 relative and a tiny residual."""
    n, rp, ci, v, rows, x_true, b = c5_system(orc)
    assert sha256_bits(b) == golden_c5["sha256_b_f64_bits"]  # same right-hand side as the fixture
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    x = solve(A, Dense.from_columns([b])).get_col(0)
    stride = golden_c5["x_stride"]
    sample = np.asarray([int(h, 16) for h in golden_c5["x_sample_bits"]], dtype=np.uint64)
    assert np.array_equal(bits(x[::stride]), sample)
    assert sha256_bits(x) == golden_c5["sha256_x_f64_bits"]
    rel = np.linalg.norm(x - x_true) / np.linalg.norm(x_true)
    assert rel < 1e-6, rel
    r = np.zeros(n)
    np.add.at(r, rows, v * x[ci.astype(np.int64)])
    assert np.linalg.norm(r - b) / np.linalg.norm(b) < 1e-12


@pytest.mark.slow
def test_c5_cholesky_factor_vs_fixture(orc, golden_c5):
    """cholesky_decomp at C5 (1e9 nonzeros of L): nnz, the hashes of
    row_ptr / col_index / value bits, and sampled full rows all equal the
    band oracle's factor."""
    g = 1000
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    L = Csr.from_csr_arrays((n, n), rp, ci, v).cholesky_decomp()
    fx = golden_c5["L"]
    assert L.get_nnz() == fx["nnz"]
    lrp = np.asarray(L.row_index, dtype=np.uint64)
    for r, row in fx["rows"].items():
        r = int(r)
        s, e = int(lrp[r]), int(lrp[r + 1])
        assert np.asarray(L.col_index[s:e], dtype=np.int64).tolist() == row["cols"]
        assert bits(np.asarray(L.v[s:e])).tolist() == [int(h, 16) for h in row["bits"]]
    assert sha256_bits(lrp.astype(np.int64)) == fx["sha256_row_ptr_i64"]
    assert sha256_bits(np.asarray(L.v)) == fx["sha256_val_f64_bits"]
    assert sha256_bits(np.asarray(L.col_index).astype(np.int64)) == fx["sha256_col_i64"]


# ----------------------------------------------------- panics and robustness
def test_backward_substitution_column_past_rhs_panics():
    """L* with an entry in column 3 against a 3-row y: the reference indexes
    x.get_col(..)[3] (lib.rs:58) and panics; so must we (no read past x)."""
    u = Csr.from_data([[2.0, 1.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0], [0.0, 0.0, 3.0, 0.0], [0.0, 0.0, 0.0, 1.0]],
                      dtype=np.float64)
    y = Dense.from_data([[1.0, 2.0, 3.0]], dtype=np.float64)
    with pytest.raises(Panic):
        backward_substitution(u, y)
    # a first entry past the RHS is only the divisor (row[0].v), never an index: no panic
    u2 = Csr.from_data([[2.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 3.0, 0.0], [0.0, 0.0, 0.0, 1.0]],
                       dtype=np.float64)
    assert backward_substitution(u2, y).get_col(0).tolist() == [0.5, 2.0, 1.0]


def test_forward_substitution_column_past_rhs_panics():
    l = Csr.from_data([[2.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0], [0.0, 1.0, 3.0, 5.0], [0.0, 0.0, 0.0, 1.0]],
                      dtype=np.float64)
    b = Dense.from_data([[1.0, 2.0, 3.0]], dtype=np.float64)
    with pytest.raises(Panic):
        forward_substitution(l, b)


def test_short_rhs_column_panics():
    """A ragged Dense (a column shorter than row_count) panics where the
    reference's index would, instead of reading past the host buffer."""
    l = Csr.from_data([[2.0, 0.0], [1.0, 1.0]], dtype=np.float64)
    b = Dense(1, 2, [np.asarray([1.0])])
    with pytest.raises(Panic):
        forward_substitution(l, b)
    a = Csr.from_data([[1.0, 0.0, 2.0], [0.0, 1.0, 0.0]], dtype=np.float64)
    with pytest.raises(Panic):  # entry in column 2 reaches past a 2-long column
        a.mul_dense(Dense(1, 3, [np.asarray([1.0, 2.0])]))
    a2 = Csr.from_data([[1.0, 1.0, 0.0], [0.0, 1.0, 0.0]], dtype=np.float64)
    got = a2.mul_dense(Dense(1, 3, [np.asarray([1.0, 2.0])]))  # column 2 never read: fine
    assert np.asarray(got.v).tolist() == [3.0, 2.0]


def test_cholesky_finishes_beside_a_kernel_holding_cus(orc):
    """The persistent factor kernels take row-blocks by atomic ticket, so
    they finish (bit-exact) while other work holds part of the GPU: large f64
    GEMMs queued on a torch side stream run concurrently on the CUs."""
    import torch

    g = 150
    n = g * g
    rp, ci, v = orc.poisson2d(g)
    expect = orc.cholesky(n, n, rp, ci, v, band=True)
    side = torch.cuda.Stream()
    m = torch.rand(6144, 6144, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(12):
            m = m @ m
            m = m / m.abs().max()
    L = Csr.from_csr_arrays((n, n), rp, ci, v).cholesky_decomp()
    busy = not side.query()  # the GEMMs were still running when the factor returned
    side.synchronize()
    assert_csr_exact(L, *expect)
    print(f"side stream still busy after the factor: {busy}")
