"""What the GPU tests of the band solvers rely on, checked without a GPU:
the systems of band_support.py have exactly the bandwidth asked for and a
small condition number (the blocked tests' bars assume kappa_2 <= 64), the
longdouble truth solves them, and the band oracle -- the GPU tests' reference
at sizes the literal O(N^3) oracle cannot reach -- equals the literal oracle
bit for bit on such bands, holes and exact zeros in L included."""

import numpy as np
import pytest

import band_support as bs
from nd_support import assert_same, csr_arrays

SMALL = tuple(s for s in bs.edge_systems() + bs.blocked_systems() if s[1] <= 500)


def test_edge_coverage():
    bs.assert_edge_coverage()


@pytest.mark.parametrize("kind,n,b,fill", SMALL, ids=lambda v: str(v))
def test_bandwidth_symmetry_and_condition(kind, n, b, fill):
    a = bs.system(kind, n, b, fill)
    assert bs.bandwidth(a) == b
    assert np.array_equal(a, a.T)
    assert np.linalg.cond(a) <= 64
    for dtype in (np.float32, np.float64):  # the rounded matrix keeps the pattern
        assert np.array_equal(a.astype(dtype) != 0, a != 0)
    if kind == "band":
        i = np.arange(b, n)
        assert np.all(a[i, i - b] != 0)  # every entry at distance exactly b
        if fill == 1.0:
            assert np.count_nonzero(a) == n + 2 * sum(n - d for d in range(1, b + 1))
    else:
        assert np.count_nonzero(np.tril(a, -2)) == 1


@pytest.mark.parametrize("n,b", [(1100, 1024), (1120, 1072)])
def test_wide_band_condition(n, b):
    a = bs.system("band", n, b, 0.5)
    assert bs.bandwidth(a) == b and np.linalg.cond(a) <= 64


@pytest.mark.parametrize("kind,n,b,fill", [("band", 1, 0, 1.0), ("band", 65, 1, 1.0), ("band", 129, 65, 1.0),
                                           ("band", 200, 129, 0.6), ("spike", 200, 65, 1.0)])
def test_longdouble_truth(kind, n, b, fill):
    """solve_longdouble's residual is at longdouble rounding, far below the
    1e-16 that the f64 bars resolve."""
    a = bs.system(kind, n, b, fill)
    rhs = np.random.default_rng(3).uniform(-1.0, 1.0, (n, 2))
    x = bs.solve_longdouble(a, b, rhs)
    r = a.astype(np.longdouble) @ x - rhs
    assert x.dtype == np.longdouble
    assert float(np.linalg.norm(r)) <= 1e-17 * np.linalg.norm(rhs)
    assert np.allclose(x.astype(np.float64), np.linalg.solve(a, rhs), rtol=1e-12, atol=0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,n,b,fill", [("band", 2, 0, 1.0), ("band", 3, 1, 1.0), ("band", 18, 17, 1.0),
                                           ("band", 130, 64, 1.0), ("band", 300, 129, 1.0), ("band", 67, 50, 0.3),
                                           ("band", 200, 113, 0.3), ("band", 300, 241, 0.3), ("spike", 130, 64, 1.0),
                                           ("spike", 300, 192, 1.0)], ids=lambda v: str(v))
def test_band_oracle_equals_literal_oracle(orc, dtype, kind, n, b, fill):
    rp, ci, v = csr_arrays(bs.system(kind, n, b, fill).astype(dtype))
    band = orc.cholesky(n, n, rp, ci, v, band=True)
    lit = orc.cholesky(n, n, rp, ci, v, band=False)
    assert_same(band, lit, "L")
    if kind == "spike":  # exact zeros inside L's band: far fewer entries than the full band
        assert len(band[2]) < n * (b + 1) // 2
    rhs = orc.gen_x_cols(1011, n, 3, dtype=dtype)
    assert_same(orc.solve(n, rp, ci, v, rhs, band=True), orc.solve(n, rp, ci, v, rhs, band=False), "x")
