"""cholesky_decomp() and solve() in reference order at every edge of their
kernel selection, on bands whose rows all differ (band_support.py: a Poisson
stencil's factor tends to a stationary limit, where a neighbour's block or two
swapped blocks change almost nothing).

Bar: the project's own, bit-exact. The factor equals orc.cholesky(band=True)
in row_ptr, col and value bits, the solution equals orc.solve(band=True) bit
for bit, f32 and f64 (test_band_systems.py pins the band oracle to the literal
one on such systems).

The bandwidths (band_support.EDGE_BANDWIDTHS, with the source lines they come
from) sit on both sides of every selection: band_walk_cfg's nine
band_backward_reg instantiations, launch_chol5's six slot counts, the forward
selection at FW3_NEAR, the 16-row tiles, and the band limit (1072: the band
kernels, 1073: chol_general and the CSR solves, same oracle bits). The rows
per bandwidth (band_support.edge_rows) are n = b + 1 (no row has its full
band), b + 2, b + 66 and 1153 = 18 * 64 + 1: both parities of n and of
n - 1 - b, which choose the branches of band_backward_reg's masked loop, full
loop and lone row 0. One test per (bandwidth, dtype) runs its row counts with
k = 1 and k = 3 right-hand columns, so each stays at a few seconds (most of
them the oracle's)."""

import numpy as np
import pytest

import band_support as bs
from basic_sparse_matrix_amd import Csr, Dense, solve
from nd_support import cols_of, csr_arrays, csr_parts, same_bits

pytestmark = pytest.mark.gpu

bs.assert_edge_coverage()  # each edge on both sides, both parities of n and of n - 1 - b per backward configuration


def check(orc, kind, n, b, fill, dtype, ks):
    rp, ci, v = csr_arrays(bs.system(kind, n, b, fill).astype(dtype))
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    what = (kind, n, b, np.dtype(dtype).name)
    lrp, lci, lv = orc.cholesky(n, n, rp, ci, v, band=True)
    got = csr_parts(A.cholesky_decomp())
    assert np.array_equal(got[0].astype(np.uint64), lrp), what
    assert np.array_equal(got[1].astype(np.uint64), lci), what
    assert same_bits(got[2], lv), what
    kmax = max(ks)
    rhs = orc.gen_x_cols(1000 + n, n, kmax, dtype=dtype)
    ex = orc.solve(n, rp, ci, v, rhs, band=True)
    for k in ks:
        x = cols_of(solve(A, Dense.from_columns(rhs[:k])))
        assert len(x) == k
        for j in range(k):
            assert same_bits(x[j], ex[j]), what + (k, j)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("b", bs.EDGE_BANDWIDTHS)
def test_band_edges_factor_and_solve_vs_oracle(orc, dtype, b):
    """band_spd (every row its own scale; half the band's entries missing
    above b = 128) at each selection edge, k = 1 and k = 3; at b = 64, 193 and
    513 also k = 17, where k (1 + FW3_HELPERS) > 256 sends a wide band to the
    one-workgroup forward solve."""
    ks = (1, 3) + ((bs.MANY_COLUMNS[b],) if b in bs.MANY_COLUMNS else ())
    for n in bs.edge_rows(b):
        check(orc, "band", n, b, bs.edge_fill(b), dtype, ks)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("b", bs.SPIKE_BANDWIDTHS)
def test_spike_bands_factor_and_solve_vs_oracle(orc, dtype, b):
    """One per backward configuration: a tridiagonal matrix whose single
    entry (r, r - b) sets the bandwidth, so L has exact zeros inside its band
    (not stored: the factor's pattern is checked too) and rows that start at
    different columns."""
    for n in bs.spike_rows(b):
        check(orc, "spike", n, b, 1.0, dtype, (1, 3))
