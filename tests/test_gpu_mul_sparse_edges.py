"""Csr::mul_sparse (sparse.rs:601-635) on the GPU at the edges of
sparse_mul_dispatch (csrc/kernels_sparse.hip): every count that sizes a
256-thread grid or a 4096-entry scan tile placed on and around that size,
every phase empty, owner_of over runs of equal offsets, keys of up to 46
bits with the top bit of either field in use, the values that decide what is
kept, the 2^32 refusal, results fed onward on the device, and the zero
dimensions at which the reference panics.

The operands and what each is meant to hit are in tests/mul_sparse_support.py
(held to it on the CPU by tests/test_mul_sparse_support.py). The expected
result is the oracle's where a.rows x b.cols <= 2^22 and the pruned merge
mul_sparse_pairs beyond; the bar is bit-exact row_index, columns and values.

Left out: b.cols = 2^31 - 1 (the transpose of rhs alone needs a 16 GiB
row_index) and the largest accepted expansion, 2^32 - 2 products (64 GiB of
keys and their sorted copy)."""

import numpy as np
import pytest

import mul_sparse_support as S
from basic_sparse_matrix_amd import Csr, Dense, Panic, _lib
from test_gpu_sparse_addsub_paths import assert_csr_bits_or_nan
from test_gpu_spmm import assert_csr_bits

pytestmark = pytest.mark.gpu


def to_csr(t):
    return Csr.from_csr_arrays((t[0], t[1]), t[2], t[3], t[4])


def expected(orc, name):
    a, b = S.operands(name)
    return orc.mul_sparse(a, b) if S.oracle_can(a, b) else S.pairs_reference(name)


def run_case(orc, name):
    a, b = S.operands(name)
    got = to_csr(a).mul_sparse(to_csr(b))
    assert got.dims.as_tuple() == (a[0], b[1])
    cmp = assert_csr_bits_or_nan if S.CASES[name].generates_nan else assert_csr_bits
    cmp(got, *expected(orc, name))
    return got


@pytest.mark.parametrize("name", S.names("size"))
def test_size_edges(orc, name):
    """nnz_a, total and n_cand on 1, 255, 256, 257, 4095, 4096 and 4097 with
    255 to 257 rows; kept outputs on both sides of candidate positions 256
    and 4096 with dropped ones among them."""
    run_case(orc, name)


@pytest.mark.parametrize("name", S.names("empty"))
def test_empty_phases(orc, name):
    """No entry in a, none in b, none that expands, or candidates that all
    cancel: row_index is rows + 1 zeros."""
    got = run_case(orc, name)
    assert S.CASES[name].expect["nnz"] == 0
    assert np.asarray(got.row_index).tolist() == [0] * (got.dims.rows + 1) and len(got.v) == 0


@pytest.mark.parametrize("name", S.names("offsets"))
def test_offset_runs(orc, name):
    run_case(orc, name)


@pytest.mark.parametrize("name", S.names("key"))
def test_key_width(orc, name):
    run_case(orc, name)


@pytest.mark.parametrize("name", S.names("wide"))
def test_wide_keys(orc, name):
    """46-bit and 34-bit keys against mul_sparse_pairs."""
    a, b = S.operands(name)
    assert not S.oracle_can(a, b)
    run_case(orc, name)


@pytest.mark.parametrize("name", S.names("values"))
def test_value_edges(orc, name):
    """A subnormal the GPU flushed, or a zero it kept, moves row_index."""
    run_case(orc, name)


def test_refusal_leaves_the_handles_usable(orc):
    a, b = S.operands("refusal")
    ca, cb = to_csr(a), to_csr(b)
    with pytest.raises(_lib.BsmError, match="expanded products") as e:
        ca.mul_sparse(cb)
    assert e.value.code == _lib.BSM_ERR_UNSUPPORTED
    small = S.csr(1, 3, [3], [2, 0, 2], np.array([3, 5, 7], np.uint32))
    assert_csr_bits(ca.mul_sparse(to_csr(small)), *orc.mul_sparse(a, small))
    assert_csr_bits(cb.transpose(), *orc.transpose(*b))


# ---- results fed onward -------------------------------------------------------
def tup(dims, res):
    return (dims[0], dims[1], *res)


@pytest.mark.parametrize("dtype", [np.float64, np.int32])
def test_chained_results(orc, dtype):
    """A device-built result keeps its handle and is analysed lazily: each
    step of each chain against the oracle's own chain."""
    o = S.chain_operands(dtype)
    a, b, c, d, d2 = (o[k] for k in "a b c d d2".split())
    A, B, C, D, D2 = (to_csr(x) for x in (a, b, c, d, d2))
    ab_ref = tup((a[0], b[1]), orc.mul_sparse(a, b))

    def fresh():
        ab = A.mul_sparse(B)
        assert_csr_bits(ab, *ab_ref[2:])
        return ab

    assert_csr_bits(fresh().mul_sparse(C), *orc.mul_sparse(ab_ref, c))
    assert_csr_bits(fresh().add_sparse(D), *orc.add_sparse(ab_ref, d))
    assert_csr_bits(D.sub_sparse(fresh()), *orc.sub_sparse(d, ab_ref))
    assert_csr_bits(fresh().transpose(), *orc.transpose(*ab_ref))
    s_ref = tup((a[0], a[1]), orc.add_sparse(a, d2))
    s = A.add_sparse(D2)
    assert_csr_bits(s, *s_ref[2:])
    assert_csr_bits(s.mul_sparse(B), *orc.mul_sparse(s_ref, b))
    t_ref = tup((a[1], a[0]), orc.transpose(*a))
    t = A.transpose()
    assert_csr_bits(t, *t_ref[2:])
    assert_csr_bits(t.mul_sparse(D), *orc.mul_sparse(t_ref, d))
    assert_csr_bits(fresh().mul_dense(Dense.from_columns(o["x"])), *orc.mul_dense(*ab_ref, o["x"]))


# ---- zero dimensions ----------------------------------------------------------
def no_entries(rows, cols, dtype=np.float64):
    return Csr.from_csr_arrays((rows, cols), np.zeros(rows + 1, np.uint64), np.zeros(0, np.uint64),
                               np.zeros(0, dtype))


def test_zero_dimensions_panic_like_the_reference():
    """self.rows == 0: the result's finalise panics (sparse.rs:209-211, 634).
    rhs.cols == 0: rhs.transpose() builds a matrix of 0 rows and its finalise
    panics (:317, :603). The same for a public transpose of 0 columns."""
    b = Csr.from_data([[1.0, 2.0, 0.0], [0.0, 3.0, 4.0]])
    with pytest.raises(Panic, match="big eek"):
        no_entries(0, 2).mul_sparse(b)
    with pytest.raises(Panic, match="big eek"):
        b.mul_sparse(no_entries(3, 0))
    with pytest.raises(Panic, match="big eek"):
        no_entries(0, 2).mul_sparse(no_entries(2, 1))  # was a 0 x 1 result
    with pytest.raises(Panic, match="big eek"):
        Csr.new((3, 0), np.float64).finalise().transpose()
    with pytest.raises(Panic, match="big eek"):
        no_entries(3, 0, np.int32).transpose()
    # neither check touches the neighbours: one row, one column
    t = no_entries(3, 1).transpose()
    assert t.dims.as_tuple() == (1, 3) and np.asarray(t.row_index).tolist() == [0, 0]
    out = no_entries(1, 2).mul_sparse(b)
    assert out.dims.as_tuple() == (1, 3) and np.asarray(out.row_index).tolist() == [0, 0]
