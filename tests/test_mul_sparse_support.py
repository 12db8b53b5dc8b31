"""The mul_sparse edge cases (tests/mul_sparse_support.py) hold what their
table says, and the pruned reference equals the oracle wherever the oracle
can go. No GPU: this is the only place where a case's sizes are asserted,
so that the GPU tests never take an expectation from the code under test."""

import numpy as np
import pytest

import mul_sparse_support as S


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view(f"u{v.dtype.itemsize}")


@pytest.mark.parametrize("name", [n for n in S.CASES if n != "refusal" and S.oracle_can(*S.operands(n))])
def test_pairs_reference_equals_oracle(orc, name):
    """Bit for bit, NaN payloads included (both run on the host), on every
    case of at most 2^22 (row, column) pairs."""
    a, b = S.operands(name)
    rp, ci, v = S.pairs_reference(name)
    erp, eci, ev = orc.mul_sparse(a, b)
    assert np.array_equal(rp, erp) and np.array_equal(ci, eci)
    assert v.dtype == ev.dtype and np.array_equal(bits(v), bits(ev))
    assert bool(np.isnan(ev).any()) == S.CASES[name].generates_nan if ev.dtype.kind == "f" else True


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_sits_on_its_edge(name):
    case = S.CASES[name]
    a, b = S.operands(name)
    if name == "refusal":
        assert S.mul_counts(a, b) == {**case.expect, "n_cand": None, "nnz": None}
        return
    ref = S.pairs_reference(name)
    counts = S.mul_counts(a, b, ref)
    for key, want in case.expect.items():
        assert counts[key] == want, (key, counts)
    if case.more_total_than_cand:
        assert counts["total"] > counts["n_cand"]
    if case.kept_at or case.dropped_at:
        keep = S.mul_keep_flags(a, b, ref)
        assert keep[list(case.kept_at)].all() and not keep[list(case.dropped_at)].any()
    assert max(len(a[4]), len(b[4])) <= 70_000


def test_size_family_covers_every_edge():
    """One case per N in E for each of nnz_a, total and n_cand, in f64 and
    u32; all six scalar types at 256 and 4096; rows on 255, 256 and 257."""
    for n in S.E:
        for q in ("nnz_a", "total", "n_cand"):
            have = {k.rsplit("-", 1)[1] for k in S.CASES if k.startswith(f"{q}={n}-")}
            want = {S.name_of(d) for d in (S.DTYPES if n in (256, 4096) else [np.float64, np.uint32])}
            assert have == want, (q, n)
    assert {S.operands(f"n_cand={n}-float64")[0][0] for n in S.E} == {255, 256, 257}


def test_offsets_case_shape():
    a, b = S.operands("offsets-float64")
    rp, ci = np.asarray(a[2], np.int64), np.asarray(a[3], np.int64)
    lens, blen = np.diff(rp), np.diff(np.asarray(b[2], np.int64))
    assert not lens[:3].any() and not lens[15:25].any() and not lens[37:].any() and lens[3] and lens[36]
    dead = lambda k: k >= b[0] or blen[k] == 0  # noqa: E731
    assert all(dead(k) for k in ci[:3]) and all(dead(k) for k in ci[-3:])
    assert a[1] > b[0] and {b[0] - 1, b[0], a[1] - 1} <= set(ci.tolist())
    assert not dead(b[0] - 1)
    sorted_rows = lambda m: all(np.all(np.diff(np.asarray(m[3], np.int64)[s:e]) > 0)  # noqa: E731
                                for s, e in zip(np.asarray(m[2], np.int64)[:-1], np.asarray(m[2], np.int64)[1:]))
    assert not sorted_rows(a) and not sorted_rows(b)


@pytest.mark.parametrize("name", S.names("key", "wide"))
def test_key_cases_touch_both_corners(name):
    """Row 0 and the last row, column 0 and the last column are all among
    the results (not only among the candidates), and the first rhs row of
    two entries holds the last column before column 0."""
    a, b = S.operands(name)
    rp, ci, _ = S.pairs_reference(name)
    rows = np.repeat(np.arange(a[0]), np.diff(np.asarray(rp, np.int64)))
    got = set(zip(rows.tolist(), np.asarray(ci, np.int64).tolist()))
    for corner in [(0, 0), (0, b[1] - 1), (a[0] - 1, 0), (a[0] - 1, b[1] - 1)]:
        assert corner in got, corner
    s = int(b[2][2])
    assert np.asarray(b[3][s:s + 2], np.int64).tolist() == [b[1] - 1, 0]
    if name in ("wide46-float64", "wide34-uint32"):
        assert np.count_nonzero(np.diff(np.asarray(a[2], np.int64))) < 50 and len(np.unique(b[3])) < 16


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_float_values_reach_every_outcome(dtype):
    name = f"values-{S.name_of(dtype)}"
    a, b = S.operands(name)
    rp, ci, v = S.pairs_reference(name)
    rows = np.repeat(np.arange(a[0]), np.diff(np.asarray(rp, np.int64)))
    at = {(int(r), int(c)): x for r, c, x in zip(rows, ci, v)}
    fi = np.finfo(dtype)
    sub, tiny, big, pos, minus = 5, 6, 7, 8, 9  # positions in float_specials
    assert 0 < at[(sub, pos)] < fi.tiny and at[(sub, minus)] < 0  # subnormal product, kept
    assert (tiny, tiny) not in at and (sub, sub) not in at  # underflow to zero, dropped
    assert at[(big, big)] == np.inf and at[(big, minus)] == -np.inf  # overflow, kept
    assert np.isnan(at[(3, 0)]) and np.isnan(at[(1, 4)])  # Inf x 0, kept
    assert np.isnan(at[(2, pos)]) and np.isnan(at[(pos, 2)])  # stored NaN
    assert (0, pos) not in at and (1, minus) not in at  # +-0 x finite, dropped
    assert np.isnan(at[(10, 10)])  # Inf + -Inf, kept
    assert (11, 11) not in at  # exact cancellation, dropped
    assert at[(12, 12)] not in (0, np.dtype(dtype).type(3.3), np.dtype(dtype).type(33.3))  # the order of the sum shows


@pytest.mark.parametrize("dtype", [np.int32, np.uint32, np.int64, np.uint64])
def test_int_values_reach_every_outcome(dtype):
    name = f"values-{S.name_of(dtype)}"
    a, b = S.operands(name)
    rp, ci, v = S.pairs_reference(name)
    rows = np.repeat(np.arange(a[0]), np.diff(np.asarray(rp, np.int64)))
    at = {(int(r), int(c)): int(x) for r, c, x in zip(rows, ci, v)}
    info = np.iinfo(dtype)
    bits_n = np.dtype(dtype).itemsize * 8
    wrap = lambda x: (x - info.min) % (1 << bits_n) + info.min  # noqa: E731
    assert at[(0, 0)] == wrap(info.max * info.max) == 1  # extreme x extreme
    assert (3, 3) not in at  # 2^(bits/2) squared wraps to exactly 0
    if info.min < 0:
        assert at[(1, 2)] == info.min and (1, 1) not in at  # min x -1 = min; min x min = 0
    assert (6, 6) not in at  # two products whose wrapped sum is 0
    assert at[(7, 7)] == wrap(2 * info.max) != 0  # a wrapped sum that is not
