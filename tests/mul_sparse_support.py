"""Operands that place Csr::mul_sparse (sparse.rs:601-635) on its edges, and
a reference that can follow them to sizes the oracle cannot.

The device path (sparse_mul_dispatch) counts, per stored entry (i, k) of
self, the length of rhs row k (`total` expanded products), packs each
product's (i, j) into a 64-bit key, sorts and uniques the keys (`n_cand`
candidates), runs the reference's merge once per candidate and keeps the
results that are not T::default() (`nnz`). Every generator below builds a
pair of operands so that one of these quantities, a key field or a value
lands where the code changes its path; CASES records which, and
tests/test_mul_sparse_support.py holds every case to it on the CPU.

An operand is the tuple the oracle takes: (rows, cols, row_index u64,
col_index u64, values). Stored zeros, unsorted rows and repeated columns
are all legal (Csr.from_csr_arrays adopts them as they are)."""

import functools
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

DTYPES = [np.float64, np.float32, np.int32, np.uint32, np.int64, np.uint64]
E = (1, 255, 256, 257, 4095, 4096, 4097)  # grid (256) and scan-tile (4096) boundaries
ORACLE_PAIRS_MAX = 1 << 22  # the oracle visits a.rows x b.cols pairs and allocates as many outputs


def name_of(dtype):
    return np.dtype(dtype).name


# ------------------------------------------------------------- the reference
def mul_sparse_pairs(a, b):
    """The reference's merge (sparse.rs:604-632), run only over the pairs
    (non-empty row of a, column that occurs in b), in row-major order. For
    any other pair the loop guard `col_position != col.len() && row_position
    != row.len()` fails at once and val stays T::default(), which is never
    inserted: the pruning drops nothing the reference keeps and changes no
    value. rhs^T is the stable sort of b's entries by column (:296-318).
    Arithmetic is the operand's numpy scalar type (integers wrap)."""
    ar, _, arp, aci, av = a
    br, _, brp, bci, bv = b
    av = np.ascontiguousarray(av)
    dt = av.dtype
    bv = np.ascontiguousarray(bv, dtype=dt)
    arp = np.asarray(arp, np.int64)
    brp = np.asarray(brp, np.int64)
    acol = np.asarray(aci, np.int64).tolist()
    bcol = np.asarray(bci, np.int64)
    order = np.argsort(bcol, kind="stable")
    jcols, start = np.unique(bcol[order], return_index=True)
    end = np.append(start[1:], len(order))
    trow = np.repeat(np.arange(br, dtype=np.int64), np.diff(brp))[order].tolist()
    tv = bv[order]
    cols_of = list(zip(jcols.tolist(), start.tolist(), end.tolist()))
    zero = dt.type(0)
    out_row, out_col, out_v = [], [], []
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(np.diff(arp)).tolist():
            p0, p1 = int(arp[i]), int(arp[i + 1])
            for j, q0, q1 in cols_of:
                p, q, val = p0, q0, zero
                while q != q1 and p != p1:
                    ca, ct = acol[p], trow[q]
                    if ca == ct:
                        val = val + av[p] * tv[q]
                        p += 1
                        q += 1
                    elif ca > ct:
                        q += 1
                    else:
                        p += 1
                if val != zero:  # NaN != 0: kept
                    out_row.append(i)
                    out_col.append(j)
                    out_v.append(val)
    counts = np.bincount(np.asarray(out_row, np.int64), minlength=ar)
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return rp, np.asarray(out_col, np.uint64), np.asarray(out_v, dtype=dt)


def mul_candidates(a, b, limit=1 << 24):
    """(nnz_a, total, sorted distinct candidate keys i * b.cols + j) as
    sparse_mul_dispatch computes them: entry (i, k) of a expands to the
    columns of rhs row k when k < b.rows, to nothing otherwise. The keys are
    None above `limit` products."""
    ar, _, arp, aci, _ = a
    br, bc, brp, bci, _ = b
    arp = np.asarray(arp, np.int64)
    brp = np.asarray(brp, np.int64)
    k = np.asarray(aci, np.int64)
    blen = np.diff(brp)
    cnt = np.where(k < br, blen[np.minimum(k, br - 1)], 0) if len(k) else np.zeros(0, np.int64)
    total = int(cnt.sum())
    if total > limit:
        return len(k), total, None
    row_of = np.repeat(np.arange(ar, dtype=np.int64), np.diff(arp))
    e = np.repeat(np.arange(len(k), dtype=np.int64), cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    j = np.asarray(bci, np.int64)[brp[k[e]] + within] if total else np.zeros(0, np.int64)
    return len(k), total, np.unique(row_of[e] * bc + j)


def mul_keep_flags(a, b, ref):
    """Per candidate, in the sorted order the device holds them: True where
    the reference result `ref` (row_index, col, v) has an entry."""
    _, _, keys = mul_candidates(a, b)
    rp = np.asarray(ref[0], np.int64)
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    kept = rows * b[1] + np.asarray(ref[1], np.int64)
    assert np.all(np.isin(kept, keys)), "a kept entry that is no candidate"
    return np.isin(keys, kept)


def mul_counts(a, b, ref=None):
    """{nnz_a, total, n_cand, nnz}; n_cand and nnz are None when the
    expansion is too large to enumerate (the refusal case)."""
    nnz_a, total, keys = mul_candidates(a, b)
    if keys is None:
        return {"nnz_a": nnz_a, "total": total, "n_cand": None, "nnz": None}
    ref = mul_sparse_pairs(a, b) if ref is None else ref
    return {"nnz_a": nnz_a, "total": total, "n_cand": len(keys), "nnz": len(ref[2])}


# ------------------------------------------------------------------ builders
def csr(rows, cols, lens, ci, v):
    rp = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.uint64)
    ci = np.asarray(ci, np.uint64)
    v = np.ascontiguousarray(v)
    assert len(rp) == rows + 1 and int(rp[-1]) == len(ci) == len(v)
    assert not len(ci) or int(ci.max()) < cols
    return rows, cols, rp, ci, v


def from_rows(rows, cols, by_row, dtype):
    """by_row: {row: [(col, value), ...]} in storage order."""
    lens = np.zeros(rows, np.int64)
    ci, v = [], []
    for r in sorted(by_row):
        lens[r] = len(by_row[r])
        ci += [c for c, _ in by_row[r]]
        v += [x for _, x in by_row[r]]
    return csr(rows, cols, lens, ci, np.asarray(v, dtype=dtype) if v else np.zeros(0, dtype))


def rand_values(rng, dtype, n):
    """Non-zero: floats of magnitude in [0.25, 2) and either sign, integers
    over the type's whole range (products and sums wrap)."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.uniform(0.25, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(dt)
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    v[v == 0] = 1
    return v


def small_values(rng, dtype, n):
    """Non-zero and small enough that no product of two wraps or rounds."""
    return rng.integers(1, 8, n).astype(dtype)


def neg(x):
    """-x in x's own type (wrapping for the unsigned ones)."""
    with np.errstate(all="ignore"):
        return (np.zeros_like(x) - x).astype(x.dtype)


def spread(rng, n, rows, empty=()):
    """Row lengths that sum to n, rows in `empty` holding nothing."""
    allowed = np.setdiff1d(np.arange(rows), np.asarray(empty, np.int64))
    return np.bincount(rng.choice(allowed, n), minlength=rows)


def few_columns(rng, cols, extra=5):
    """Column 0, the last column (the only one with the top bit of the column
    field set when cols = 2^b + 1), their neighbours and a few random ones."""
    fixed = [0, cols - 1, cols // 2, (cols - 1) // 2, max(cols - 2, 0)]
    return np.unique(np.concatenate([fixed, rng.integers(0, cols, extra)])).astype(np.int64)


def random_rhs(rng, k_rows, cols, dtype, max_len=4, values=rand_values):
    """k_rows x cols, rows of 0..max_len entries (row 0 has one, row 1 none)
    drawn with repeats from few_columns; the first row of two or more
    entries starts with the last column, then column 0."""
    lens = rng.integers(0, max_len + 1, k_rows)
    lens[0] = 1
    if k_rows > 1:
        lens[1] = 0
    if k_rows > 2:
        lens[2] = max(2, max_len)
    distinct = few_columns(rng, cols)
    ci = distinct[rng.integers(0, len(distinct), int(lens.sum()))]
    if k_rows > 2:
        s = int(lens[:2].sum())
        ci[s:s + 2] = [cols - 1, 0]
    return csr(k_rows, cols, lens, ci, values(rng, dtype, len(ci)))


def rng_for(*key):
    return np.random.default_rng([int(x) for x in key])


def rows_for(n):
    return (255, 256, 257)[E.index(n) % 3]


# ---------------------------------------------------------------- size edges
def size_nnz_a(n, dtype):
    """a holds exactly n entries over rows_for(n) rows (some empty), columns
    in [0, b.rows + 2): the last two name no rhs row."""
    rng = rng_for(1, n, DTYPES.index(dtype))
    rows, k_rows = rows_for(n), 24
    b = random_rhs(rng, k_rows, 40, dtype)
    ci = rng.integers(0, k_rows + 2, n)
    ci[0] = 2  # a row of b that has entries: total > 0 even at n == 1
    return csr(rows, k_rows + 2, spread(rng, n, rows, empty=[1, rows - 1]), ci, rand_values(rng, dtype, n)), b


def size_total(n, dtype):
    """The rhs row lengths of a's entries sum to exactly n; one entry in
    eight expands to nothing (an empty rhs row, or a column >= b.rows)."""
    rng = rng_for(2, n, DTYPES.index(dtype))
    rows, k_rows = rows_for(n), 24
    b = random_rhs(rng, k_rows, 40, dtype)
    blen = np.diff(np.asarray(b[2], np.int64))
    ks, rem = [], n
    while rem:
        k = int(rng.choice(np.flatnonzero((blen > 0) & (blen <= rem))))
        ks.append(k)
        rem -= int(blen[k])
    dead = np.concatenate([np.flatnonzero(blen == 0), [k_rows, k_rows + 1]])
    ks = np.concatenate([ks, rng.choice(dead, len(ks) // 8 + 3)]).astype(np.int64)
    rng.shuffle(ks)
    return csr(rows, k_rows + 2, spread(rng, len(ks), rows, empty=[0, rows - 2]), ks,
               rand_values(rng, dtype, len(ks))), b


GROUP_WIDTHS = (1, 1, 1, 1, 2, 3, 4, 5, 7, 9)


def size_n_cand(n, dtype):
    """Exactly n distinct (i, j). rhs rows g and g + G both hold the columns
    of block g (widths GROUP_WIDTHS; row g repeats one of them), so a row of
    a that names groups S has sum(width[g], g in S) candidates however often
    it names them: through g, through g + G, through both (the same (i, j)
    by two k) or through g twice. total > n_cand always."""
    rng = rng_for(3, n, DTYPES.index(dtype))
    rows, g_n = rows_for(n), len(GROUP_WIDTHS)
    width = np.asarray(GROUP_WIDTHS)
    first = np.concatenate([[0], np.cumsum(width)]) + 3  # columns 0..2 and the last two stay empty
    cols = int(first[-1]) + 2
    b_rows = {}
    for g in range(g_n):
        block = np.arange(first[g], first[g + 1])
        one = rng.permutation(np.concatenate([block, block[:1]]) if width[g] > 1 else block)
        two = rng.permutation(block)
        b_rows[g] = list(zip(one.tolist(), rand_values(rng, dtype, len(one))))
        b_rows[g + g_n] = list(zip(two.tolist(), rand_values(rng, dtype, len(two))))
    b = from_rows(2 * g_n, cols, b_rows, dtype)
    sets = [[] for _ in range(rows)]
    order = [int(i) for i in rng.permutation(rows) if i not in (2, rows - 1)]
    rem = n
    while rem:
        before = rem
        for i in order:
            free = [g for g in range(g_n) if g not in sets[i] and width[g] <= rem]
            if free:
                g = int(rng.choice(free))
                sets[i].append(g)
                rem -= int(width[g])
                if not rem:
                    break
        assert rem < before, "the rows cannot hold this many candidates"
    a_rows, forced = {}, False
    for i in order:
        ks = []
        for g in sets[i]:
            variant = int(rng.integers(0, 4)) if forced else 2
            forced = True
            ks += [[g], [g + g_n], [g, g + g_n], [g, g]][variant]
        if ks:
            a_rows[i] = list(zip(ks, rand_values(rng, dtype, len(ks))))
    return from_rows(rows, 2 * g_n, a_rows, dtype), b


def cancelling(dtype, rows, live_rows, keep):
    """Sorted operands in which candidate (i, j) is x_i y_j + (-x_i) z_j: z_j
    = y_j where keep(j) is False (the sum is exactly zero, in every type, and
    the candidate is dropped) and 2 y_j where it is True (kept). 16 groups of
    8 columns: each live row has 128 candidates, columns 0..127 in order, so
    candidate position = 128 * (rank of the row) + j."""
    rng = rng_for(4, rows, len(live_rows), DTYPES.index(dtype))
    g_n, w = 16, 8
    a_rows, b_rows = {}, {}
    for i in live_rows:
        x = small_values(rng, dtype, 1)
        a_rows[i] = [(k, x[0]) for k in range(g_n)] + [(k, neg(x)[0]) for k in range(g_n, 2 * g_n)]
    for g in range(g_n):
        y = small_values(rng, dtype, w)
        js = list(range(g * w, (g + 1) * w))
        b_rows[g] = list(zip(js, y))
        b_rows[g + g_n] = [(j, y[t] * 2 if keep(j) else y[t]) for t, j in enumerate(js)]
    return from_rows(rows, 2 * g_n, a_rows, dtype), from_rows(2 * g_n, g_n * w, b_rows, dtype)


def cancel_straddle(dtype):
    """41 live rows among 257: 5248 candidates of which columns 0 and the odd
    ones are kept, so kept outputs sit at candidate positions 255 | 256 and
    4095 | 4096 (j = 127 | 0) with dropped ones before and between them."""
    live = [r for r in range(3, 257, 6)][:41]
    return cancelling(dtype, 257, live, lambda j: j == 0 or j % 2 == 1)


def cancel_all(dtype):
    """3 live rows of 128 candidates each, every one of them exactly zero."""
    return cancelling(dtype, 9, [1, 4, 7], lambda j: False)


# -------------------------------------------------------------- empty phases
def empty_a(dtype):
    rng = rng_for(5, DTYPES.index(dtype))
    return csr(5, 7, np.zeros(5), [], np.zeros(0, dtype)), random_rhs(rng, 7, 9, dtype)


def empty_b(dtype):
    rng = rng_for(6, DTYPES.index(dtype))
    a = csr(6, 7, spread(rng, 30, 6), rng.integers(0, 7, 30), rand_values(rng, dtype, 30))
    return a, csr(7, 9, np.zeros(7), [], np.zeros(0, dtype))


def total_zero(dtype, how):
    """a has 300 entries and none expands: every column is >= b.rows
    ("past"), names an empty rhs row ("empty_rows"), or either ("mixed")."""
    rng = rng_for(7, DTYPES.index(dtype), len(how))
    k_rows = 12
    lens = np.where(np.arange(k_rows) % 2 == 1, 3, 0)  # the even rhs rows are empty
    b = csr(k_rows, 9, lens, rng.integers(0, 9, int(lens.sum())), rand_values(rng, dtype, int(lens.sum())))
    past = np.arange(k_rows, k_rows + 5)
    empty_rows = np.arange(0, k_rows, 2)
    pool = {"past": past, "empty_rows": empty_rows, "mixed": np.concatenate([past, empty_rows])}[how]
    ci = rng.choice(pool, 300)
    if how == "mixed":
        ci[:2] = [k_rows, 0]
    return csr(7, k_rows + 5, spread(rng, 300, 7), ci, rand_values(rng, dtype, 300)), b


# ------------------------------------------------------------------- offsets
def offsets(dtype):
    """owner_of over runs of equal offsets. a (40 x 26): rows 0-2, 15-24 and
    37-39 are empty; its first three entries (row 3) and its last three (row
    36) expand to nothing; a.cols = b.rows + 6 with entries at k = b.rows -
    1, b.rows and a.cols - 1; unsorted rows with repeated columns on both
    sides."""
    rng = rng_for(8, DTYPES.index(dtype))
    k_rows, cols = 20, 30
    blen = rng.integers(1, 6, k_rows)
    blen[[0, 7, 8]] = 0
    blen[k_rows - 1] = 4
    b = csr(k_rows, cols, blen, rng.integers(0, 6, int(blen.sum())) * 5 + rng.integers(0, 2, int(blen.sum())),
            rand_values(rng, dtype, int(blen.sum())))
    a_cols = k_rows + 6
    lens = rng.integers(4, 12, 40)
    lens[[0, 1, 2] + list(range(15, 25)) + [37, 38, 39]] = 0
    ci = rng.integers(0, a_cols, int(lens.sum()))
    ci[:3] = [k_rows, 7, a_cols - 1]
    ci[3:6] = [k_rows - 1, k_rows - 1, 9]  # a repeated column right after the dead run
    ci[-3:] = [0, a_cols - 1, k_rows]
    ci[-6:-3] = [k_rows - 1, 3, k_rows - 1]
    return csr(40, a_cols, lens, ci, rand_values(rng, dtype, len(ci))), b


def long_candidate(dtype):
    """One candidate whose merge is long on both sides: row 1 of a has 3000
    unsorted entries over 2000 columns, column 0 of b 3000 entries (rhs rows
    repeat column 0), so rhs^T's row 0 repeats its keys too."""
    rng = rng_for(9, DTYPES.index(dtype))
    k_rows = 2000
    blen = np.full(k_rows, 2)
    blen[:1000] = 3
    bci = np.zeros(int(blen.sum()), np.int64)
    brp = np.concatenate([[0], np.cumsum(blen)])
    bci[brp[:-1]] = 1  # each rhs row: column 1, then column 0 twice (rows 0-999) or once
    assert int((bci == 0).sum()) == 3000
    b = csr(k_rows, 2, blen, bci, rand_values(rng, dtype, len(bci)))
    lens = [5, 3000, 0]
    ci = rng.integers(0, k_rows, 3005)
    return csr(3, k_rows, lens, ci, rand_values(rng, dtype, 3005)), b


# ----------------------------------------------------------------- key width
KEY_COLS = (1, 2, 3, 256, 257, 65536, 65537)
KEY_ROWS = (1, 2, 3, 256, 257)


def key_width(a_rows, b_cols, dtype, live=8):
    """Result dims a_rows x b_cols. a has entries in row 0, in the last row
    (the only one with the row field's top bit set when a_rows = 2^b + 1) and
    in up to `live` rows between; b's entries come from few_columns, the
    last column before column 0 inside a row."""
    rng = rng_for(10, a_rows, b_cols, DTYPES.index(dtype))
    k_rows = 16
    b = random_rhs(rng, k_rows, b_cols, dtype, max_len=5)
    rows_live = np.unique(np.concatenate([[0, a_rows - 1, a_rows // 2, (a_rows - 1) // 2],
                                          rng.integers(0, a_rows, live)]))
    lens = np.zeros(a_rows, np.int64)
    lens[rows_live] = rng.integers(1, 7, len(rows_live))
    lens[[0, a_rows - 1]] = 1
    ci = rng.integers(0, k_rows, int(lens.sum()))
    ci[0] = 2
    ci[-1] = 2  # rhs row 2 holds the last column and column 0: the four corners are results
    return csr(a_rows, k_rows, lens, ci, rand_values(rng, dtype, len(ci))), b


WIDE = {"wide46": (2**20 + 1, 2**24 + 1), "wide34": (65537, 65537)}


def wide(which, dtype):
    """46-bit and 34-bit keys: row 2^20 (or 65536) and the top column are the
    ones whose field has only its top bit set. Fewer than 50 live rows and 16
    distinct columns, so mul_sparse_pairs follows where the oracle cannot."""
    a_rows, b_cols = WIDE[which]
    return key_width(a_rows, b_cols, dtype, live=36)


# -------------------------------------------------------------------- values
def float_specials(dtype):
    fi = np.finfo(dtype)
    return np.array([0.0, -0.0, np.nan, np.inf, -np.inf, fi.smallest_subnormal, fi.tiny, fi.max, 1.7, -1.7],
                    dtype=dtype)


def float_values(dtype):
    """Rows 0-9 of a hold the specials at k = 0 and rhs row 0 holds them in
    columns 0-9: candidate (i, j) is specials[i] * specials[j]. That gives a
    subnormal product (subnormal x +-1.7, kept), tiny x tiny (0, dropped),
    max x max and max x -1.7 (+-Inf, kept), Inf x 0 (NaN, kept), stored NaN
    times anything (kept), +-0 x finite (dropped). Row 10: Inf + -Inf (NaN,
    kept). Row 11: x y + (-x) y (dropped). Row 12: big + small - big (small is 1.65 ulp of big), whose
    value depends on the order of the three products (kept)."""
    dt = np.dtype(dtype)
    s = float_specials(dt)
    big, small = (dt.type(1.7e16), dt.type(3.3)) if dt.itemsize == 8 else (dt.type(1.7e8), dt.type(33.3))
    one = dt.type(1.0)
    a_rows = {i: [(0, x)] for i, x in enumerate(s)}
    a_rows[10] = [(1, one), (2, one)]
    a_rows[11] = [(3, dt.type(1.7)), (4, dt.type(-1.7))]
    a_rows[12] = [(5, one), (6, one), (7, one)]
    b_rows = {0: [(j, x) for j, x in enumerate(s)], 1: [(10, dt.type(np.inf))], 2: [(10, dt.type(-np.inf))],
              3: [(11, dt.type(0.3))], 4: [(11, dt.type(0.3))], 5: [(12, big)], 6: [(12, small)],
              7: [(12, -big)]}
    return from_rows(14, 8, a_rows, dt), from_rows(8, 13, b_rows, dt)


def int_specials(dtype):
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    info = np.iinfo(dt)
    raw = [info.max, info.min, -1, 1 << (bits // 2), 1, 3]
    return np.array([x % (1 << bits) for x in raw], dtype=f"u{dt.itemsize}").view(dt)


def int_values(dtype):
    """Candidate (i, j), i, j < 6, is specials[i] * specials[j] at k = 0:
    extreme x extreme, min x -1, 2^(bits/2) squared (wraps to exactly 0,
    dropped; so does min x min in the signed types). Row 6: 2^(bits-1) +
    2^(bits-1) (two products whose wrapped sum is 0, dropped). Row 7: max +
    max (wraps to a non-zero value, kept)."""
    dt = np.dtype(dtype)
    s = int_specials(dt)
    bits = dt.itemsize * 8
    half = np.array([1 << (bits - 1)], dtype=f"u{dt.itemsize}").view(dt)[0]
    one = dt.type(1)
    a_rows = {i: [(0, x)] for i, x in enumerate(s)}
    a_rows[6] = [(1, one), (2, one)]
    a_rows[7] = [(3, one), (4, one)]
    b_rows = {0: [(j, x) for j, x in enumerate(s)], 1: [(6, half)], 2: [(6, half)], 3: [(7, s[0])], 4: [(7, s[0])]}
    return from_rows(8, 5, a_rows, dt), from_rows(5, 8, b_rows, dt)


# ------------------------------------------------------------------- refusal
def refusal():
    """65 536 stored entries of a in column 0 against an rhs row of 65 536
    entries: 2^32 expanded products, one more than sparse_mul_dispatch
    accepts (total < UINT32_MAX). The largest accepted size is not run: its
    keys and their sorted copy alone are 64 GiB."""
    n = 1 << 16
    rng = rng_for(11)
    a = csr(1, 1, [n], np.zeros(n), np.ones(n, np.uint32))
    return a, csr(1, n, [n], rng.permutation(n), rng.integers(1, 9, n).astype(np.uint32))


# -------------------------------------------------------------------- chains
def chain_operands(dtype):
    """a (70 x 50), b (50 x 60), c (60 x 40), d (70 x 60, row 5 of 2500
    unsorted entries: past the one-wave cap of add/sub), d2 (70 x 50) and
    three dense columns of length 60; unsorted rows, small values so that
    the integer chain stays readable (the float one rounds all the same)."""
    rng = rng_for(12, DTYPES.index(dtype))

    def operand(rows, cols, mean, long_row=None):
        lens = rng.integers(0, 2 * mean, rows)
        lens[[0, rows - 1]] = 0
        if long_row is not None:
            lens[long_row] = 2500
        n = int(lens.sum())
        v = rng.uniform(-2, 2, n).astype(dtype) if np.dtype(dtype).kind == "f" else \
            rng.integers(-9, 10, n).astype(dtype)
        return csr(rows, cols, lens, rng.integers(0, cols, n), v)

    ops = {"a": operand(70, 50, 5), "b": operand(50, 60, 5), "c": operand(60, 40, 5),
           "d": operand(70, 60, 5, long_row=5), "d2": operand(70, 50, 5)}
    ops["x"] = [rng.integers(-3, 4, 60).astype(dtype) for _ in range(3)]
    return ops


# ----------------------------------------------------------------- the table
@dataclass(frozen=True)
class Case:
    family: str
    make: Callable
    expect: dict = field(default_factory=dict)  # counts this case must hit exactly
    kept_at: tuple = ()        # candidate positions that must be kept ...
    dropped_at: tuple = ()     # ... and dropped
    more_total_than_cand: bool = False
    generates_nan: bool = False


def _table():
    t = {}
    for n in E:
        for dtype in (DTYPES if n in (256, 4096) else [np.float64, np.uint32]):
            d = name_of(dtype)
            t[f"nnz_a={n}-{d}"] = Case("size", functools.partial(size_nnz_a, n, dtype), {"nnz_a": n})
            t[f"total={n}-{d}"] = Case("size", functools.partial(size_total, n, dtype), {"total": n})
            t[f"n_cand={n}-{d}"] = Case("size", functools.partial(size_n_cand, n, dtype), {"n_cand": n},
                                        more_total_than_cand=True)
    for dtype in (np.float64, np.uint32, np.int64):
        d = name_of(dtype)
        t[f"cancel_straddle-{d}"] = Case(
            "size", functools.partial(cancel_straddle, dtype),
            {"nnz_a": 41 * 32, "total": 41 * 256, "n_cand": 41 * 128, "nnz": 41 * 65},
            kept_at=(0, 255, 256, 4095, 4096), dropped_at=(2, 254, 258, 4094, 4098))
        t[f"cancel_all-{d}"] = Case("empty", functools.partial(cancel_all, dtype),
                                    {"nnz_a": 96, "total": 768, "n_cand": 384, "nnz": 0})
    for dtype in (np.float64, np.int32):
        d = name_of(dtype)
        t[f"empty_a-{d}"] = Case("empty", functools.partial(empty_a, dtype),
                                 {"nnz_a": 0, "total": 0, "n_cand": 0, "nnz": 0})
        t[f"empty_b-{d}"] = Case("empty", functools.partial(empty_b, dtype),
                                 {"nnz_a": 30, "total": 0, "n_cand": 0, "nnz": 0})
        for how in ("past", "empty_rows", "mixed"):
            t[f"total_zero_{how}-{d}"] = Case("empty", functools.partial(total_zero, dtype, how),
                                              {"nnz_a": 300, "total": 0, "n_cand": 0, "nnz": 0})
        t[f"offsets-{d}"] = Case("offsets", functools.partial(offsets, dtype))
        t[f"long_candidate-{d}"] = Case("offsets", functools.partial(long_candidate, dtype), {"nnz_a": 3005})
    for i, r in enumerate(KEY_ROWS):
        for j, c in enumerate(KEY_COLS):
            dtype = DTYPES[(i + j) % len(DTYPES)]
            t[f"key-{r}x{c}-{name_of(dtype)}"] = Case("key", functools.partial(key_width, r, c, dtype))
    for which, dtype in (("wide46", np.float64), ("wide34", np.uint32)):
        t[f"{which}-{name_of(dtype)}"] = Case("wide", functools.partial(wide, which, dtype))
    for dtype in (np.float64, np.float32):
        t[f"values-{name_of(dtype)}"] = Case("values", functools.partial(float_values, dtype), generates_nan=True)
    for dtype in (np.int32, np.uint32, np.int64, np.uint64):
        t[f"values-{name_of(dtype)}"] = Case("values", functools.partial(int_values, dtype))
    t["refusal"] = Case("refusal", refusal, {"nnz_a": 1 << 16, "total": 1 << 32})
    return t


CASES = _table()


def names(*families):
    return [n for n, c in CASES.items() if c.family in families]


@functools.lru_cache(maxsize=None)
def operands(name):
    """The case's (a, b), built once and handed out read-only."""
    a, b = CASES[name].make()
    for arr in (*a[2:], *b[2:]):
        arr.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def pairs_reference(name):
    ref = mul_sparse_pairs(*operands(name))
    for arr in ref:
        arr.setflags(write=False)
    return ref


def oracle_can(a, b):
    return a[0] * b[1] <= ORACLE_PAIRS_MAX
