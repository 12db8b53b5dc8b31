"""Operands that put add_sparse / sub_sparse (csrc/kernels_sparse.hip) on every
branch of the long-row pipeline, and the child process that runs them under
ONE setting of the once-per-process switches BSM_SS_SPLIT and BSM_SS_PRESPLIT.

tests/test_gpu_sparse_addsub_paths.py imports the builders for its in-process
tests and starts this file as a fresh child per setting. Not a test module.

argv: out_json case [case ...]. Each case is built, run through add and sub in
both operand orders, and compared bit for bit with the oracle's two-pointer
merge in the child; one record per case goes to out_json (name, ok, which of
the four calls differed first and at which index). Around each case the child
prints a BEGIN and an END line, so that the parent can tell which of the
library's BSM_SS_DEBUG lines ("long rows / chunks / pieces") belong to it.

case names (dt: f64 f32 i32 u32 i64):
  long:<pattern>:<dt>     one 30,000-entry row per side, columns as in
                          test_add_sub_long_rows_vs_oracle (LONG_PATTERNS)
  caps:<dt>:<order>       top-level pieces whose side lengths sit on the
                          staging cap (split_cap<T>()), on LR_CHUNK, on LEAF;
                          order: unsorted | sorted (the median cut)
  nest:<variant>:<dt>     ~72 nested descending segments per side: the work
                          stack of piece_split fills up; variant: both | lack
                          (the rhs side has no segment maxima: one-sided cuts)
  budget:<dt>             equal descending rows: the scan budget runs out
  many:<dt>               600 rows, 400 of them long, of every kind
  pre:<dt>                pieces of 512 / 513 entries (PRE_MIN) and one nested
                          piece that takes all PRE_CUTS cuts of the first pass
  diag:<kind>:<dt>        the smallest long-row operands (the diagnostic
                          levels); kind: row65 (one row of LONG_ROW + 1
                          entries) | cap1 (split_cap<T>() + 1 per side)
"""

import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# the constants of csrc/addsub_plan.hpp (the first three) and csrc/kernels_sparse.hip
WROW_CAP = 2048
LONG_ROW = 64
LR_CHUNK = 2048
LEAF = 64
PRE_MIN = 512
PRE_CUTS = 7

DTYPES = {"f64": np.float64, "f32": np.float32, "i32": np.int32, "u32": np.uint32, "i64": np.int64}

LONG_PATTERNS = ["both_have_max", "rhs_lacks_max", "unequal_max_counts", "one_side_empty", "sorted_long",
                 "sorted_duplicates", "one_sorted", "all_equal", "descending_equal", "descending", "three_columns",
                 "wide_columns"]


def split_cap(dtype):
    """split_cap<T>(): entries per side that piece_split stages in LDS."""
    return 4096 if np.dtype(dtype).itemsize <= 4 else 2048


def make_values(rng, col, dtype, side):
    """Values for the entries at columns `col` of operand `side` (0: a, 1: b).

    Floats come from uniform(-3, 3): no sum of two is exact, so a + b, b + a
    taken in the wrong order, a - b against -(b - a), or a pair summed with
    the wrong partner differ in bits. 4-byte integers lie next to the type's
    limits, so sums wrap. In about one column of twenty the value is a
    function of the column alone, a's f(c) against b's -f(c) (even columns:
    cancels under add) or f(c) (odd columns: cancels under sub), so that
    whichever two entries of such a column meet, the pair is dropped."""
    dt = np.dtype(dtype)
    col = np.asarray(col, np.int64)
    n = len(col)
    if dt.kind == "f":
        v = rng.uniform(-3, 3, n).astype(dt)
        f = ((col % 97) * 0.37 + 0.1).astype(dt)
    elif dt.itemsize == 4:
        info = np.iinfo(dt)
        near = rng.integers(1, 5, n)
        v = np.where(rng.random(n) < 0.5, info.max - near, info.min + near).astype(dt)
        f = (info.max - (col % 5)).astype(dt)
    else:
        v = rng.integers(-3, 4, n).astype(dt)
        v[v == 0] = 1 + side
        f = (col % 5 + 1).astype(dt)
    fixed = (col * 7919) % 1000 < 50
    if side == 1:
        f = np.where(col % 2 == 0, np.zeros(1, dt) - f, f).astype(dt)  # wraps for unsigned
    v[fixed] = f[fixed]
    return v


def assemble(rng, rows_a, rows_b, cols, dtype, same=()):
    """(dims, (row_ptr, col, v) of a, the same of b) from per-row column
    arrays; in the rows listed in `same`, b's values repeat a's (a - a)."""
    out = []
    for side, rows in enumerate((rows_a, rows_b)):
        lens = [len(r) for r in rows]
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        ci = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)])
        assert ci.size == 0 or (0 <= ci.min() and ci.max() < cols)
        v = make_values(rng, ci, dtype, side)
        out.append([rp, ci.astype(np.uint64), v])
    for r in same:
        assert np.array_equal(rows_a[r], rows_b[r])
        a0, b0 = int(out[0][0][r]), int(out[1][0][r])
        out[1][2][b0:b0 + len(rows_b[r])] = out[0][2][a0:a0 + len(rows_a[r])]
    return (len(rows_a), cols), tuple(out[0]), tuple(out[1])


# ------------------------------------------------------------ section 2 ----
def long_row_columns(pattern, rng, n=30_000, cols=500):
    """The twelve column patterns of test_add_sub_long_rows_vs_oracle."""
    ca = rng.integers(0, cols, n)
    cb = rng.integers(0, cols, n)
    if pattern == "rhs_lacks_max":
        cb = np.minimum(cb, cols - 2)
    if pattern == "unequal_max_counts":
        ca[rng.random(n) < 0.05] = cols - 1
    if pattern == "sorted_long":
        ca, cb = np.sort(ca), np.sort(cb)
    if pattern == "sorted_duplicates":
        ca, cb = np.sort(ca // 50), np.sort(cb[: n // 3] // 50)
    if pattern == "one_sorted":
        ca = np.sort(ca)
    if pattern == "all_equal":
        ca, cb = np.full(n, 7), np.full(n // 2, 7)
    if pattern == "descending_equal":
        ca = np.sort(ca)[::-1].copy()
        cb = ca.copy()
    if pattern == "descending":
        ca, cb = np.sort(ca)[::-1].copy(), np.sort(cb)[::-1].copy()
    if pattern == "three_columns":
        ca, cb = ca % 3, cb % 3
    if pattern == "wide_columns":
        cols = 1 << 30
        ca, cb = rng.integers(0, cols, n), rng.integers(0, cols, n)
    if pattern == "one_side_empty":
        cb = cb[:0]
    return ca, cb, cols


def two_rows(rng, ca, cb, cols, dtype):
    """A short first row (5 and 3 entries) and the long row, as the int64 test has them."""
    ka, kb = min(5, len(ca)), min(3, len(cb))
    return assemble(rng, [ca[:ka], ca[ka:]], [cb[:kb], cb[kb:]], cols, dtype)


def build_long(pattern, dtype):
    rng = np.random.default_rng(len(pattern))
    ca, cb, cols = long_row_columns(pattern, rng)
    return two_rows(rng, ca, cb, cols, dtype)


# ------------------------------------------------------------ section 3 ----
def below(rng, n, m, srt):
    c = rng.integers(0, m, n)
    return np.sort(c) if srt else c


def row_of_pieces(rng, pieces, m, srt):
    """Both sides of a row whose top-level pieces (cut at the pairs of the row
    maximum m) have exactly the given (la, lb) side lengths: every piece but
    the last is closed by a pair of m, the last is the row's tail."""
    a, b = [], []
    for k, (la, lb) in enumerate(pieces):
        a.append(below(rng, la, m, srt))
        b.append(below(rng, lb, m, srt))
        if k + 1 < len(pieces):
            a.append([m])
            b.append([m])
    return np.concatenate(a).astype(np.int64), np.concatenate(b).astype(np.int64)


def side_with_m(rng, n, mpos, m, srt):
    """n entries below m with m itself at the positions mpos; srt: every
    stretch between two m is sorted."""
    c = rng.integers(0, m, n)
    cuts = sorted(mpos)
    if srt:
        lo = 0
        for p in cuts + [n]:
            c[lo:p] = np.sort(c[lo:p])
            lo = p + 1
    c[cuts] = m
    return c.astype(np.int64)


def caps_rows(rng, cap, m, srt):
    """Rows of section 3 for one staging cap."""
    s = 700
    ra, rb = [], []

    def add(pair):
        ra.append(pair[0])
        rb.append(pair[1])

    # a first piece with its closing pair and the tail piece without one, each
    # with cap - 2 .. cap + 1 entries on self, on rhs, on both sides. With the
    # pair a side of cap - 1 is the longest that is staged (the pair fills the
    # last LDS slot); without it, a side of cap.
    for d in (-2, -1, 0, 1):
        add(row_of_pieces(rng, [(cap + d, s), (cap + d, s)], m, srt))
        add(row_of_pieces(rng, [(s, cap + d), (s, cap + d)], m, srt))
        add(row_of_pieces(rng, [(cap + d, cap + d), (cap + d, cap + d)], m, srt))
    add(row_of_pieces(rng, [(cap - 1, cap), (cap, cap)], m, srt))
    add(row_of_pieces(rng, [(cap, cap - 1), (cap, cap + 1)], m, srt))
    ra.append(np.zeros(0, np.int64))  # an empty row between long rows
    rb.append(np.zeros(0, np.int64))
    # small pieces: 64 entries are a leaf at once, 65 take one cut; sides of
    # 64, 65 and 4096 (the ranges of lower_bound_wave when sorted)
    add(row_of_pieces(rng, [(32, 32), (32, 33), (64, 1), (1, 64), (0, 65), (65, 0), (64, 0), (64, 65), (65, 64),
                            (4096, 100), (100, 4096), (4096, 4096), (64, 64), (33, 32)], m, srt))
    # row sides of LR_CHUNK - 1, LR_CHUNK, LR_CHUNK + 1 and 2 LR_CHUNK + 1
    # entries, m in more than one chunk of a side, 3 against 5 occurrences
    # (twice) and 0 against 4 (only one side holds m: one piece, no pair)
    c = LR_CHUNK
    ra.append(side_with_m(rng, c - 1, [5, 1000, c - 2], m, srt))
    rb.append(side_with_m(rng, 2 * c + 1, [0, c - 1, c, 4000, 2 * c], m, srt))
    ra.append(side_with_m(rng, c + 1, [], m, srt))
    rb.append(side_with_m(rng, c, [1, 100, c - 2, c - 1], m, srt))
    ra.append(side_with_m(rng, 2 * c + 1, [c - 1, c, 2 * c], m, srt))
    rb.append(side_with_m(rng, c, [0, 1024, 1025, 1026, c - 1], m, srt))
    ra.append(side_with_m(rng, c, [0, c - 1, 77, 78], m, srt))  # 4 against 0, the other way round
    rb.append(side_with_m(rng, c - 1, [], m, srt))
    ra.append(below(rng, 7, m, srt))  # a short last row
    rb.append(below(rng, 9, m, srt))
    return ra, rb


def build_caps(dtype, order):
    rng = np.random.default_rng(31 + np.dtype(dtype).itemsize + (order == "sorted"))
    m = 900
    ra, rb = caps_rows(rng, split_cap(dtype), m, order == "sorted")
    return assemble(rng, ra, rb, m + 1, dtype)


# ------------------------------------------------------------ section 4 ----
def nest_side(rng, lens, width, with_top):
    """Segments i = 0, 1, ...: segment i lies in the band [i * width,
    (i + 1) * width), descends inside, and (with_top) starts with the band's
    largest column, which occurs nowhere else. No stretch of two or more
    segments is sorted, and the largest column of a prefix of segments is the
    first entry of its last segment."""
    out = []
    for i, n in enumerate(lens):
        top = (i + 1) * width - 1
        if with_top:
            seg = np.concatenate([[top], np.sort(rng.integers(i * width, top, n - 1))[::-1]])
        else:
            seg = np.sort(rng.integers(i * width, top, n))[::-1]
        out.append(seg)
    return np.concatenate(out).astype(np.int64)


def nest_columns(rng, total, nseg, min_len, lack):
    """Segment lengths grow by 1 / 0.9 (at least min_len): every cut at the
    maximum peels the last segment, about a tenth of the piece, so the cuts'
    scans sum to about ten passes over the piece, inside the budget of 32,
    and every cut leaves one more entry on the stack."""
    w = (1 / 0.9) ** np.arange(nseg)
    lens = np.maximum(min_len, np.round(w * total / w.sum())).astype(np.int64)
    width = 1 << 13
    assert lens.max() < width
    ca = nest_side(rng, lens, width, True)
    cb = nest_side(rng, lens, width, not lack)
    return ca, cb, nseg * width


def build_nest(variant, dtype):
    rng = np.random.default_rng(41)
    ca, cb, cols = nest_columns(rng, 30_000, 72, 12, variant == "lack")
    return two_rows(rng, ca, cb, cols, dtype)


def build_budget(dtype):
    rng = np.random.default_rng(43)
    ca = np.sort(rng.integers(0, 500, 30_000))[::-1].copy()
    # the same short first row on both sides: the long rows start at the same entry and stay equal
    return assemble(rng, [ca[:5], ca[5:]], [ca[:5], ca[5:]], 500, dtype)


# ------------------------------------------------------------ section 5 ----
def build_many(dtype):
    """600 rows, 400 of them long (a second block of every grid_of launch):
    long rows first and last, runs of adjacent long rows, long rows between
    empty and short rows, rows long by one side alone, rows of exactly 65
    entries, three rows of several chunks, and long rows a - a that leave no
    output between non-empty neighbours."""
    rng = np.random.default_rng(53)
    rows, cols = 600, 300
    ra, rb, same = [], [], []
    exact65 = [(65, 0), (0, 65), (32, 33), (64, 1)]
    big = {100: (5000, 4500), 300: (3000, 0), 500: (2500, 6200)}

    def both(la, lb):
        ra.append(rng.integers(0, cols, la))
        rb.append(rng.integers(0, cols, lb))

    for r in range(rows):
        k = r % 12
        if r in big:
            both(*big[r])
        elif r == 0:
            both(100, 80)
        elif r == rows - 1:
            both(70, 90)
        elif k in (0, 1, 2, 10):
            both(int(rng.integers(40, 150)), int(rng.integers(40, 150)))
        elif k == 3:
            both(0, 0)
        elif k == 4:
            both(0, int(rng.integers(65, 200)))
        elif k == 6:
            both(int(rng.integers(65, 200)), 0)
        elif k == 7:
            both(*exact65[(r // 12) % 4])
        elif k == 8:
            c = rng.integers(0, cols, int(rng.integers(80, 150)))
            ra.append(c)
            rb.append(c.copy())
            same.append(r)
        elif k in (5, 9):
            both(int(rng.integers(1, 30)), int(rng.integers(1, 30)))
        else:
            both(1, 0)
    n_long = sum(len(x) + len(y) > LONG_ROW for x, y in zip(ra, rb))
    assert n_long > 256 and sum(map(len, ra)) < 200_000 and sum(map(len, rb)) < 200_000
    return assemble(rng, ra, rb, cols, dtype, same)


# ------------------------------------------------------------ section 6 ----
def build_pre(dtype):
    """For the two-pass form: top-level pieces of PRE_MIN and PRE_MIN + 1
    entries (the first pass leaves the one whole and cuts the other), and a
    nested piece of ~8,000 entries per side whose largest part stays above
    PRE_MIN for all PRE_CUTS cuts, so it goes out as PRE_CUTS + 1 pieces."""
    rng = np.random.default_rng(61)
    width = 1 << 13
    na, nb, cols = nest_columns(rng, 8_000, 20, 40, False)
    pa, pb = row_of_pieces(rng, [(256, 256), (256, 257), (511, 1), (1, 512), (300, 213), (PRE_MIN, PRE_MIN),
                                 (200, 100)], 400, False)
    short = rng.integers(0, width, 5)
    return assemble(rng, [pa, short, na], [pb, short[:2], nb], cols, dtype)


# ------------------------------------------------------------ section 8 ----
def build_diag(kind, dtype):
    """The smallest long-row operands, for the diagnostic levels: row65, one
    long row of LONG_ROW + 1 entries (33 and 32) between two short rows;
    cap1, one row of split_cap<T>() + 1 entries on each side."""
    rng = np.random.default_rng(67)
    la, lb = (33, 32) if kind == "row65" else (split_cap(dtype) + 1,) * 2
    cols = 40 if kind == "row65" else 900
    ra = [rng.integers(0, cols, n) for n in (5, la, 7)]
    rb = [rng.integers(0, cols, n) for n in (3, lb, 0)]
    return assemble(rng, ra, rb, cols, dtype)


def build(name):
    p = name.split(":")
    if p[0] == "diag":
        return build_diag(p[1], DTYPES[p[2]])
    if p[0] == "long":
        return build_long(p[1], DTYPES[p[2]])
    if p[0] == "caps":
        return build_caps(DTYPES[p[1]], p[2])
    if p[0] == "nest":
        return build_nest(p[1], DTYPES[p[2]])
    if p[0] == "budget":
        return build_budget(DTYPES[p[1]])
    if p[0] == "many":
        return build_many(DTYPES[p[1]])
    if p[0] == "pre":
        return build_pre(DTYPES[p[1]])
    raise ValueError("unknown case " + name)


# the cases every child runs: sections 2 (one 8-byte, one 4-byte type), 3, 4, 5 and the two-pass extras
CHILD_CASES = ([f"long:{p}:{dt}" for dt in ("f64", "i32") for p in LONG_PATTERNS]
               + [f"caps:{dt}:{o}" for dt in ("f64", "f32") for o in ("unsorted", "sorted")]
               + [f"nest:{v}:{dt}" for v in ("both", "lack") for dt in ("f64", "u32")]
               + ["budget:f64", "budget:f32", "many:f64", "many:u32", "pre:f64", "pre:u32"])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def first_difference(got, rp, ci, v):
    """None when the result equals the oracle's bit for bit, else (what, index)."""
    for what, g, w in (("row_ptr", np.asarray(got.row_index, np.uint64), np.asarray(rp, np.uint64)),
                       ("col", np.asarray(got.col_index, np.uint64), np.asarray(ci, np.uint64)),
                       ("v", bits(np.asarray(got.v)), bits(np.asarray(v, dtype=got.dtype)))):
        if g.shape != w.shape:
            return what + " length", int(min(g.size, w.size))
        ne = np.flatnonzero(g != w)
        if ne.size:
            return what, int(ne[0])
    return None


def run_case(name, orc):
    from basic_sparse_matrix_amd import Csr

    dims, sa, sb = build(name)
    a, b = Csr.from_csr_arrays(dims, *sa), Csr.from_csr_arrays(dims, *sb)
    xa, xb = (dims[0], dims[1]) + sa, (dims[0], dims[1]) + sb
    for call, op, ref, (x, y), (ox, oy) in (("a+b", Csr.add_sparse, orc.add_sparse, (a, b), (xa, xb)),
                                            ("b+a", Csr.add_sparse, orc.add_sparse, (b, a), (xb, xa)),
                                            ("a-b", Csr.sub_sparse, orc.sub_sparse, (a, b), (xa, xb)),
                                            ("b-a", Csr.sub_sparse, orc.sub_sparse, (b, a), (xb, xa))):
        d = first_difference(op(x, y), *ref(ox, oy))
        if d is not None:
            return dict(ok=False, call=call, what=d[0], first_mismatch=d[1])
    return dict(ok=True, call=None, what=None, first_mismatch=None)


def main():
    out_json, cases = sys.argv[1], sys.argv[2:]
    from oracle import pyoracle as orc

    from basic_sparse_matrix_amd import _lib

    _lib.require_device()
    env = {k: v for k, v in os.environ.items() if k.startswith("BSM_")}
    records = []
    for name in cases:
        t0 = time.perf_counter()
        print("BEGIN " + name, flush=True)
        try:
            rec = run_case(name, orc)
        except Exception as ex:
            rec = dict(ok=False, call=None, what=f"{type(ex).__name__}: {ex}", first_mismatch=None)
        rec.update(case=name, env=env, seconds=round(time.perf_counter() - t0, 3))
        records.append(rec)
        print(f"END {name} {'ok' if rec['ok'] else 'FAIL'} {rec['seconds']} s", flush=True)
        with open(out_json, "w") as f:  # rewritten per case: what ran is on record if a later case dies
            json.dump(records, f)


if __name__ == "__main__":
    main()
