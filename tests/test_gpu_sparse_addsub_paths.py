"""add_sparse / sub_sparse on every path of csrc/kernels_sparse.hip, bit for
bit against the oracle's two-pointer merge (sparse.rs:484-599): the wave path
with its LDS full, the thread path against one piece, and the long-row
pipeline (chunks, the cut at the pairs of the row maximum, piece_split's
staging caps, work stack, leaf list, scan budget, median cut and one-sided
copy) at every scalar width; the older piece_merge (BSM_SS_SPLIT=0) and the
two-pass form (BSM_SS_PRESPLIT=1), which are read once per process, in child
processes (tests/sparse_addsub_worker.py, which also builds the operands);
and the diagnostic levels 2, 3 and 4 of BSM_SS_DEBUG, which hand the kernels
their stamp buffers or end every phase with a synchronise.

Every comparison is add and sub in both operand orders. Where a test means a
path it also reads the library's BSM_SS_DEBUG line ("long rows, chunks,
pieces"), so a case meant for the pipeline cannot pass through the wave path
and a case meant for the wave path cannot pass through the pipeline.

A child that ends by a signal or runs out of time stops the child tests:
every remaining case fails at once and no further child is started.
"""

import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sparse_addsub_worker as W
from basic_sparse_matrix_amd import Csr
from test_gpu_sparse_ops import arrays
from test_gpu_spmm import assert_csr_bits

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "sparse_addsub_worker.py")
SWITCHES = ("BSM_SS_SPLIT", "BSM_SS_PRESPLIT", "BSM_SS_WAVE", "BSM_SS_DEBUG")
DEBUG_LINE = re.compile(r"\[bsm ss debug\] long rows (\d+), chunks (\d+), pieces (\d+)")


def n_long_rows(sa, sb):
    la, lb = np.diff(sa[0].astype(np.int64)), np.diff(sb[0].astype(np.int64))
    return int(np.count_nonzero(la + lb > W.LONG_ROW))


def check(orc, capfd, monkeypatch, case, pipeline=True, cmp=assert_csr_bits, debug="1"):
    """add and sub in both orders against the oracle; pipeline: every call
    took the general path and cut exactly the rows above LONG_ROW into
    pieces; else: no call did (the wave path). Returns the four calls'
    piece counts and what the library wrote to stderr."""
    dims, sa, sb = case
    a, b = Csr.from_csr_arrays(dims, *sa), Csr.from_csr_arrays(dims, *sb)
    monkeypatch.setenv("BSM_SS_DEBUG", debug)
    capfd.readouterr()
    for op, ref in [(Csr.add_sparse, orc.add_sparse), (Csr.sub_sparse, orc.sub_sparse)]:
        cmp(op(a, b), *ref(arrays(a), arrays(b)))
        cmp(op(b, a), *ref(arrays(b), arrays(a)))
    err = capfd.readouterr().err
    lines = DEBUG_LINE.findall(err)
    if pipeline:
        assert len(lines) == 4, lines
        for n_long, n_chunks, n_pieces in lines:
            assert int(n_long) == n_long_rows(sa, sb) and int(n_pieces) >= int(n_long) > 0, lines
    else:
        assert lines == []
    return [int(n_pieces) for _, _, n_pieces in lines], err


# ---- 1. dispatch boundaries -------------------------------------------------
EDGE_DTYPES = [np.float64, np.float32, np.uint32, np.int64]


def edge_matrix(rng, shapes, cols, dtype, fill_a, fill_b):
    """The rows `shapes` (la, lb), two short filler rows after each."""
    ra, rb = [], []
    for la, lb in shapes:
        for fa, fb in [(la, lb), (int(rng.integers(0, fill_a + 1)), int(rng.integers(0, fill_b + 1))),
                       (int(rng.integers(0, fill_a + 1)), 0)]:
            ra.append(rng.integers(0, cols, fa))
            rb.append(rng.integers(0, cols, fb))
    return W.assemble(rng, ra, rb, cols, dtype)


def wave_splits(t):
    return [(t, 0), (0, t), (t // 2, t - t // 2), (1, t - 1)]


def longest(spec):
    return int(np.diff(spec[0].astype(np.int64)).max())


@gpu
@pytest.mark.parametrize("dtype", EDGE_DTYPES)
def test_general_path_rows_around_wave_cap(orc, capfd, monkeypatch, dtype):
    """Rows of 2047, 2048 and 2049 entries on the two sides together, split
    (all, 0), (0, all), halves and (1, rest), unsorted with repeats, in one
    matrix of 36 rows: the 2049 rows put the whole call on the general path."""
    rng = np.random.default_rng(101)
    shapes = [s for t in (2047, 2048, 2049) for s in wave_splits(t)]
    case = edge_matrix(rng, shapes, 300, dtype, 40, 40)
    assert longest(case[1]) + longest(case[2]) > W.WROW_CAP
    check(orc, capfd, monkeypatch, case)


@gpu
@pytest.mark.parametrize("split", range(4))
@pytest.mark.parametrize("dtype", EDGE_DTYPES)
def test_wave_path_with_lds_full(orc, capfd, monkeypatch, dtype, split):
    """The longest row holds exactly WROW_CAP = 2048 entries on its two sides
    together (the operands' longest rows add up to the cap: the wave path,
    sc[] / sv[] filled to the last slot), beside a row of 2047."""
    rng = np.random.default_rng(102 + split)
    shapes = [wave_splits(2048)[split], wave_splits(2047)[split]]
    la, lb = shapes[0]
    case = edge_matrix(rng, shapes, 300, dtype, min(40, la), min(40, lb))
    assert longest(case[1]) + longest(case[2]) == W.WROW_CAP
    check(orc, capfd, monkeypatch, case, pipeline=False)


@gpu
@pytest.mark.parametrize("dtype", EDGE_DTYPES)
def test_thread_path_rows_around_long_row(orc, capfd, monkeypatch, dtype):
    """BSM_SS_WAVE=0: rows of 63 and 64 entries are merged by one thread
    (addsub_count / addsub_fill), rows of 65 are one piece each."""
    monkeypatch.setenv("BSM_SS_WAVE", "0")
    rng = np.random.default_rng(103)
    shapes = [s for t in (63, 64, 65) for s in [(t, 0), (0, t), (t // 2, t - t // 2), (t - 1, 1)]]
    case = edge_matrix(rng, shapes, 40, dtype, 20, 20)
    assert n_long_rows(case[1], case[2]) == 4
    check(orc, capfd, monkeypatch, case)


# ---- 2. the structured long rows at every width ------------------------------
@gpu
@pytest.mark.parametrize("pattern", W.LONG_PATTERNS)
@pytest.mark.parametrize("dt", ["f64", "f32", "i32"])
def test_long_rows_every_width(orc, capfd, monkeypatch, dt, pattern):
    """The twelve column patterns of test_add_sub_long_rows_vs_oracle with
    8-byte and 4-byte floats (inexact sums, about 5 % cancelling pairs) and
    int32 next to its limits (sums wrap): split_cap<T>() is 2048 or 4096."""
    check(orc, capfd, monkeypatch, W.build(f"long:{pattern}:{dt}"))


# ---- 3. pieces on the staging caps -------------------------------------------
@gpu
@pytest.mark.parametrize("order", ["unsorted", "sorted"])
@pytest.mark.parametrize("dt", ["f64", "i64", "f32", "u32"])
def test_pieces_on_the_caps(orc, capfd, monkeypatch, dt, order):
    """First pieces (closing pair) and tail pieces (none) with split_cap - 2
    .. split_cap + 1 entries on one side and on both, row sides of LR_CHUNK
    - 1 .. 2 LR_CHUNK + 1 with the maximum in several chunks (3 against 5 and
    0 against 4 occurrences), pieces of 64 and 65 entries; sorted: the median
    cut, lower_bound_wave over 64, 65 and 4096 entries."""
    check(orc, capfd, monkeypatch, W.build(f"caps:{dt}:{order}"))


# ---- 4. the work stack and the scan budget -----------------------------------
LEAF = W.LEAF
STACK = 64


KEYS = ["full_stack_push", "full_stack_entries", "max_depth", "leaf", "budget_leaf", "one_sided_copy", "median_cut",
        "pair_cut", "self_only_cut", "rhs_only_cut", "pieces", "staged", "staged_to_last_slot", "cut_from_global"]


def model_cut(ca, cb, x, st):
    """cut_piece: the two parts of sub-piece x in the order they are pushed."""
    a0, a1, b0, b1, p = x
    na, nb = a1 - a0, b1 - b0
    sa, sb = ca[a0:a1], cb[b0:b1]
    if np.all(sa[:-1] <= sa[1:]) and np.all(sb[:-1] <= sb[1:]):  # both sides sorted: by value at the median
        v = int(sa[na // 2]) if na >= nb else int(sb[nb // 2])
        qa, qb = a0 + int(np.searchsorted(sa, v)), b0 + int(np.searchsorted(sb, v))
        if qa == a0 and qb == b0 and v < 0x7FFFFFFF:
            qa, qb = a0 + int(np.searchsorted(sa, v + 1)), b0 + int(np.searchsorted(sb, v + 1))
        if not (qa == a0 and qb == b0) and not (qa == a1 and qb == b1):
            st["median_cut"] += 1
            return (qa, a1, qb, b1, p), (a0, qa, b0, qb, False)
    mx = max(int(sa.max()), int(sb.max()))
    ha, hb = np.flatnonzero(sa == mx), np.flatnonzero(sb == mx)
    if ha.size and hb.size:
        st["pair_cut"] += 1
        return (a0 + int(ha[0]) + 1, a1, b0 + int(hb[0]) + 1, b1, p), (a0, a0 + int(ha[0]), b0, b0 + int(hb[0]), True)
    if ha.size:
        st["self_only_cut"] += 1
        return (a0 + int(ha[0]), a1, b1, b1, p), (a0, a0 + int(ha[0]), b0, b1, False)
    st["rhs_only_cut"] += 1
    return (a1, a1, b0 + int(hb[0]), b1, p), (a0, a1, b0, b0 + int(hb[0]), False)


def model_piece(ca, cb, pair, st, cap):
    """piece_split's cut recursion on one top-level piece, by its columns
    alone: the stack depth, the scan budget, what is staged in LDS (cap
    entries per side) and the branch of every cut. It says which branches an
    input reaches; it computes no values."""
    stack = [(0, len(ca), 0, len(cb), pair)]
    budget = 32 * (len(ca) + len(cb)) + 4096
    staged, sp_base = False, 0

    def push(x):
        if len(stack) == STACK:  # demoted to a serial leaf
            st["full_stack_push"] += 1
            st["full_stack_entries"] = max(st["full_stack_entries"], (x[1] - x[0]) + (x[3] - x[2]))
            return
        stack.append(x)
        st["max_depth"] = max(st["max_depth"], len(stack))

    while stack:
        if staged and len(stack) == sp_base:
            staged = False
        x = stack.pop()
        a0, a1, b0, b1, p = x
        na, nb = a1 - a0, b1 - b0
        if (not staged and na > 0 and nb > 0 and na + nb > LEAF and budget >= 0 and na + p <= cap
                and nb + p <= cap):
            staged, sp_base = True, len(stack)
            st["staged"] += 1
            st["staged_to_last_slot"] += na + p == cap or nb + p == cap
        if na + nb <= LEAF or na == 0 or nb == 0 or budget < 0:
            if na + nb == 0 and not p:
                continue
            if na > 0 and nb > 0:
                st["leaf"] += 1
                st["budget_leaf"] += na + nb > LEAF  # budget < 0 reached with a piece still worth cutting
            else:
                st["one_sided_copy"] += 1
            continue
        budget -= na + nb
        st["cut_from_global"] += not staged
        for part in model_cut(ca, cb, x, st):
            push(part)


def model_presplit(ca, cb, pair, st):
    """The cuts-only first pass of BSM_SS_PRESPLIT=1 on one top-level piece: the number of pieces it emits."""
    stack = [(0, len(ca), 0, len(cb), pair)]
    for _ in range(W.PRE_CUTS):
        sizes = [(x[1] - x[0]) + (x[3] - x[2]) for x in stack]
        big = sizes.index(max(sizes))
        x = stack[big]
        if sizes[big] <= W.PRE_MIN or x[1] == x[0] or x[3] == x[2]:
            break
        stack[big] = stack[-1]
        stack.pop()
        stack.extend(model_cut(ca, cb, x, st))
    return len(stack)


def top_pieces(ca, cb):
    """The top-level cut of a long row at the pairs of its maximum: (self stretch, rhs stretch, closing pair)."""
    m = max(int(ca.max()) if len(ca) else -1, int(cb.max()) if len(cb) else -1)
    ia, ib = np.flatnonzero(ca == m), np.flatnonzero(cb == m)
    pa = pb = 0
    for k in range(min(len(ia), len(ib))):
        yield ca[pa:ia[k]], cb[pb:ib[k]], True
        pa, pb = int(ia[k]) + 1, int(ib[k]) + 1
    yield ca[pa:], cb[pb:], False


def model_row(ca, cb, cap=2048, st=None):
    st = dict.fromkeys(KEYS, 0) if st is None else st
    for xa, xb, pair in top_pieces(ca, cb):
        model_piece(xa, xb, pair, st, cap)
        st["pieces"] += 1
    return st


def rows_of(case):
    _, sa, sb = case
    ra, rb = sa[0].astype(np.int64), sb[0].astype(np.int64)
    for r in range(len(ra) - 1):
        yield sa[1][ra[r]:ra[r + 1]].astype(np.int64), sb[1][rb[r]:rb[r + 1]].astype(np.int64)


def model_matrix(case, cap):
    """The model on every long row of a case."""
    st = dict.fromkeys(KEYS, 0)
    for ca, cb in rows_of(case):
        if len(ca) + len(cb) > W.LONG_ROW:
            model_row(ca, cb, cap, st)
    return st


def model_case(case):
    """The model on the long second row of a two-row case."""
    _, sa, sb = case
    a1, b1 = int(sa[0][1]), int(sb[0][1])
    return model_row(sa[1][a1:].astype(np.int64), sb[1][b1:].astype(np.int64))


def test_cut_model_on_the_stack_and_budget_inputs():
    """No GPU: the nested inputs fill piece_split's 64-entry stack while the
    budget lasts (both cut kinds), the equal descending rows spend the budget."""
    both = model_case(W.build("nest:both:f64"))
    assert both["full_stack_push"] >= 1 and both["full_stack_entries"] > LEAF and both["pair_cut"] >= STACK, both
    lack = model_case(W.build("nest:lack:f64"))
    assert lack["full_stack_push"] >= 1 and lack["full_stack_entries"] > LEAF, lack
    assert lack["self_only_cut"] >= 8 and lack["rhs_only_cut"] >= 8, lack
    spent = model_case(W.build("budget:f64"))
    assert spent["budget_leaf"] >= 1 and spent["full_stack_push"] == 0, spent


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("order", ["unsorted", "sorted"])
def test_cut_model_on_the_cap_inputs(dt, order):
    """No GPU: the rows of section 3 fill the staging area to its last slot
    (with and without a closing pair), leave pieces one entry too long to be
    cut from global memory, and take every kind of cut."""
    st = model_matrix(W.build(f"caps:{dt}:{order}"), W.split_cap(W.DTYPES[dt]))
    # seven top-level pieces end on the last slot (three first pieces with cap - 1 entries and their pair,
    # four tails with cap entries on a side); twelve have a side too long by one or two entries
    assert st["staged_to_last_slot"] >= 7 and st["cut_from_global"] >= 12, st
    assert st["self_only_cut"] >= 1 and st["rhs_only_cut"] >= 1 and st["one_sided_copy"] >= 1, st
    assert (st["median_cut"] >= 100) == (order == "sorted"), st


def test_cut_model_on_the_two_pass_input():
    """No GPU: under BSM_SS_PRESPLIT=1 the first pass leaves a piece of
    PRE_MIN entries whole, cuts one of PRE_MIN + 1, and spends all PRE_CUTS
    cuts on the nested piece (PRE_CUTS + 1 pieces go to the second pass)."""
    rows = list(rows_of(W.build("pre:f64")))
    st = dict.fromkeys(KEYS, 0)
    emitted = {len(xa) + len(xb): model_presplit(xa, xb, pair, st) for xa, xb, pair in top_pieces(*rows[0])}
    assert emitted[W.PRE_MIN] == 1 and emitted[W.PRE_MIN + 1] == 2 and emitted[2 * W.PRE_MIN] >= 2, emitted
    nested = [model_presplit(xa, xb, pair, st) for xa, xb, pair in top_pieces(*rows[2])]
    assert max(nested) == W.PRE_CUTS + 1, nested


@gpu
@pytest.mark.parametrize("dt", ["f64", "u32"])
@pytest.mark.parametrize("variant", ["both", "lack"])
def test_full_work_stack(orc, capfd, monkeypatch, variant, dt):
    """push() with sp == 64: the sub-piece is demoted to a serial leaf."""
    case = W.build(f"nest:{variant}:{dt}")
    st = model_case(case)
    assert st["full_stack_push"] >= 1 and st["full_stack_entries"] > LEAF, st
    check(orc, capfd, monkeypatch, case)


@gpu
@pytest.mark.parametrize("dt", ["f64", "f32", "i64"])
def test_scan_budget_spent(orc, capfd, monkeypatch, dt):
    """Equal descending rows: every cut peels one pair, the budget runs out
    and the rest is merged as it stands."""
    case = W.build(f"budget:{dt}")
    st = model_case(case)
    assert st["budget_leaf"] >= 1, st
    check(orc, capfd, monkeypatch, case)


# ---- 5. many long rows in one call -------------------------------------------
@gpu
@pytest.mark.parametrize("dt", ["f64", "u32"])
def test_many_long_rows(orc, capfd, monkeypatch, dt):
    """400 long rows among 600 (two blocks in every launch over long rows):
    compact_flags, long_extents, the chunk list's per-side offsets, the
    pieces' starts, long_row_totals_slots and pos_copy across rows."""
    case = W.build(f"many:{dt}")
    assert n_long_rows(case[1], case[2]) > 256
    check(orc, capfd, monkeypatch, case)


# ---- 6. the once-per-process switches, in child processes --------------------
ENVS = {"default": {}, "merge": {"BSM_SS_SPLIT": "0"}, "presplit": {"BSM_SS_PRESPLIT": "1"}}
_records = {}   # setting -> {case: record} of the child that ran it
_dead = []      # why no further child may start (a child ended by a signal or timed out)


def _child(env_name, tmp_path_factory, settings=None, cases=W.CHILD_CASES):
    """The records of the one child of setting env_name (started at its first
    use): `cases` under the switches `settings` (ENVS[env_name] and
    BSM_SS_DEBUG=1 when not given)."""
    if env_name in _records:
        return _records[env_name]
    if _dead:
        pytest.fail("not started: " + _dead[0])
    out = tmp_path_factory.mktemp("addsub_" + env_name) / "records.json"
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(dict(ENVS[env_name], BSM_SS_DEBUG="1") if settings is None else settings)
    log = ""
    try:
        r = subprocess.run([sys.executable, "-u", WORKER, str(out)] + cases, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        log = r.stdout.decode(errors="replace")
        if r.returncode < 0 or r.returncode in (134, 139):
            _dead.append(f"the child of setting {env_name} ended with status {r.returncode}: {log[-3000:]}")
    except subprocess.TimeoutExpired as ex:
        log = (ex.stdout or b"").decode(errors="replace")
        _dead.append(f"the child of setting {env_name} ran out of time: {log[-3000:]}")
    recs = {}
    if out.exists():
        recs = {rec["case"]: rec for rec in json.loads(out.read_text())}
    recs["__log__"] = log
    _records[env_name] = recs
    return recs


@gpu
@pytest.mark.parametrize("case", W.CHILD_CASES)
@pytest.mark.parametrize("env_name", list(ENVS))
def test_switch_case(env_name, case, tmp_path_factory):
    recs = _child(env_name, tmp_path_factory)
    rec = recs.get(case)
    log = recs["__log__"]
    if rec is None:
        pytest.fail(f"no record of {case} under setting {env_name}; " + (_dead[0] if _dead else log[-3000:]))
    for k in ("BSM_SS_SPLIT", "BSM_SS_PRESPLIT", "BSM_SS_WAVE"):  # the child really ran under the setting
        assert rec["env"].get(k) == ENVS[env_name].get(k), rec["env"]
    assert rec["ok"], f"{rec['call']}: {rec['what']} differs first at {rec['first_mismatch']}"
    # the four calls of the case went through the long-row pipeline
    part = log[log.index(f"BEGIN {case}\n"):log.index(f"END {case} ")]
    lines = DEBUG_LINE.findall(part)
    assert len(lines) == 4 and all(int(p) >= int(n) > 0 for n, _, p in lines), part[-2000:]


# ---- 7. special float values --------------------------------------------------
SPECIAL = [0.0, -0.0, np.nan, np.inf, -np.inf, 1.7, -1.7]


def special_case(dtype):
    """Every pair of stored +0.0, -0.0, NaN, +Inf, -Inf, x, -x at one column
    (Inf + -Inf, Inf - Inf, x + -x among them) and each of them alone on
    either side (0 - -0.0, 0 - +0.0 under sub): three short sorted rows, a
    sorted long row with the same pairs, and an unsorted long row with
    repeated columns, where the merge decides what meets what."""
    combos = ([(x, y) for x in SPECIAL for y in SPECIAL] + [(x, None) for x in SPECIAL]
              + [(None, y) for y in SPECIAL])
    rng = np.random.default_rng(71)

    def row(items, cols_of):
        ca = [c for c, (x, _) in zip(cols_of, items) if x is not None]
        cb = [c for c, (_, y) in zip(cols_of, items) if y is not None]
        return (ca, [x for x, _ in items if x is not None]), (cb, [y for _, y in items if y is not None])

    rows = [row(combos[i:i + 21], range(21)) for i in range(0, 63, 21)]
    rows.append(row(combos * 8, range(63 * 8)))
    shuffled = [combos[i] for i in rng.permutation(np.arange(63 * 16) % 63)]
    rows.append(row(shuffled, rng.integers(0, 40, len(shuffled)).tolist()))
    specs = []
    for side in (0, 1):
        rp = np.concatenate([[0], np.cumsum([len(r[side][0]) for r in rows])]).astype(np.uint64)
        ci = np.concatenate([np.asarray(r[side][0], np.uint64) for r in rows])
        v = np.concatenate([np.asarray(r[side][1], dtype) for r in rows])
        specs.append((rp, ci, v))
    return (len(rows), 600), specs[0], specs[1]


def assert_csr_bits_or_nan(got, rp, ci, v):
    """assert_csr_bits, except where the oracle's value is NaN: there the
    result is NaN too (a generated NaN's sign differs between host and GPU)."""
    ev = np.asarray(v, dtype=got.dtype)
    gv = np.asarray(got.v)
    assert np.array_equal(np.asarray(got.row_index, np.uint64), np.asarray(rp, np.uint64)), "row_ptr differs"
    assert np.array_equal(np.asarray(got.col_index, np.uint64), np.asarray(ci, np.uint64)), "col_idx differs"
    assert gv.shape == ev.shape and gv.dtype == ev.dtype
    nan = np.isnan(ev)
    assert np.array_equal(np.isnan(gv), nan), "NaN at other positions"
    bad = np.flatnonzero((W.bits(gv) != W.bits(ev)) & ~nan)
    assert bad.size == 0, f"{bad.size} values differ, first at {bad[:5]}: {gv[bad[:5]]} vs {ev[bad[:5]]}"


@gpu
@pytest.mark.parametrize("path", ["wave", "general"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_special_float_values(orc, capfd, monkeypatch, dtype, path):
    """Arith<T>::nz decides the output pattern: stored and computed +-0.0 are
    dropped, NaN and +-Inf kept, on the wave path and (BSM_SS_WAVE=0) on the
    thread path of the short rows and the pipeline of the long ones."""
    if path == "general":
        monkeypatch.setenv("BSM_SS_WAVE", "0")
    case = special_case(dtype)
    assert n_long_rows(case[1], case[2]) == 2 and longest(case[1]) + longest(case[2]) <= W.WROW_CAP
    check(orc, capfd, monkeypatch, case, pipeline=path == "general", cmp=assert_csr_bits_or_nan)


# ---- 8. the diagnostic levels of BSM_SS_DEBUG ---------------------------------
# Levels 2 and 4 hand piece_merge / piece_split a stamp buffer, level 3 ends
# every phase with a synchronise: each on the smallest long-row operands, on
# the general path (BSM_SS_WAVE=0: the row of 65 entries alone would take the
# wave path), with the result still the oracle's and as many pieces as under
# level 1.
DIAG_CASES = [f"diag:{kind}:{dt}" for kind in ("row65", "cap1") for dt in ("f64", "u32")]
DIAG_ENVS = {"level2": {"BSM_SS_WAVE": "0", "BSM_SS_SPLIT": "0", "BSM_SS_DEBUG": "2"},
             "level3": {"BSM_SS_WAVE": "0", "BSM_SS_DEBUG": "3"}}
MERGE_LINE = re.compile(r"\[bsm ss debug\] piece_merge over (\d+) pieces: per piece staging ")
SPLIT_LINE = re.compile(r"\[bsm ss split\] (\d+) pieces, mean ")
TIME_LINE = re.compile(r"^\[bsm ss time\] (.+?) +\d+\.\d{3} ms$", re.M)
TIME_LABELS = ["count + long-row scan", "long rows + extents", "row maxima + counts", "pieces", "piece_split + scan",
               "row scan + nnz", "output alloc", "fill + copy", "scope exit (frees)"]


def default_pieces(orc, capfd, monkeypatch, case):
    """The four calls' piece counts under level 1 (and the results against the oracle)."""
    monkeypatch.setenv("BSM_SS_WAVE", "0")
    return check(orc, capfd, monkeypatch, W.build(case))[0]


def diag_child(level, case, tmp_path_factory):
    """What the child of that level wrote while it ran `case`, its result checked."""
    recs = _child(level, tmp_path_factory, DIAG_ENVS[level], DIAG_CASES)
    rec, log = recs.get(case), recs["__log__"]
    if rec is None:
        pytest.fail(f"no record of {case} under {level}; " + (_dead[0] if _dead else log[-3000:]))
    for k in SWITCHES:  # the child really ran under the setting
        assert rec["env"].get(k) == DIAG_ENVS[level].get(k), rec["env"]
    assert rec["ok"], f"{rec['call']}: {rec['what']} differs first at {rec['first_mismatch']}"
    return log[log.index(f"BEGIN {case}\n"):log.index(f"END {case} ")]


@gpu
@pytest.mark.parametrize("case", DIAG_CASES)
def test_debug_level_2_piece_merge_stamps(orc, capfd, monkeypatch, tmp_path_factory, case):
    """BSM_SS_DEBUG=2 under BSM_SS_SPLIT=0 (a child): piece_merge writes its
    six stamps per piece and the host reports them, once per call."""
    pieces = default_pieces(orc, capfd, monkeypatch, case)
    part = diag_child("level2", case, tmp_path_factory)
    assert [int(p) for _, _, p in DEBUG_LINE.findall(part)] == pieces, part[-2000:]
    assert [int(p) for p in MERGE_LINE.findall(part)] == pieces, part[-2000:]


@gpu
@pytest.mark.parametrize("case", DIAG_CASES)
def test_debug_level_3_phase_times(orc, capfd, monkeypatch, tmp_path_factory, case):
    """BSM_SS_DEBUG=3 (read once per process: a child): every phase of every
    call ends with a synchronise and a line, the labels in their order."""
    pieces = default_pieces(orc, capfd, monkeypatch, case)
    part = diag_child("level3", case, tmp_path_factory)
    assert [int(p) for _, _, p in DEBUG_LINE.findall(part)] == pieces, part[-2000:]
    assert TIME_LINE.findall(part) == TIME_LABELS * 4, part[-3000:]


@gpu
@pytest.mark.parametrize("case", DIAG_CASES)
def test_debug_level_4_piece_split_stamps(orc, capfd, monkeypatch, case):
    """BSM_SS_DEBUG=4 (read per call: in this process): piece_split writes
    its nine stamps per piece and the host reports them, once per call."""
    pieces = default_pieces(orc, capfd, monkeypatch, case)
    got, err = check(orc, capfd, monkeypatch, W.build(case), debug="4")
    assert got == pieces and [int(p) for p in SPLIT_LINE.findall(err)] == pieces, err[-2000:]
