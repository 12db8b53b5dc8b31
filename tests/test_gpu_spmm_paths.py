"""Every SpMV / SpMM row kernel behind Csr::mul_dense and Csr::mul_vector
(csrc/kernels_spmm.hip, launch_spmm) at each scalar type, each start value
(+0 for mul_dense, -0 for mul_vector) and the chunk, tile and template edges
of that kernel, bit for bit against the oracle (sparse.rs:426-482).

Every test first asks the library which kernel it will launch for the shape
(bsm_dev_spmm_kernel, the host rule of csrc/spmm_rule.hpp that launch_spmm
itself switches on), so a test "of spmv_wave" cannot pass through another
kernel. The shapes keep the other schedules out of the way: X stays below the
sizes at which the tiled copy or the column panels are built.

Inputs are built in numpy, with non-decreasing columns (and repeats) in every
row, so mul_vector sums the very arrays the test built. Floats are drawn from
uniform(-2, 2) on both sides: sums pass through mixed signs, and
reorder_sensitive() asserts on the CPU, once per float matrix, that summing a
row's products in reversed storage order changes the bits of at least a third
of the rows with five entries or more. That third is a condition on the
inputs, not a tolerance: with these values the reference alone changes about
50 % of the rows of five entries, 68 % of twelve and 83 % of forty, in f32
and f64 alike. Integers take the full range of the type, so sums wrap.
"""

import numpy as np
import pytest

from basic_sparse_matrix_amd import Csr, Dense, _lib
from test_gpu_spmm import assert_csr_bits

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32, np.int32, np.uint32, np.int64, np.uint64]
UNKNOWN = 2**64 - 1  # max_row_len of the device-level call


class K:
    """enum class SpmmKernel (csrc/spmm_rule.hpp, include/bsm.h)"""

    NONE, THREAD12, WAVE8, WAVE12, WAVE16, ROWS16, STREAM2, STREAM4, STREAM8 = range(9)
    K32_ROWS4_U4, K32_ROWS4_U2, K32_WAVE4, K32_WAVE4_PIPE, K32_WAVE8_PIPE = range(9, 14)
    RW2_4, RW4_4, RW8_4, RW16_8, RW32_8, RW64_8 = range(14, 20)


STREAM = {2: K.STREAM2, 4: K.STREAM4, 8: K.STREAM8}


def rowwave_for(k):
    return K.RW2_4 if k <= 2 else K.RW4_4 if k <= 4 else K.RW8_4 if k <= 8 else K.RW16_8 if k <= 16 else \
        K.RW32_8 if k <= 32 else K.RW64_8


def kernel_of(dtype, rows, nnz, k, max_row_len, x=0, y=0):
    return _lib.load().bsm_dev_spmm_kernel(_lib.DTYPE_CODES[np.dtype(dtype)], rows, nnz, k, max_row_len, x, y)


def handle_kernel(m, k):
    """The kernel a handle call (mul_dense with k columns, mul_vector) runs on
    case m: the analysed longest row, aligned operands; neither the tiled copy
    nor the column panels are wanted for the shape."""
    lib = _lib.load()
    code = _lib.DTYPE_CODES[m.dt]
    assert not lib.bsm_dev_tiled_wanted(code, m.rows, m.n_cols, m.nnz, k, m.max_len)
    assert lib.bsm_dev_spmm_panel_cols(code, m.n_cols, k) == 0
    return kernel_of(m.dt, m.rows, m.nnz, k, m.max_len)


# ------------------------------------------------------------------ inputs
def values(rng, dt, n):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return rng.uniform(-2, 2, n).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def sorted_cols(rng, lens, n_cols):
    """Columns non-decreasing inside every row, with repeats."""
    rows_of = np.repeat(np.arange(len(lens)), lens)
    c = rng.integers(0, n_cols, int(lens.sum()))
    return c[np.lexsort((c, rows_of))].astype(np.uint64)


def seq_sum(p):
    return np.cumsum(p, dtype=p.dtype)[-1]  # cumsum adds one by one, in order


def reorder_sensitive(rp, ci, v, x):
    """The inputs can tell a reordered sum from the right one (module docstring)."""
    p = v * x[ci.astype(np.int64)]
    rp = rp.astype(np.int64)
    ib = np.uint64 if v.dtype.itemsize == 8 else np.uint32
    long = np.nonzero(np.diff(rp) >= 5)[0]
    changed = sum(int(seq_sum(p[rp[r]:rp[r + 1]]).view(ib) != seq_sum(p[rp[r]:rp[r + 1]][::-1]).view(ib))
                  for r in long)
    assert len(long) >= 20 and 3 * changed >= len(long), (len(long), changed)


class Case:
    """A matrix, k right-hand columns and the oracle's two results (computed
    once, shared, never written)."""

    def __init__(self, orc, rng, lens, n_cols, dtype, k=1, vector=True, sensitive=True):
        self.dt = np.dtype(dtype)
        lens = np.asarray(lens, dtype=np.int64)
        self.rows, self.n_cols, self.k = len(lens), n_cols, k
        self.lens = lens
        self.rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.nnz = int(self.rp[-1])
        self.max_len = int(lens.max()) if len(lens) else 0
        self.ci = sorted_cols(rng, lens, n_cols)
        self.v = values(rng, self.dt, self.nnz)
        self.x_cols = [values(rng, self.dt, n_cols) for _ in range(k)]
        if self.dt.kind == "f" and sensitive:
            reorder_sensitive(self.rp, self.ci, self.v, self.x_cols[0])
        self.finish(orc, vector)

    def finish(self, orc, vector=True):
        self.csr = Csr.from_csr_arrays((self.rows, self.n_cols), self.rp, self.ci, self.v)
        self.exp_dense = orc.mul_dense(self.rows, self.n_cols, self.rp, self.ci, self.v, self.x_cols)
        self.exp_vec = orc.mul_vector(self.rows, self.n_cols, self.rp, self.ci, self.v, self.x_cols[0]) \
            if vector else None
        for a in (self.rp, self.ci, self.v, *self.x_cols, *self.exp_dense):
            a.flags.writeable = False

    def mul_dense(self):
        return self.csr.mul_dense(Dense.from_columns(self.x_cols))

    def mul_vector(self):
        out = np.full(self.rows, 7, dtype=self.dt)  # every row must be written
        self.csr.mul_vector(self.x_cols[0], out)
        return out


_cases = {}


@pytest.fixture(scope="module", autouse=True)
def release_cases():
    """The shared cases (and their device handles) live as long as this module's tests."""
    yield
    _cases.clear()


def cached(key, make):
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def assert_vector_bits(m, out):
    bad = np.nonzero(bits(out) != bits(m.exp_vec))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}: {out[bad[:5]]} vs {m.exp_vec[bad[:5]]}"
    empty = m.lens == 0
    assert empty.any()
    if m.dt.kind == "f":  # float Sum starts from -0.0: an empty row is -0.0, sign bit set
        assert np.all(out[empty] == 0) and np.all(np.signbit(out[empty]))
    else:
        assert np.all(out[empty] == 0)


def partition(rng, total, n, avoid=None):
    """n row lengths (empty ones included) adding up to total; with avoid, some
    row starts before entry `avoid` and ends after it (it straddles that edge)."""
    cuts = np.sort(rng.integers(0, total + 1, n - 1))
    if avoid is not None:
        assert 1 < avoid < total
        cuts[cuts == avoid] -= 1
    lens = np.diff(np.concatenate([[0], cuts, [total]]))
    if avoid is not None:
        starts = np.cumsum(lens) - lens
        assert np.any((starts < avoid) & (starts + lens > avoid))
    return lens


# ------------------------------------- 1. the short-row SpMV kernels' edges
SPMV_CONFIGS = [(0, None), (1, 2), (1, 4), (1, 8), (2, None), (3, None), (4, None), (5, None), (6, None)]
BY_VARIANT = {2: K.ROWS16, 3: K.WAVE16, 4: K.WAVE12, 5: K.WAVE8, 6: K.THREAD12}


def thread_lens(rng):
    """spmv_thread<12>: U = 12 entries per pass, so 0, 1, 11, 12, 13, 24, 25,
    48; empty rows first, last and in runs; 5 x 256 + 1 rows; nothing longer
    than 48, so the default kernel for this matrix is spmv_thread."""
    cyc = [0, 1, 11, 12, 13, 24, 25, 48, 0, 0, 1, 0, 2, 0, 3, 0]
    lens = np.array(([0] * 3 + cyc * 80)[:1281])
    lens[-2:] = [48, 0]
    return lens


def wave_lens(rng):
    """spmv_wave<ITEMS>: one wave per 64 rows, CAP = 64 ITEMS entries per
    chunk. For each CAP (512, 768, 1024): 64-row groups of CAP - 1, CAP,
    CAP + 1 and 2 CAP + 1 entries (the last two with a row across the chunk
    edge); a group of empty rows first; a group with one row longer than every
    CAP; light groups; a last group of one row. 6 x 256 + 1 rows."""
    groups = [np.zeros(64, dtype=np.int64)]
    for cap in (512, 768, 1024):
        for e in (cap - 1, cap, cap + 1, 2 * cap + 1):
            groups.append(partition(rng, e, 64, cap if e > cap else None))
    g = partition(rng, 100, 64)
    g[20] = 1100
    groups.append(g)
    while len(groups) < 24:
        groups.append(rng.integers(0, 4, 64))
    groups.append(np.array([5]))
    return np.concatenate(groups)


def rows_lens(rng):
    """spmv_rows<16>: one workgroup per 256 rows, 4096 entries per chunk:
    256-row blocks of 4095, 4096, 4097 and 8193 entries (the last two with a
    row across the chunk edge), an empty block first, light blocks, a last
    block of one empty row. 8 x 256 + 1 rows."""
    blocks = [np.zeros(256, dtype=np.int64)]
    for e in (4095, 4096, 4097, 8193):
        blocks.append(partition(rng, e, 256, 4096 if e > 4096 else None))
    for _ in range(3):
        blocks.append(rng.integers(0, 4, 256))
    blocks.append(np.array([0]))
    return np.concatenate(blocks)


SPMV_MATRICES = {"thread": (thread_lens, K.THREAD12), "wave": (wave_lens, K.WAVE8), "rows": (rows_lens, K.WAVE8)}


def spmv_case(orc, name, dtype):
    def make():
        rng = np.random.default_rng([11, sorted(SPMV_MATRICES).index(name), DTYPES.index(dtype)])
        m = Case(orc, rng, SPMV_MATRICES[name][0](rng), 300, dtype)
        assert m.rows % 256 == 1 and m.nnz <= 12 * m.rows  # the short-row side of SPMV_ROWS_AVG
        assert m.lens[0] == 0 and (m.lens[-1] == 0 or name == "wave")
        return m

    return cached(("spmv", name, dtype), make)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(SPMV_MATRICES))
def test_spmv_short_row_kernels_at_their_edges(orc, monkeypatch, name, dtype):
    """One ragged matrix per short-row kernel (spmv_thread, spmv_wave,
    spmv_rows) holding that kernel's edges, through every BSM_SPMV_VARIANT
    0..6 and BSM_SPMV_ITEMS 2 / 4 / 8 under variant 1, by mul_dense with one
    column (+0 start, row counts written) and by mul_vector (-0 start, no row
    counts): all six scalar types, the kernel asserted before the bits. In
    mul_vector every empty float row is -0.0 and every empty integer row 0."""
    m = spmv_case(orc, name, dtype)
    default = SPMV_MATRICES[name][1]
    assert (default == K.THREAD12) == (m.max_len <= 48)
    for variant, items in SPMV_CONFIGS:
        monkeypatch.setenv("BSM_SPMV_VARIANT", str(variant))
        monkeypatch.setenv("BSM_SPMV_ITEMS", str(items or 4))
        want = default if variant == 0 else STREAM[items] if variant == 1 else BY_VARIANT[variant]
        assert handle_kernel(m, 1) == want, (variant, items)
        assert_csr_bits(m.mul_dense(), *m.exp_dense)
        assert_vector_bits(m, m.mul_vector())


# ------------------------------------------------ 2. spmv_stream's own edges
STREAM_DTYPES = [np.float64, np.float32, np.int32, np.uint64]


def stream_lens(rng, items):
    """Workgroup b of spmv_stream<ITEMS> owns the rows that start in entries
    [b CHUNK, (b + 1) CHUNK), CHUNK = 256 ITEMS; it keeps up to CAP = 2 CHUNK
    products in LDS and falls back beyond. Each segment below starts on a
    multiple of CHUNK (a filler row realigns after it), so its rows are one
    workgroup's:
      leading empty rows; 600 rows of 0 or 1 entries (three trips of the
      256-thread row loop, rp reloaded after the first); n == CAP and
      n == CAP + 1 (the switch to the fallback); rows of CHUNK and CHUNK + 1
      alone; long rows of CAP, CAP + 1 and 2 CAP + 1 (one, two and three
      workgroup passes); ordinary rows; trailing empty rows.
    In the fallback the rows before the last one start inside one chunk, so
    they hold at most CHUNK - 1 entries together, and n > CAP then makes the
    last row at least CHUNK + 2 long: (CHUNK - 1, CHUNK + 2) is the closest
    pair the fallback can meet, and a fallback row of exactly CHUNK or
    CHUNK + 1 entries cannot exist. (CHUNK - 1, CHUNK + 1) is n == CAP."""
    C = 256 * items
    CAP = 2 * C
    lens = []

    def seg(ls):
        assert sum(lens) % C == 0
        lens.extend(int(x) for x in ls)
        pad = -sum(lens) % C
        if pad:
            lens.append(pad)

    seg([0] * 5 + [3, 0, 2])
    ones = np.zeros(600, dtype=np.int64)
    ones[rng.choice(600, 250, replace=False)] = 1
    seg(ones)
    seg([10, CAP - 10])      # n == CAP: LDS
    seg([11, CAP - 10])      # n == CAP + 1: fallback, thread sum + workgroup pass
    seg([C - 1, C + 2])      # fallback: the longest short row, the shortest long row
    seg([C - 1, C + 1])      # n == CAP with a row of CHUNK + 1
    seg([C])
    seg([C + 1])
    seg([CAP])
    seg([CAP + 1])
    seg([0, 2 * CAP + 1, 0])
    seg(rng.integers(0, 30, 200))
    lens.extend([0, 0, 0])
    return np.array(lens)


def stream_tail_lens(rng, items):
    """nnz == 3 CHUNK exactly, then five empty rows: the last workgroup starts
    at lo == nnz and owns only those."""
    C = 256 * items
    lens = []
    while sum(lens) < 3 * C:
        lens.append(min(int(rng.integers(5, 40)), 3 * C - sum(lens)))
    return np.array(lens + [0] * 5)


@pytest.mark.parametrize("items", [2, 4, 8])
@pytest.mark.parametrize("dtype", STREAM_DTYPES)
def test_spmv_stream_at_its_edges(orc, monkeypatch, dtype, items):
    """spmv_stream<2 | 4 | 8> on stream_lens and stream_tail_lens (their
    docstrings list the edges), reached by the default route (more than 12
    entries per row on average), through mul_dense and mul_vector."""
    monkeypatch.setenv("BSM_SPMV_ITEMS", str(items))
    for i, make_lens in enumerate((stream_lens, stream_tail_lens)):
        def make():
            rng = np.random.default_rng([12, i, items, DTYPES.index(dtype)])
            return Case(orc, rng, make_lens(rng, items), 500, dtype)

        m = cached(("stream", i, items, dtype), make)
        assert m.nnz > 12 * m.rows and (i == 0 or (m.nnz == 3 * 256 * items and not m.lens[-5:].any()))
        assert handle_kernel(m, 1) == STREAM[items]
        assert_csr_bits(m.mul_dense(), *m.exp_dense)
        assert_vector_bits(m, m.mul_vector())


@pytest.mark.parametrize("rows", [4097, 262145])
@pytest.mark.parametrize("dtype", STREAM_DTYPES)
def test_spmv_stream_row_search_rounds(orc, monkeypatch, dtype, rows):
    """wave_lower_bound_rp probes 64 rows per round: 4,097 rows take three
    rounds and 262,145 take four. Mostly empty rows with a few thousand
    entries (first and last row included), so BSM_SPMV_VARIANT=1 sends them
    to spmv_stream, where each workgroup owns thousands of rows."""
    def make():
        rng = np.random.default_rng([13, rows, DTYPES.index(dtype)])
        lens = np.zeros(rows, dtype=np.int64)
        pick = np.concatenate([[0, 1, 4095, 4096, rows - 2, rows - 1], rng.choice(rows, 1500, replace=False)])
        lens[pick] = rng.integers(1, 4, len(pick))
        lens[rng.choice(rows, 8, replace=False)] = 9  # rows of five entries or more for reorder_sensitive
        lens[rng.choice(rows, 40, replace=False)] = rng.integers(5, 9, 40)
        return Case(orc, rng, lens, 700, dtype)

    m = cached(("rounds", rows, dtype), make)
    monkeypatch.setenv("BSM_SPMV_VARIANT", "1")
    for items in (2, 4, 8):
        monkeypatch.setenv("BSM_SPMV_ITEMS", str(items))
        assert handle_kernel(m, 1) == STREAM[items]
        assert_csr_bits(m.mul_dense(), *m.exp_dense)
        assert_vector_bits(m, m.mul_vector())


# -------------------------------------------- 3. the scan past one carry block
def test_scan_past_one_carry_block(orc, monkeypatch):
    """exclusive_scan_i32_to_i64 scans the per-row result counts in tiles of
    4,096 rows and scan_tile_prefix walks the tile sums in blocks of 256 with a
    carry: 257 x 4,096 + 5 rows put the last two tiles in a second block.
    About 50,000 rows of one to three entries (the last rows among them), the
    rest empty; k = 1 by the default kernel and by spmv_stream; row_ptr,
    col_idx and values against the oracle."""
    rows = 257 * 4096 + 5
    rng = np.random.default_rng(14)
    lens = np.zeros(rows, dtype=np.int64)
    pick = np.concatenate([rng.choice(rows, 50000, replace=False), np.arange(rows - 4200, rows, 7), [0, rows - 1]])
    lens[pick] = rng.integers(1, 4, len(pick))
    lens[rng.choice(rows, 60, replace=False)] = rng.integers(5, 12, 60)
    m = Case(orc, rng, lens, 1000, np.float64, vector=False)
    erp = m.exp_dense[0]
    assert erp[256 * 4096] > 0 and erp[-1] > erp[256 * 4096]  # a carry, and results after it
    for variant, want in (("0", K.WAVE8), ("1", K.STREAM4)):
        monkeypatch.setenv("BSM_SPMV_VARIANT", variant)
        assert handle_kernel(m, 1) == want
        assert_csr_bits(m.mul_dense(), *m.exp_dense)


# ----------------------------------- 4. special values through every family
def assert_csr_bits_nan(got, rp, ci, v):
    """Structure exact (a NaN result is a stored entry, sparse.rs:229 drops
    only == 0); values bit-exact where the oracle's is not NaN, NaN where it
    is (payload and sign of a NaN differ between the host and the GPU)."""
    assert np.array_equal(np.asarray(got.row_index, np.uint64), np.asarray(rp, np.uint64)), "row_ptr differs"
    assert np.array_equal(np.asarray(got.col_index, np.uint64), np.asarray(ci, np.uint64)), "col_idx differs"
    assert_values_nan(np.asarray(got.v), v)


def assert_values_nan(gv, ev):
    assert gv.dtype == ev.dtype and gv.shape == ev.shape
    nan = np.isnan(ev)
    assert np.all(np.isnan(gv[nan])), "a NaN of the oracle is not NaN"
    bad = np.nonzero(bits(gv)[~nan] != bits(ev)[~nan])[0]
    assert bad.size == 0, f"{bad.size} values differ, first at {bad[:5]}: {gv[~nan][bad[:5]]} vs {ev[~nan][bad[:5]]}"


def special_case(orc, dtype, k):
    """A and x seeded with +0.0, -0.0, NaN, +Inf, -Inf, subnormals and
    magnitudes whose products overflow, among uniform(-2, 2) values: fixed
    rows whose sums are a subnormal, -0.0 (from -0 alone), an overflow, NaN by
    Inf - Inf and by 0 x Inf and an exact cancellation, then random rows of 0
    to 20 entries with every sixth value special."""
    dt = np.dtype(dtype)
    sub, big = (1e-40, 1e30) if dt == np.float32 else (5e-310, 1e200)
    spec = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, sub, -sub, big, -big], dtype=dt)
    assert 0 < spec[5] < np.finfo(dt).tiny
    head = np.array([1.0, 0.0, -0.0, np.nan, np.inf, -np.inf, sub, big, -big, 0.5], dtype=dt)
    fixed = [[(0, sub), (0, sub)], [(6, 1.0)], [(6, 0.5), (6, 0.5)], [(2, 1.0)], [(1, -1.0), (2, 1.0)], [(7, big)],
             [(7, big), (8, big)], [(1, np.inf)], [(3, 0.0)], [(0, 1.5), (0, -1.5)], [(0, sub), (0, -sub), (9, sub)],
             [], [(0, sub), (9, -sub), (9, 3 * sub)]]

    def make():
        rng = np.random.default_rng([15, DTYPES.index(dtype), k])
        n_cols = 64
        lens = np.concatenate([[len(r) for r in fixed], rng.integers(0, 21, 400), [0]]).astype(np.int64)
        m = Case.__new__(Case)
        m.dt, m.lens, m.rows, m.n_cols, m.k = dt, lens, len(lens), n_cols, k
        m.rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        m.nnz, m.max_len = int(m.rp[-1]), int(lens.max())
        m.ci = sorted_cols(rng, lens, n_cols)
        m.v = values(rng, dt, m.nnz)
        hit = rng.random(m.nnz) < 1 / 6
        m.v[hit] = spec[rng.integers(0, len(spec), int(hit.sum()))]
        nf = sum(len(r) for r in fixed)
        m.ci[:nf] = [c for r in fixed for c, _ in r]
        m.v[:nf] = [val for r in fixed for _, val in r]
        x = values(rng, dt, n_cols)
        hit = rng.random(n_cols) < 1 / 6
        x[hit] = spec[rng.integers(0, len(spec), int(hit.sum()))]
        x[:10] = head
        # column j is x rotated by j inside the head and inside the rest, so every column meets every special
        m.x_cols = [np.concatenate([np.roll(x[:10], j), np.roll(x[10:], 3 * j)]) for j in range(k)]
        with np.errstate(all="ignore"):
            m.finish(orc)
        ev = m.exp_dense[2]
        assert np.isnan(ev).any() and np.isinf(ev).any()
        assert np.any((ev != 0) & (np.abs(ev) < np.finfo(dt).tiny)), "no subnormal result to keep"
        assert m.nnz <= 12 * m.rows and m.max_len <= 48
        return m

    return cached(("special", dtype, k), make)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_special_values_spmv_kernels(orc, monkeypatch, dtype):
    """special_case through BSM_SPMV_VARIANT 0..6 (spmv_thread, spmv_stream,
    spmv_rows, spmv_wave<16 | 12 | 8>, spmv_thread), by mul_dense and by
    mul_vector: subnormal sums kept (f32 1e-40, f64 5e-310: a build that
    flushed them fails), NaN results NaN and stored, the rest bit-exact."""
    m = special_case(orc, dtype, 1)
    for variant in range(7):
        monkeypatch.setenv("BSM_SPMV_VARIANT", str(variant))
        want = K.THREAD12 if variant == 0 else K.STREAM4 if variant == 1 else BY_VARIANT[variant]
        assert handle_kernel(m, 1) == want
        assert_csr_bits_nan(m.mul_dense(), *m.exp_dense)
        assert_values_nan(m.mul_vector(), m.exp_vec)
    ev = m.exp_vec
    assert np.any((ev == 0) & np.signbit(ev) & (m.lens > 0))  # -0.0 from entries, not only from empty rows


@pytest.mark.parametrize("dtype,k,variant,want", [
    (np.float64, 3, 0, K.RW4_4), (np.float32, 3, 0, K.RW4_4), (np.float32, 32, 0, K.RW32_8),
    (np.float64, 32, 0, K.K32_ROWS4_U4), (np.float64, 32, 1, K.RW32_8), (np.float64, 32, 2, K.K32_WAVE4),
    (np.float64, 32, 3, K.K32_WAVE4_PIPE), (np.float64, 32, 4, K.K32_WAVE8_PIPE),
    (np.float64, 32, 5, K.K32_ROWS4_U4), (np.float64, 32, 6, K.K32_ROWS4_U2)])
def test_special_values_spmm_kernels(orc, monkeypatch, dtype, k, variant, want):
    """special_case through spmm_rowwave at k = 3, f32 at k = 32 and every
    k = 32 f64 kernel (BSM_SPMM_VARIANT 0..6)."""
    monkeypatch.setenv("BSM_SPMM_VARIANT", str(variant))
    m = special_case(orc, dtype, k)
    assert handle_kernel(m, k) == want
    assert_csr_bits_nan(m.mul_dense(), *m.exp_dense)


# ------------------------------------------- 5. spmm_rowwave's template edges
ROWWAVE_KS = [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129]


@pytest.mark.parametrize("k", ROWWAVE_KS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32, np.uint64])
def test_rowwave_every_k_edge_and_row_length(orc, monkeypatch, dtype, k):
    """spmm_rowwave<T, KL, U> gathers S = 64 / KL entries per instruction and
    S U per step: 301 = 4 x 75 + 1 rows whose lengths are every value 0..300
    cover S, S U and their neighbours for all six instantiations, and
    k = KL, KL + 1, 128 and 129 the column-block loop's one, two and three
    passes. f64 at k = 32 is forced here by BSM_SPMM_VARIANT=1."""
    if np.dtype(dtype) == np.float64 and k == 32:
        monkeypatch.setenv("BSM_SPMM_VARIANT", "1")

    def make():
        rng = np.random.default_rng([16, DTYPES.index(dtype), k])
        return Case(orc, rng, rng.permutation(301), 200, dtype, k=k, vector=False)

    m = cached(("rowwave", dtype, k), make)
    assert handle_kernel(m, k) == rowwave_for(k)
    assert_csr_bits(m.mul_dense(), *m.exp_dense)


def k32_lens(rng, rows):
    """Four rows per wave (spmm_k32_f64_rows4), sixteen per workgroup: groups
    of four rows with one long row in each of the four places and three empty
    ones, a wave of four empty rows, then every length 0..100, then short rows
    up to `rows`."""
    head = [200, 0, 0, 0, 0, 150, 0, 0, 0, 0, 0, 0, 0, 0, 130, 0, 0, 0, 0, 90]
    lens = np.concatenate([head, rng.permutation(101), rng.integers(0, 6, rows - 121)])
    assert len(lens) == rows
    return lens


@pytest.mark.parametrize("rows", [129, 143])
@pytest.mark.parametrize("variant,want", [(2, K.K32_WAVE4), (3, K.K32_WAVE4_PIPE), (4, K.K32_WAVE8_PIPE),
                                          (5, K.K32_ROWS4_U4), (6, K.K32_ROWS4_U2)])
def test_k32_f64_kernels_every_row_length(orc, monkeypatch, variant, want, rows):
    """The k = 32 f64 kernels on rows of every length 0..100 (chunks of 16 and
    32 entries with a four-entry tail; U = 4 and 2 for the four-row kernels),
    with rows % 16 of 1 and 15 and the groups of k32_lens."""
    monkeypatch.setenv("BSM_SPMM_VARIANT", str(variant))

    def make():
        rng = np.random.default_rng([17, rows])
        return Case(orc, rng, k32_lens(rng, rows), 200, np.float64, k=32, vector=False)

    m = cached(("k32", rows), make)
    assert rows % 16 in (1, 15)
    assert handle_kernel(m, 32) == want
    assert_csr_bits(m.mul_dense(), *m.exp_dense)


# --------------------------------------------------- 6. misaligned operands
def dense_of(m):
    rp, ci, v = m.exp_dense
    y = np.zeros((m.rows, m.k), dtype=m.dt)
    y[np.repeat(np.arange(m.rows), np.diff(rp.astype(np.int64))), ci.astype(np.int64)] = v
    return y


@pytest.mark.parametrize("avg", [10, 40])
def test_misaligned_operands_take_the_generic_kernel(orc, avg):
    """The k = 32 f64 kernels load double2, so x and y must sit on 16-byte
    addresses; an operand 8 bytes into a larger tensor sends bsm_dev_spmm to
    spmm_rowwave<double, 32, 8>, and bsm_dev_spmm_panelled with a plan built
    falls back to it as well (it must not reinterpret). Same bits as the
    aligned run and as the oracle. avg 10 / 40: the aligned kernel is the
    four-row one / the pipelined one-row one."""
    import torch

    from basic_sparse_matrix_amd import device

    k, rows, n_cols = 32, 333, 400
    rng = np.random.default_rng([18, avg])
    m = Case(orc, rng, rng.integers(0, 2 * avg + 1, rows), n_cols, np.float64, k=k, vector=False)
    exp = torch.from_numpy(dense_of(m)).view(torch.int64)
    blk = device.DeviceCsrBlock(0, rows, n_cols, torch.from_numpy(m.rp.astype(np.int64)).cuda(),
                                torch.from_numpy(m.ci.astype(np.int32)).cuda(), torch.from_numpy(m.v.copy()).cuda(),
                                m.dt)
    x_host = torch.from_numpy(np.ascontiguousarray(np.stack(m.x_cols, axis=1)))
    x_al = x_host.cuda()
    x_big = torch.empty(n_cols * k + 1, dtype=torch.float64, device="cuda")
    x_mis = x_big[1:].view(n_cols, k)
    x_mis.copy_(x_al)
    y_big = torch.empty(rows * k + 1, dtype=torch.float64, device="cuda")
    y_mis = y_big[1:].view(rows, k)
    y_al = torch.empty((rows, k), dtype=torch.float64, device="cuda")
    assert x_al.data_ptr() % 16 == 0 and y_al.data_ptr() % 16 == 0
    assert x_mis.data_ptr() % 16 == 8 and y_mis.data_ptr() % 16 == 8
    aligned_kernel = K.K32_ROWS4_U4 if m.nnz <= 24 * rows else K.K32_WAVE4_PIPE
    assert (avg == 10) == (m.nnz <= 24 * rows)

    def run(x, y, want):
        assert kernel_of(m.dt, rows, m.nnz, k, UNKNOWN, x.data_ptr(), y.data_ptr()) == want
        y.fill_(float("nan"))
        nz = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        blk.spmm(x, y, nz)
        torch.cuda.synchronize()
        assert torch.equal(y.cpu().view(torch.int64), exp)
        assert torch.equal(nz.cpu(), (y != 0).sum(dim=1).to(torch.int32).cpu())

    for plan in (0, 100):
        assert blk.plan(k, panel_cols=plan) == plan
        run(x_al, y_al, aligned_kernel)  # with a plan: the panel passes (the rule is not asked)
        run(x_mis, y_al, K.RW32_8)
        run(x_al, y_mis, K.RW32_8)
        run(x_mis, y_mis, K.RW32_8)


# ------------------------------------- 7. spmm_split_int's slice boundaries
def split_lens(rng):
    """Each wave of spmm_split_int sums a slice of 512 entries; a row cut by
    the slices leaves one partial per slice (slot 1 where it starts, slot 0 in
    the later ones). Entry positions in brackets:
      a row from a multiple of 512 past the next one [0, 700); a row ending
      exactly on one [700, 1024); two empty rows on the boundary; a row of
      exactly 512 aligned [1024, 1536), stored whole; an empty row; a row of
      1,024 aligned [1536, 2560), two slices; [2560, 2660); a row over parts
      of two slices and three whole ones [2660, 4658); short rows; a last row
      that makes nnz a multiple of 512; two empty rows."""
    lens = [700, 324, 0, 0, 512, 0, 1024, 100, 1998] + [int(x) for x in rng.integers(0, 10, 150)]
    lens.append(512 - sum(lens) % 512)
    return np.array(lens + [0, 0])


@pytest.mark.parametrize("k", [2, 3, 33, 64, 65, 129])
@pytest.mark.parametrize("dtype", [np.int32, np.uint32, np.int64, np.uint64])
def test_split_int_rows_on_slice_boundaries(orc, monkeypatch, dtype, k):
    """The nnz-balanced integer schedule (BSM_SPMM_SPLIT=1 forces it below its
    8,192-entry threshold) on split_lens, full-range values. The schedule is
    chosen before the kernel rule, whose answer for the shape is the row-wave
    kernel it replaces."""
    def make():
        rng = np.random.default_rng([19, DTYPES.index(dtype), k])
        m = Case(orc, rng, split_lens(rng), 300, dtype, k=k, vector=False)
        rp = m.rp.astype(np.int64)
        assert m.nnz % 512 == 0 and rp[1] > 512 and rp[2] == 1024 and rp[4] == 1024 and rp[5] == 1536
        assert rp[7] == 2560 and rp[8] % 512 and (rp[9] - 1) // 512 - rp[8] // 512 == 4
        return m

    m = cached(("split", dtype, k), make)
    wants_split = lambda: _lib.load().bsm_dev_spmm_wants_split(_lib.DTYPE_CODES[m.dt], k, m.max_len)
    assert handle_kernel(m, k) == rowwave_for(k)
    assert m.max_len < 8192 and wants_split() == 0  # unset: the row-wave kernel, by the row-length threshold
    monkeypatch.setenv("BSM_SPMM_SPLIT", "0")
    assert wants_split() == 0
    assert_csr_bits(m.mul_dense(), *m.exp_dense)
    monkeypatch.setenv("BSM_SPMM_SPLIT", "1")
    assert wants_split() == 1  # what spmm_launch_locked asks before it launches spmm_split_dispatch
    assert_csr_bits(m.mul_dense(), *m.exp_dense)


def test_kernel_query_rejects_an_unknown_dtype():
    lib = _lib.load()
    assert lib.bsm_dev_spmm_kernel(6, 10, 10, 1, 5, 0, 0) == -1
    assert lib.bsm_dev_spmm_kernel(-1, 10, 10, 1, 5, 0, 0) == -1
    assert kernel_of(np.float64, 0, 0, 32, 0) == K.NONE
    assert lib.bsm_dev_spmm_wants_split(6, 2, 9000) == -1
    split = lib.bsm_dev_spmm_wants_split
    assert split(_lib.BSM_I32, 2, 8192) == 1 and split(_lib.BSM_I32, 2, 8191) == 0
    assert split(_lib.BSM_F32, 2, 9000) == 0 and split(_lib.BSM_U64, 1, 9000) == 0
