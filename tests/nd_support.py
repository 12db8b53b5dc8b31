"""What the GPU tests of the nd solver share: the named systems with their
BSM_ND_LEAF, the right-hand sides, and the comparisons. Each test file keeps
its own list of the systems it runs and its own account of why those and why
its bounds; a helper that only one feature uses stays in that feature's file.

Everything cached here is shared by every test file of a session, so the
arrays it hands out are read-only: a test that wants to change one copies it
first. The package is imported where a Csr or a Dense is made, so the tests of
the oracle alone can take csr_arrays from here."""

import functools

import numpy as np

# (g, BSM_ND_LEAF) of orc.poisson2d(g): one-pivot fronts with 63 padding pivots (leaf1), several levels (g11-leaf8),
# one dense front of two pivot tiles (onefront), a parent more than one level above a child (g40-leaf64), leaves of
# several pivot tiles (g40-leaf256)
POISSON = {"g5-leaf1": (5, "1"), "g9-leaf1": (9, "1"), "g11-leaf8": (11, "8"), "g11-onefront": (11, "100000"),
           "g40-leaf64": (40, "64"), "g40-leaf256": (40, "256")}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- comparisons ----------------------------------------------------------------


def rel_err(x, ref):
    x = np.asarray(x, np.float64)
    ref = np.asarray(ref, np.float64)
    return np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def assert_same(got, want, what=""):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), (what, i)


def cols_of(d):
    return [np.asarray(d.get_col(j)).copy() for j in range(d.get_dims().cols)]


def csr_parts(m):
    return [np.asarray(m.row_index).copy(), np.asarray(m.col_index).copy(), np.asarray(m.v).copy()]


# ---- dense <-> CSR --------------------------------------------------------------


def csr_arrays(a):
    """(row_ptr, col, values) of the nonzeros of a dense matrix, square or not."""
    nzr, nzc = np.nonzero(a != 0)
    rp = np.concatenate([[0], np.cumsum(np.bincount(nzr, minlength=a.shape[0]))]).astype(np.uint64)
    return rp, nzc.astype(np.uint64), a[nzr, nzc]


def dense_of(rp, ci, v, n):
    a = np.zeros((n, n), dtype=np.float64)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(rp).astype(np.int64)))
    a[rows, np.asarray(ci).astype(np.int64)] = np.asarray(v, dtype=np.float64)
    return a


# ---- the systems ----------------------------------------------------------------


def _block_diag(g, factors, eye):
    """diag(f P for f in factors, 3 I_eye), P the Poisson matrix of a g x g grid."""
    import scipy.sparse as sp
    from oracle import pyoracle as orc

    rp, ci, v = orc.poisson2d(g)
    P = sp.csr_matrix((v, ci.astype(np.int64), rp.astype(np.int64)), shape=(g * g, g * g))
    M = sp.block_diag([f * P for f in factors] + ([sp.identity(eye) * 3.0] if eye else []), format="csr")
    M.sort_indices()
    return M.shape[0], M.indptr.astype(np.uint64), M.indices.astype(np.uint64), M.data.astype(np.float64)


@functools.lru_cache(maxsize=None)
def system(name):
    """(n, rp, ci, v as f64, leaf or None), built once."""
    from oracle import pyoracle as orc

    if name in POISSON:
        g, leaf = POISSON[name]
        rp, ci, v = orc.poisson2d(g)
        n, v = g * g, np.asarray(v, dtype=np.float64)
    elif name == "blocks":  # two grids and nine isolated vertices: fronts with np == 0
        (n, rp, ci, v), leaf = _block_diag(12, [1.0, 2.0], 9), None
    elif name == "triple":  # three copies of the 7 x 7-grid Poisson matrix: every eigenvalue three times and more
        (n, rp, ci, v), leaf = _block_diag(7, [1.0, 1.0, 1.0], 0), None
    elif name == "random":  # an irregular tree
        rng = np.random.default_rng(7)
        n, leaf = 300, None
        a = np.zeros((n, n))
        mask = rng.random((n, n)) < 0.02
        vals = rng.uniform(-1.0, 1.0, (n, n))
        a[mask] = vals[mask]
        a = np.tril(a, -1)
        a = a + a.T
        a[np.arange(n), np.arange(n)] = np.abs(a).sum(axis=1) + 1.0 + rng.random(n)
        rp, ci, v = csr_arrays(a)
    else:
        raise KeyError(name)
    return (n, *_frozen(rp, ci, v), leaf)


@functools.lru_cache(maxsize=None)
def dense_system(name):
    """(n, S dense f64, the leaf for the host analysis, BSM_ND_LEAF) of a Poisson system or of `blocks`, for the
    tests that choose their entries through nd_analyse's tree. These run `blocks` with BSM_ND_LEAF=64: at the default
    leaf the two grids are one leaf each and no front is empty."""
    n, rp, ci, v, leaf = system(name)
    if name == "blocks":
        leaf = "64"
    (s,) = _frozen(dense_of(rp, ci, v, n))
    return n, s, int(leaf), leaf


def dense_setup(monkeypatch, name):
    monkeypatch.setenv("BSM_ND_LEAF", dense_system(name)[3])


def dense_matrix(s, dtype):
    """A fresh Csr of the nonzeros of a dense matrix."""
    from basic_sparse_matrix_amd import Csr

    rp, ci, v = csr_arrays(s)
    return Csr.from_csr_arrays(s.shape, rp, ci, v.astype(dtype))


@functools.lru_cache(maxsize=None)
def coords(name):
    """(rows, cols) of the stored entries, in storage order."""
    n, rp, ci, _, _ = system(name)
    return _frozen(np.repeat(np.arange(n), np.diff(rp.astype(np.int64))), ci.astype(np.int64))


@functools.lru_cache(maxsize=None)
def rhs_cols(name):
    """Three f64 right-hand columns."""
    from oracle import pyoracle as orc

    return _frozen(*(np.asarray(c, dtype=np.float64) for c in orc.gen_x_cols(2001, system(name)[0], 3)))


def rhs(name, dtype, k=3):
    from basic_sparse_matrix_amd import Dense

    return Dense.from_columns([c.astype(dtype) for c in rhs_cols(name)[:k]])


def setup(monkeypatch, name):
    leaf = system(name)[4]
    if leaf is not None:
        monkeypatch.setenv("BSM_ND_LEAF", leaf)


def matrix(name, dtype, v=None):
    """A fresh Csr (a fresh device handle) of the pattern, with the system's values or v."""
    from basic_sparse_matrix_amd import Csr

    n, rp, ci, v0, _ = system(name)
    return Csr.from_csr_arrays((n, n), rp, ci, np.asarray(v0 if v is None else v).astype(dtype))


# ---- the mirrored matrix S and its backward error --------------------------------


def sym_dense(name, v):
    """S as the library defines it, dense f64: the stored entries with column <= row, mirrored."""
    n = system(name)[0]
    r, c = coords(name)
    low = np.zeros((n, n))
    keep = c <= r
    low[r[keep], c[keep]] = np.asarray(v, dtype=np.float64)[keep]
    return low + np.tril(low, -1).T


def default_tol(S):
    return (int((S != 0).sum(axis=1).max()) + 2) * 2.0 ** -53


def omega_np(S, x, b):
    """The backward error from a longdouble residual."""
    L = np.longdouble
    r = np.asarray(b, L) - np.asarray(S, L) @ np.asarray(x, L)
    return float(np.abs(r).max() / (np.abs(S).sum(axis=1).max() * np.abs(np.asarray(x, L)).max() + np.abs(b).max()))


# ---- restated pieces of the library's Krylov loops -------------------------------


def _scale(v):
    """The power of two a vector is divided by before it is rounded to the factor's dtype."""
    m = np.abs(v).max()
    return 2.0 ** np.floor(np.log2(m)) if m > 0 and np.isfinite(m) else 1.0


M64 = (1 << 64) - 1


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


@functools.lru_cache(maxsize=None)
def _start_block(n, block, seed):
    out = np.zeros((n, block))
    h0 = _mix64(seed ^ ((6 * 0xD1B54A32D192ED03) & M64))
    for r in range(n):
        hr = _mix64(h0 ^ r)
        for c in range(block):
            h = _mix64(hr ^ ((c * 0x9E3779B97F4A7C15) & M64))
            out[r, c] = 2.0 * ((0.5 + (h >> 11) * 2.0 ** -53) - 1.0)
    return _frozen(out)[0]


def start_block(n, block, seed=0, dtype=np.float64):
    """The eigensolvers' start block, restated: bsm_hash(seed, row, column, 6) mapped to [-1, 1)."""
    return _start_block(n, block, seed).astype(dtype)


# ---- the C-ABI ------------------------------------------------------------------


def assert_exported_and_bound(names):
    """The symbols are exported by the library and declared to ctypes; they are additions, so the API version is 1."""
    from basic_sparse_matrix_amd import _lib

    lib = _lib.load()
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for n in names:
        assert hasattr(lib, n), f"{n} not exported by libbsm_hip.so"
        assert n in bound, f"{n} not declared in _lib.SIGNATURES"
    assert lib.bsm_api_version() == 1
