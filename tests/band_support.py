"""Band systems that the solver tests share: symmetric positive definite
matrices of an exact bandwidth whose rows all differ, so that a kernel which
reads a neighbouring block, or swaps two blocks, changes the answer at once
(a Poisson stencil's factor tends to a stationary limit and forgives both).

The generators take an rng and return a dense symmetric float64 matrix; the
tests turn it into CSR with nd_support.csr_arrays. system() names one matrix
per (kind, n, b, fill), the same in every test file, and hands it out
read-only."""

import functools

import numpy as np


def _dominant_scaled(rng, low):
    """low: strict lower triangle. Symmetrise, diagonal = sum |offdiag| +
    U(0.5, 1.5) (strictly dominant, so SPD), then D A D with D log-uniform in
    [0.5, 2] per row: the scaling is what makes the rows differ."""
    n = low.shape[0]
    a = low + low.T
    a[np.arange(n), np.arange(n)] = np.abs(a).sum(axis=1) + rng.uniform(0.5, 1.5, n)
    d = np.exp2(rng.uniform(-1.0, 1.0, n))
    a = d[:, None] * a * d[None, :]
    return 0.5 * (a + a.T)  # (d_i a) d_j and (d_j a) d_i may round apart


def _values(rng, shape):
    """Uniform in (-1, 1) with |v| >= 0.05."""
    return rng.uniform(0.05, 1.0, shape) * rng.choice([-1.0, 1.0], shape)


def band_spd(rng, n, b, fill):
    """SPD of bandwidth exactly b: below the diagonal an entry at distance
    d = i - j <= b is present with probability fill, every entry at distance
    exactly b is present."""
    assert 0 <= b < max(n, 1)
    low = np.zeros((n, n))
    if b:
        i = np.arange(n)[:, None]
        d = np.arange(1, b + 1)[None, :]
        keep = ((rng.random((n, b)) < fill) | (d == b)) & (i - d >= 0)
        v = _values(rng, (n, b))
        ii, dd = np.nonzero(keep)
        low[ii, ii - dd - 1] = v[ii, dd]
    return _dominant_scaled(rng, low)


def spike_spd(rng, n, b):
    """Tridiagonal plus the single entry (r, r - b), r the row nearest n / 2
    that has a column r - b: one entry sets the bandwidth, so L holds exact
    zeros inside its band and its rows start at different columns."""
    assert 2 <= b < n
    low = np.zeros((n, n))
    low[np.arange(1, n), np.arange(n - 1)] = _values(rng, n - 1)
    r = max(b, n // 2)
    low[r, r - b] = _values(rng, ())
    return _dominant_scaled(rng, low)


def bandwidth(a):
    i, j = np.nonzero(a)
    return int(np.abs(i - j).max()) if i.size else 0


@functools.lru_cache(maxsize=4)  # the tests of one system follow one another; a session's worth would be gigabytes
def system(kind, n, b, fill=1.0):
    """The one "band" or "spike" matrix of these parameters, read-only."""
    rng = np.random.default_rng([{"band": 1, "spike": 2}[kind], n, b, int(round(fill * 100))])
    a = band_spd(rng, n, b, fill) if kind == "band" else spike_spd(rng, n, b)
    a.setflags(write=False)
    return a


def solve_longdouble(a, b, rhs):
    """a^-1 rhs in np.longdouble (rhs: (n, k)) for an SPD a of bandwidth <= b:
    a plain right-looking band Cholesky on a moving (b + 1)^2 window, then the
    two substitutions. The high-precision truth of the f64 tests."""
    ld = np.longdouble
    n, w = a.shape[0], b + 1
    lc = np.zeros((n, w), ld)  # lc[j, d] = L[j + d, j]
    win = np.zeros((w, w), ld)
    m = min(w, n)
    win[:m, :m] = a[:m, :m]
    for j in range(n):
        col = win[:, 0] / np.sqrt(win[0, 0])
        lc[j] = col
        nxt = np.zeros_like(win)
        nxt[:b, :b] = win[1:, 1:] - np.outer(col[1:], col[1:])
        r = j + w  # the row that enters the window: columns j + 1 .. r
        if r < n:
            nxt[b, :] = a[r, j + 1:r + 1]
            nxt[:, b] = a[j + 1:r + 1, r]
        win = nxt
    x = np.array(rhs, dtype=ld)
    for i in range(n):
        d = np.arange(1, min(b, i) + 1)
        x[i] = (x[i] - lc[i - d, d] @ x[i - d]) / lc[i, 0]
    for i in range(n - 1, -1, -1):
        d = np.arange(1, min(b, n - 1 - i) + 1)
        x[i] = (x[i] - lc[i, d] @ x[i + d]) / lc[i, 0]
    return x


# ---- reference order: every kernel-selection edge (test_gpu_solver_band_edges.py) ----

# band_walk_cfg (kernels_solve.hip:961-972), the (SEG, NL) of the band_backward_reg that launch_backward
# (kernels_solve.hip:2354-2372) starts: (largest bandwidth, SEG, NL)
BACKWARD_CFGS = ((64, 1, 64), (128, 2, 64), (256, 4, 64), (512, 8, 64), (768, 12, 64), (896, 16, 56), (1000, 40, 25),
                 (1024, 16, 64), (2048, 32, 64))
BAND_LIMIT = 64 * 17 - 16  # band_factor (kernels_solve.hip:1840): wider bands go to chol_general
FW3_NEAR = 192  # kernels_solve.hip:652; the forward selection is kernels_solve.hip:2406
# launch_chol5's slot counts M = 1, 2, 4, 8, 16, 17 by w4 = b + 15 <= 64 .. 1024 (kernels_solve.hip:1859-1865)
CHOL5_LAST = (49, 113, 241, 497, 1009)

EDGE_BANDWIDTHS = tuple(sorted(
    {0, 1, 2, 15, 16, 17}  # no band at all, and both sides of the 16-row tile (TR, C4_TB: kernels_solve.hip:44, 235)
    | {b + s for b in CHOL5_LAST for s in (0, 1)}
    | {b + s for b, _, _ in BACKWARD_CFGS[:-1] for s in (0, 1)}
    | {FW3_NEAR, FW3_NEAR + 1}
    | {BAND_LIMIT, BAND_LIMIT + 1}))
MANY_COLUMNS = {64: 17, 193: 17, 513: 17}  # k (1 + FW3_HELPERS) > 256: the one-workgroup forward solve on a wide band
SPIKE_BANDWIDTHS = (64, 128, 256, 512, 768, 896, 1000, 1024, BAND_LIMIT)  # one per backward configuration


def backward_cfg(b):
    return next((seg, nl) for top, seg, nl in BACKWARD_CFGS if b <= top)


def edge_rows(b):
    """No full row (n = b + 1), one (b + 2), past one 64-row block (b + 66),
    and 18 blocks of 64 plus one row: the forward solve's 8 waves and its two
    triangle buffers wrap, and an odd n ends on the lone row 0."""
    return (b + 1, b + 2, b + 66) + ((1153,) if b + 66 < 1153 else ())


def edge_fill(b):
    return 1.0 if b <= 128 else 0.5


def assert_edge_coverage():
    """The parametrisation's own check: every backward configuration,
    band_chol5 slot count and forward branch has a bandwidth on each side of
    its boundary, and between them the row counts of every backward
    configuration give both parities of n and of n - 1 - b (which branches of
    band_backward_reg's masked loop, full loop and lone row 0 run), with
    n = b + 1 and n = b + 2 among them, and it has its spike system."""
    bws = EDGE_BANDWIDTHS
    for last in tuple(top for top, _, _ in BACKWARD_CFGS[:-1]) + CHOL5_LAST + (FW3_NEAR, BAND_LIMIT):
        assert last in bws and last + 1 in bws, last
    assert {backward_cfg(b) for b in bws} == {(seg, nl) for _, seg, nl in BACKWARD_CFGS}
    for cfg in {backward_cfg(b) for b in bws}:
        rows = [(n, b) for b in bws if backward_cfg(b) == cfg and b <= BAND_LIMIT for n in edge_rows(b)]
        assert {n % 2 for n, _ in rows} == {0, 1} and {(n - 1 - b) % 2 for n, b in rows} == {0, 1}, cfg
        assert {n - b for n, b in rows} >= {1, 2, 66}, cfg
        assert any(backward_cfg(b) == cfg for b in SPIKE_BANDWIDTHS), cfg
    # the many-column forward branch: k (1 + FW3_HELPERS) > 256, below and above FW3_NEAR
    assert all(b in bws and k * 17 > 256 for b, k in MANY_COLUMNS.items())
    assert any(b > FW3_NEAR for b in MANY_COLUMNS) and any(b <= FW3_NEAR for b in MANY_COLUMNS)


# ---- blocked order (test_gpu_solver_blocked.py) ------------------------------------------

BLOCKED_PAIRS = ((1, 0), (2, 1), (63, 62), (64, 0), (64, 1), (64, 63), (65, 1), (65, 64), (127, 63), (128, 64),
                 (129, 65), (129, 128), (200, 15), (200, 16), (200, 17), (200, 127), (200, 129), (321, 64),
                 (321, 191), (321, 193), (450, 257))
BLOCKED_SPIKES = ((200, 65), (321, 129))
BLOCKED_TICKETS = (4096, 70)  # more (block, column) tickets than any grid holds, with k = 64


def blocked_fill(b):
    return 1.0 if b < 100 else 0.6


def blocked_systems():
    """(kind, n, b, fill) of every blocked-order system but the ticket case."""
    return tuple(("band", n, b, blocked_fill(b)) for n, b in BLOCKED_PAIRS) + \
        tuple(("spike", n, b, 1.0) for n, b in BLOCKED_SPIKES)


def edge_systems():
    """(kind, n, b, fill) of every reference-order system."""
    return tuple(("band", n, b, edge_fill(b)) for b in EDGE_BANDWIDTHS for n in edge_rows(b)) + \
        tuple(("spike", n, b, 1.0) for b in SPIKE_BANDWIDTHS for n in spike_rows(b))


def spike_rows(b):
    return (b + 66,) + ((1153,) if b <= 512 else ())
