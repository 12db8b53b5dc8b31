"""The kept nd factor's solve with sparse right-hand sides and selected rows
(NdFactor.solve_sparse / inv_block, device.nd_factor_solve_sparse,
bsm_nd_factor_solve_sparse): only the fronts on the paths from
b's entries to the root run the forward pass, only those from the requested
rows' fronts the backward pass, each with the dense solve's operations in its
order. So the contract is EQUALITY with f.solve on the densified b
(np.array_equal: a zero's sign is the one thing a skipped front can change);
nothing here has a tolerance.

The systems are nd_support.dense_system's with their BSM_ND_LEAF:
  g5-leaf1     one pivot beside 63 padding pivots; a path over every level
  g11-leaf8    two entries of one column in different leaves that meet at an
               ancestor; an entry that starts in a separator; a requested row
               in a leaf the forward pass never visits (y = 0, x != 0)
  g40-leaf256  several pivot tiles per front; an entry and a requested row in
               a leaf's second tile
  blocks       fronts with np = 0 on the path; b in one component (the second
               grid) and rows asked for in the other: exact zeros come back
b (columns(), below) is chosen through the permutation: column 0 has an entry at
the first vertex of the deepest leaf A, one in another leaf B and (where a
leaf has more than 64 pivots) one in a leaf's second pivot tile, A's if it can
be; with k = 3 column 1 is EMPTY and column 2 has an entry in a separator and
one in leaf A (the same path as column 0); k = 33 (past one chunk of 32) adds 30 seeded columns of one or two
entries. The values are multiples of 1/4 (f32 holds them), none is -0. The
rows asked for (rows_of()) are unsorted and repeat: a vertex of a leaf no entry
of b lies in, A's second tile, a separator, the last vertex of the new order
(the root's, where it has pivots), and a few seeded ones."""

import functools

import numpy as np
import pytest

from basic_sparse_matrix_amd import Csr, Dense, MatErr, MatErrKind, _lib, cholesky_nd
from basic_sparse_matrix_amd.solver import nd_analyse
from nd_support import csr_arrays, dense_matrix, dense_setup, dense_system, same_bits

gpu = pytest.mark.gpu

SYSTEMS = ("g5-leaf1", "g11-leaf8", "g40-leaf256", "blocks")
KS = (1, 3, 33)
# (the matrix's dtype, the factor's)
DTYPES = [(np.float64, np.float64), (np.float64, np.float32), (np.float32, np.float32)]
CASES = [(s, k, d) for s in SYSTEMS for k in KS for d in DTYPES]
CASE_IDS = [f"{s}-k{k}-{np.dtype(d[0]).name}-factor-{np.dtype(d[1]).name}" for s, k, d in CASES]
FEW = [("g5-leaf1", 3, DTYPES[2]), ("g11-leaf8", 33, DTYPES[0]), ("g40-leaf256", 3, DTYPES[1]),
       ("blocks", 33, DTYPES[0])]
FEW_IDS = [f"{s}-k{k}-{np.dtype(d[0]).name}-factor-{np.dtype(d[1]).name}" for s, k, d in FEW]


@functools.lru_cache(maxsize=None)
def _tree(name):
    n, s, leaf, _ = dense_system(name)
    rp, ci, _ = csr_arrays(s)
    t = nd_analyse(n, rp, ci, leaf=leaf)
    owner = np.zeros(n, dtype=np.int64)  # by NEW index
    for i, (a, b) in enumerate(zip(t["start"], t["end"])):
        owner[a:b] = i
    t["owner"] = owner
    pinv = np.empty(n, dtype=np.int64)
    pinv[t["perm"]] = np.arange(n)
    t["pinv"] = pinv
    return t


def path(name, node):
    t = _tree(name)
    out = []
    while node >= 0:
        out.append(int(node))
        node = t["parent"][node]
    return out


def reach(name, vertices):
    """The union of the paths from the fronts owning `vertices` (A's order) to their roots."""
    t = _tree(name)
    out = set()
    for v in vertices:
        out.update(path(name, t["owner"][t["pinv"][int(v)]]))
    return out


@functools.lru_cache(maxsize=None)
def _places(name):
    """The vertices (A's order) the docstring names, from the host analysis."""
    n, s, _, _ = dense_system(name)
    t = _tree(name)
    perm, start, end, level = t["perm"], t["start"], t["end"], t["level"]
    leaves = [i for i in range(len(start)) if level[i] == 0 and end[i] > start[i]]
    if name == "blocks":  # b stays in the second component (vertices 144 .. 287): its paths cross the empty front
        leaves = [i for i in leaves if 144 <= perm[start[i]] < 288]
    a = min(leaves, key=lambda i: (-len(path(name, i)), int(start[i])))  # the deepest leaf
    b = next(i for i in leaves if i != a and set(path(name, a)) & set(path(name, i)))
    seps = [i for i in range(len(start)) if level[i] > 0 and end[i] > start[i]
            and (name != "blocks" or 144 <= perm[start[i]] < 288)]
    sep = min(seps, key=lambda i: (level[i], i))
    # the leaf whose second pivot tile is used: A where it has one, else the largest leaf
    tl = a if end[a] - start[a] > 68 else max(leaves, key=lambda i: (int(end[i] - start[i]), -i))
    out = {"a": int(perm[start[a]]), "b": int(perm[start[b]]), "sep": int(perm[start[sep]]),
           "a_next": int(perm[start[a] + 1]) if end[a] - start[a] > 1 else int(perm[start[a]]),
           "a_tile2": int(perm[start[tl] + 64 + 3]) if end[tl] - start[tl] > 68 else None,
           "last": int(perm[n - 1]), "leaf_a": a, "leaf_b": b, "leaf_t": tl, "sep_node": sep}
    # a leaf that neither column 0 nor column 2 visits
    busy = reach(name, [v for v in (out["a"], out["b"], out["sep"], out["a_tile2"]) if v is not None])
    other = [i for i in range(len(start)) if level[i] == 0 and end[i] > start[i] and i not in busy]
    out["unvisited"] = int(perm[start[other[-1]]]) if other else None
    out["unvisited_node"] = other[-1] if other else None
    return out


@functools.lru_cache(maxsize=None)
def columns(name, k):
    """b (n x k, f64 values that f32 holds exactly, no -0). Never modified."""
    n = dense_system(name)[0]
    p = _places(name)
    rng = np.random.default_rng(7 + k)

    def val():
        return float(rng.choice([-1.0, 1.0]) * rng.integers(1, 9) / 4.0)

    b = np.zeros((n, k))
    b[p["a"], 0] = 1.0
    b[p["b"], 0] = val()
    if p["a_tile2"] is not None:
        b[p["a_tile2"], 0] = val()
    if k >= 3:  # column 1 stays empty
        b[p["sep"], 2] = val()
        b[p["a_next"], 2] = val()
    lo, hi = (144, 288) if name == "blocks" else (0, n)
    for c in range(3, k):
        for v in lo + rng.choice(hi - lo, size=1 + c % 2, replace=False):
            b[v, c] = val()
    assert not np.signbit(b[b == 0]).any() and np.array_equal(b, b.astype(np.float32).astype(np.float64))
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def rows_of(name):
    """The rows asked for: unsorted, with repeats."""
    n = dense_system(name)[0]
    p = _places(name)
    rng = np.random.default_rng(11)
    r = [p["last"], p["sep"], p["a"]]
    r += [p[x] for x in ("unvisited", "a_tile2") if p[x] is not None]
    r += [int(v) for v in rng.choice(n, size=4, replace=False)]
    r += [p["last"], r[3]]
    out = np.array(r, dtype=np.int64)
    out.setflags(write=False)
    return out


def b_csr(b, dtype):
    rp, ci, v = csr_arrays(b)
    return Csr.from_csr_arrays(b.shape, rp, ci, v.astype(dtype))


def arr(d):
    """A Dense as an array (rows x cols)."""
    dims = d.get_dims()
    if dims.cols == 0:
        return np.zeros((dims.rows, 0))
    return np.stack([np.asarray(d.get_col(j)) for j in range(dims.cols)], axis=1)


def dense_solve(f, b):
    """f.solve of the densified b, as an array."""
    b = np.asarray(b, dtype=f.dtype)
    return arr(f.solve(Dense.from_columns([np.ascontiguousarray(b[:, j]) for j in range(b.shape[1])])))


# ---- no GPU: the structure each system is here for -----------------------------


def test_the_entries_and_rows_are_where_the_docstring_says():
    t = _tree("g5-leaf1")
    assert ((t["end"] - t["start"])[t["level"] == 0] == 1).all()  # one real pivot per leaf front
    assert len(path("g5-leaf1", _places("g5-leaf1")["leaf_a"])) == t["level"].max() + 1  # across every level
    p, t = _places("g11-leaf8"), _tree("g11-leaf8")
    assert p["leaf_a"] != p["leaf_b"] and t["level"][p["leaf_a"]] == 0 and t["level"][p["leaf_b"]] == 0
    assert set(path("g11-leaf8", p["leaf_a"])) & set(path("g11-leaf8", p["leaf_b"]))  # that meet
    assert t["level"][p["sep_node"]] > 0  # an entry that starts in a separator
    visited = reach("g11-leaf8", np.nonzero(columns("g11-leaf8", 3).any(axis=1))[0])
    assert p["unvisited_node"] is not None and p["unvisited_node"] not in visited  # y = 0 there, x is not
    assert p["unvisited"] in rows_of("g11-leaf8")
    p, t = _places("g40-leaf256"), _tree("g40-leaf256")
    assert (t["end"] - t["start"]).max() > 128  # leaves of more than two pivot tiles
    q = t["pinv"][p["a_tile2"]]
    assert 64 <= q - t["start"][p["leaf_t"]] < 128 and t["owner"][q] == p["leaf_t"]  # a leaf's second tile
    assert columns("g40-leaf256", 1)[p["a_tile2"], 0] != 0 and p["a_tile2"] in rows_of("g40-leaf256")
    p, t = _places("blocks"), _tree("blocks")
    on_path = reach("blocks", [p["a"]])
    assert any(t["start"][x] == t["end"][x] for x in on_path)  # fronts with np == 0 on the path
    used = np.nonzero(columns("blocks", 33).any(axis=1))[0]
    assert (used >= 144).all() and (used < 288).all()  # b in the second component alone
    for name in SYSTEMS:
        b = columns(name, 33)
        assert not b[:, 1].any() and b[:, 0].any()  # an empty column
        a = _places(name)["leaf_a"]  # two columns on the same path
        assert a in reach(name, np.nonzero(b[:, 0])[0]) and a in reach(name, np.nonzero(b[:, 2])[0])
        r = rows_of(name)
        assert len(set(r.tolist())) < len(r) and (np.diff(r) < 0).any()  # repeated, unsorted


# ---- on the GPU -----------------------------------------------------------------


@gpu
@pytest.mark.parametrize("name,k,dtypes", CASES, ids=CASE_IDS)
def test_equality(monkeypatch, name, k, dtypes):
    """1 (equality, host and device, inv_block) and 3a (the counts are the unions of paths)."""
    from basic_sparse_matrix_amd import device

    dense_setup(monkeypatch, name)
    src, fdt = dtypes
    n, s, _, _ = dense_system(name)
    t = _tree(name)
    b, rows = columns(name, k), rows_of(name)
    bc = b_csr(b, fdt)
    with cholesky_nd(dense_matrix(s, src), factor_dtype=fdt) as f:
        assert np.array_equal(f.perm, t["perm"])  # the entries were chosen through this permutation
        want = dense_solve(f, b)
        assert want.dtype == np.dtype(fdt) and np.isfinite(want).all()
        x, info = f.solve_sparse(bc, rows, info=True)
        assert x.dtype == np.dtype(fdt)
        got = arr(x)
        assert got.shape == (len(rows), k)
        assert np.array_equal(got, want[rows])
        nodes = len(t["start"])
        entries = np.nonzero(b.any(axis=1))[0]
        print("info", info, "of", nodes)
        assert info == (len(reach(name, entries)), len(reach(name, rows)), nodes, (k + 31) // 32)
        # it really skips: the rows' paths never cover the tree, nor do those of up to three columns (33
        # seeded columns may reach every leaf of a small tree: the count above is then the whole tree)
        assert info[1] < nodes and (k > 3 or info[0] < nodes)
        # every row
        xa, info_all = f.solve_sparse(bc, info=True)
        assert np.array_equal(arr(xa), want)
        assert info_all == (info[0], nodes, nodes, info[3])
        # sorted and unique rows; one row
        u = np.unique(rows)
        assert np.array_equal(arr(f.solve_sparse(bc, u)), want[u])
        assert np.array_equal(arr(f.solve_sparse(bc, rows[3:4])), want[rows[3:4]])
        # inv_block against the solves of unit columns
        cols = np.concatenate([entries[:3], rows[:2]])
        unit = np.zeros((n, len(cols)))
        unit[cols, np.arange(len(cols))] = 1.0
        z = f.inv_block(rows, cols)
        assert z.dtype == np.dtype(fdt) and np.array_equal(z, dense_solve(f, unit)[rows])
        # the device call against the host call
        xd = device.nd_factor_solve_sparse(f, bc, rows).cpu().numpy()
        assert same_bits(xd, got)
        xd = device.nd_factor_solve_sparse(f, bc).cpu().numpy()
        assert same_bits(xd, arr(xa))
        if name == "blocks":  # b in one component, rows in the other: exact zeros
            far = np.array([143, 0, 77, 290])
            z = arr(f.solve_sparse(bc, far))
            assert np.array_equal(z, np.zeros((4, k))) and np.array_equal(want[far], np.zeros((4, k)))


@gpu
@pytest.mark.parametrize("name,k,dtypes", FEW, ids=FEW_IDS)
def test_independence(monkeypatch, name, k, dtypes):
    """2: a value depends neither on the other rows asked for nor on the call's other columns, and repeats."""
    dense_setup(monkeypatch, name)
    src, fdt = dtypes
    s = dense_system(name)[1]
    b, rows = columns(name, k), rows_of(name)
    with cholesky_nd(dense_matrix(s, src), factor_dtype=fdt) as f:
        base = arr(f.solve_sparse(b_csr(b, fdt), rows))
        assert same_bits(arr(f.solve_sparse(b_csr(b, fdt), rows)), base)
        full = arr(f.solve_sparse(b_csr(b, fdt)))
        for j in sorted({0, 2 % k, k - 1}):
            one = b_csr(b[:, j:j + 1], fdt)
            for e in (0, 3, len(rows) - 1):
                got = arr(f.solve_sparse(one, rows[e:e + 1]))
                assert same_bits(got, base[e:e + 1, j:j + 1]), (j, e)
                # with every row: the dense backward levels instead of the path's
                assert np.array_equal(full[rows[e], j], got[0, 0])
            assert same_bits(arr(f.solve_sparse(one, rows)), base[:, j:j + 1]), j


@gpu
@pytest.mark.parametrize("name,k,dtypes", FEW, ids=FEW_IDS)
def test_nothing_undefined_is_read(monkeypatch, name, k, dtypes):
    """3b: BSM_ND_POISON=1 -- every temporary starts as NaN; the results are finite and unchanged."""
    from basic_sparse_matrix_amd import device

    dense_setup(monkeypatch, name)
    src, fdt = dtypes
    s = dense_system(name)[1]
    b, rows = columns(name, k), rows_of(name)
    cols = np.nonzero(b.any(axis=1))[0][:3]

    def run():
        with cholesky_nd(dense_matrix(s, src), factor_dtype=fdt) as f:
            bc = b_csr(b, fdt)
            return [arr(f.solve_sparse(bc, rows)), arr(f.solve_sparse(bc)), f.inv_block(rows, cols),
                    device.nd_factor_solve_sparse(f, bc, rows).cpu().numpy()]

    base = run()
    monkeypatch.setenv("BSM_ND_POISON", "1")
    got = run()
    for g, w in zip(got, base):
        assert np.isfinite(g).all()
        assert same_bits(g, w)


@gpu
@pytest.mark.parametrize("name,k,dtypes", FEW, ids=FEW_IDS)
def test_it_sees_the_current_factor(monkeypatch, name, k, dtypes):
    """4: after refactor(a2) and after update(w), equality with f.solve still holds."""
    dense_setup(monkeypatch, name)
    src, fdt = dtypes
    n, s, _, _ = dense_system(name)
    b, rows = columns(name, k), rows_of(name)
    bc = b_csr(b, fdt)
    with cholesky_nd(dense_matrix(s, src), factor_dtype=fdt) as f:
        x0 = arr(f.solve_sparse(bc, rows))
        f.refactor(dense_matrix(1.5 * s, src))
        want = dense_solve(f, b)
        x1 = arr(f.solve_sparse(bc, rows))
        assert np.array_equal(x1, want[rows]) and not np.array_equal(x1, x0)
        w = np.zeros((n, 1))
        w[_places(name)["a"], 0] = 0.5  # a diagonal column: always inside the pattern
        f.update(b_csr(w, src))
        want = dense_solve(f, b)
        x2 = arr(f.solve_sparse(bc, rows))
        assert np.array_equal(x2, want[rows]) and not np.array_equal(x2, x1)
        assert np.array_equal(arr(f.solve_sparse(bc)), want)


@gpu
def test_refusals_leave_the_outputs_untouched(monkeypatch):
    """5: every refusal of bsm.h, through the C-ABI with the outputs prefilled, host and device."""
    import torch

    name, (src, fdt) = "g11-leaf8", DTYPES[0]
    dense_setup(monkeypatch, name)
    n, s, _, _ = dense_system(name)
    lib = _lib.require_device()
    cp = np.array([0, 2, 2, 3], dtype=np.uint64)
    br = np.array([3, 77, 5], dtype=np.uint64)
    bv = np.array([1.0, -0.5, 2.0])
    xr = np.array([100, 0, 0], dtype=np.uint64)
    sentinel = -77.25
    xs = [np.full(3, sentinel) for _ in range(3)]
    xt = torch.full((3, 3), sentinel, dtype=torch.float64, device="cuda")
    info = np.full(4, 9, dtype=np.uint32)

    def host(h, k=3, c=cp, r=br, v=bv, nq=3, q=xr, x=True):
        return lib.bsm_nd_factor_solve_sparse(h, k, _lib.ptr(c) if c is not None else None,
                                              _lib.ptr(r) if r is not None else None,
                                              _lib.ptr(v) if v is not None else None, nq,
                                              _lib.ptr(q) if q is not None else None,
                                              _lib.ptr_array(xs) if x else None, _lib.ptr(info))

    def dev(h, k=3, c=cp, r=br, v=bv, nq=3, q=xr, x=True):
        return lib.bsm_dev_nd_factor_solve_sparse(h, k, _lib.ptr(c) if c is not None else None,
                                                  _lib.ptr(r) if r is not None else None,
                                                  _lib.ptr(v) if v is not None else None, nq,
                                                  _lib.ptr(q) if q is not None else None,
                                                  xt.data_ptr() if x else None, _lib.ptr(info),
                                                  torch.cuda.current_stream().cuda_stream)

    def untouched():
        return (all(np.array_equal(x, np.full(3, sentinel)) for x in xs) and np.array_equal(info, [9, 9, 9, 9])
                and bool((xt == sentinel).all()))

    u64 = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    with cholesky_nd(dense_matrix(s, src)) as f:
        h = f.handle
        for call in (host, dev):
            inv, oob = _lib.BSM_ERR_INVALID, _lib.BSM_ERR_OUT_OF_BOUNDS
            for rc, what in ((call(None), "null"), (call(h, c=None), "null"), (call(h, r=None), "null"),
                             (call(h, v=None), "null"), (call(h, x=False), "null")):
                assert rc == inv and what in _lib.last_error()
            assert call(h, c=u64(1, 2, 2, 3)) == inv and "col_ptr[0]" in _lib.last_error()
            assert call(h, c=u64(0, 2, 1, 3)) == inv and "not ascending" in _lib.last_error()
            assert call(h, r=u64(77, 3, 5)) == inv and "strictly ascending" in _lib.last_error()
            assert call(h, r=u64(3, 3, 5)) == inv and "strictly ascending" in _lib.last_error()
            assert call(h, q=None) == inv and "xrows is null" in _lib.last_error()
            assert call(h, r=u64(3, n, 5)) == oob and f"row {n}" in _lib.last_error()
            assert call(h, q=u64(100, n, 0)) == oob and f"row {n}" in _lib.last_error()
            assert untouched(), call.__name__
            if torch.cuda.device_count() > 1:  # a factor is used on the device it was made on
                torch.cuda.set_device(1)
                try:
                    assert call(h) == inv and "device" in _lib.last_error()
                finally:
                    torch.cuda.set_device(0)
                assert untouched()
        # the Python mirror
        bc = Csr.from_csr_arrays((n, 1), np.arange(n + 1, dtype=np.uint64).clip(0, 1), np.zeros(1, dtype=np.uint64),
                                 np.ones(1))
        with pytest.raises(MatErr) as me:
            f.solve_sparse(bc, [0, n])
        assert me.value.kind == MatErrKind.OutOfBounds
        with pytest.raises(MatErr) as me:
            f.inv_block([0], [n])
        assert me.value.kind == MatErrKind.OutOfBounds
        with pytest.raises(TypeError):
            f.solve_sparse(Csr.from_csr_arrays((n, 1), np.arange(n + 1, dtype=np.uint64).clip(0, 1),
                                               np.zeros(1, dtype=np.uint64), np.ones(1, dtype=np.float32)))
        # the call as it stands is fine, and fills everything
        assert host(h) == _lib.BSM_OK and dev(h) == _lib.BSM_OK
        assert not any((x == sentinel).any() for x in xs) and not bool((xt == sentinel).any())
        assert same_bits(np.stack(xs, axis=1), xt.cpu().numpy())
        assert info[2] == len(_tree(name)["start"]) and info[3] == 1
        for x in xs:
            x[:] = sentinel
        xt.fill_(sentinel)
        info[:] = 9
        # no-ops: no columns; no rows (a non-null xrows with nq == 0)
        assert host(h, k=0) == _lib.BSM_OK and dev(h, k=0) == _lib.BSM_OK
        assert untouched()
        assert host(h, nq=0) == _lib.BSM_OK and np.array_equal(info, [0, 0, 0, 0])
        info[:] = 9
        assert dev(h, nq=0) == _lib.BSM_OK and np.array_equal(info, [0, 0, 0, 0])
        info[:] = 9
        assert untouched()
        # a handle without values refuses, as the solves do
        bad = s.copy()
        bad[n // 2, n // 2] = -bad[n // 2, n // 2]
        with pytest.raises(_lib.BsmError, match="positive definite"):
            f.refactor(dense_matrix(bad, src))
        for call in (host, dev):
            assert call(h) == _lib.BSM_ERR_INVALID and "refactor first" in _lib.last_error()
        assert untouched()
        f.refactor(dense_matrix(s, src))
        assert host(h) == _lib.BSM_OK
        want = dense_solve(f, _dense_of(cp, br, bv, n))
        assert np.array_equal(np.stack(xs, axis=1), want[xr.astype(np.int64)])


def _dense_of(cp, rows, vals, n):
    out = np.zeros((n, len(cp) - 1))
    for c in range(len(cp) - 1):
        for e in range(int(cp[c]), int(cp[c + 1])):
            out[int(rows[e]), c] = vals[e]
    return out
