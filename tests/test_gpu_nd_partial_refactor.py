"""The kept nd factor's partial refactor (NdFactor.refactor_partial,
bsm_nd_factor_refactor_partial / _since): new values at a few
places of the factored pattern, and only the fronts on the paths from those
entries to the roots factored again, by refactor's kernel on refactor's inputs
in refactor's order. So the contract is EQUALITY with a fresh cholesky_nd of
the new matrix (same_bits / np.array_equal on l(), solve, logdet, inv_diag);
nothing here has a tolerance but eigsh's own residual test.

The systems and their BSM_ND_LEAF are nd_support.dense_system's; the places
(through the permutation from nd_analyse) are test_gpu_nd_sparse_solve.py's.
A changed diagonal entry grows by a multiple of 1/4 and a changed edge shrinks
to 3/4 of its value (both triangles, though the upper one is never read), so
every new matrix stays diagonally dominant, hence SPD, and f32 holds its
values."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from basic_sparse_matrix_amd import Csr, Dense, MatErr, MatErrKind, _lib, cholesky_nd
from nd_support import assert_same, dense_matrix, dense_setup, dense_system
# the places through nd_analyse's tree, and the cases, are the sparse solve's
from test_gpu_nd_sparse_solve import DTYPES, SYSTEMS, _places, _tree, arr, b_csr, path, reach

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(s, d) for s in SYSTEMS for d in DTYPES]
CASE_IDS = [f"{s}-{np.dtype(d[0]).name}-factor-{np.dtype(d[1]).name}" for s, d in CASES]
FEW = [("g5-leaf1", DTYPES[2]), ("g11-leaf8", DTYPES[0]), ("g40-leaf256", DTYPES[1]), ("blocks", DTYPES[0])]
FEW_IDS = [f"{s}-{np.dtype(d[0]).name}-factor-{np.dtype(d[1]).name}" for s, d in FEW]


def _leaf_edge(name, leaf):
    """A stored off-diagonal (i, j) with both ends among `leaf`'s own vertices, or None."""
    s, t = dense_system(name)[1], _tree(name)
    vs = [int(v) for v in t["perm"][t["start"][leaf]:t["end"][leaf]]]
    for i in vs:
        for j in vs:
            if j < i and s[i, j] != 0:
                return (i, j)
    return None


@functools.lru_cache(maxsize=None)
def groups(name):
    """name -> the list of (i, j) positions (A's order) of each case the module's tests walk."""
    n, s, _, _ = dense_system(name)
    t, p = _tree(name), _places(name)
    pinv = t["pinv"]
    out = {"leaf-diagonal": [(p["a"], p["a"])], "root": [(p["last"], p["last"])]}
    e = _leaf_edge(name, p["leaf_a"]) or _leaf_edge(name, p["leaf_t"])
    if e:
        out["leaf-edge"] = [e]
    # the smaller new index in a separator: an edge to a later vertex where the separator's first vertex has one
    later = [int(w) for w in np.nonzero(s[p["sep"]])[0] if pinv[w] > pinv[p["sep"]]]
    out["separator"] = [(later[0], p["sep"])] if later else [(p["sep"], p["sep"])]
    if p["a_tile2"] is not None:
        out["second-tile"] = [(p["a_tile2"], p["a_tile2"])]
    out["two-leaves"] = [(p["a"], p["a"]), (p["b"], p["b"])]
    rng = np.random.default_rng(17)
    lo_r, lo_c = np.nonzero(np.tril(s) != 0)
    if name == "blocks":  # one component only (the second grid): the other one's fronts stay out
        keep = (lo_r >= 144) & (lo_r < 288)
        lo_r, lo_c = lo_r[keep], lo_c[keep]
    pick = rng.choice(lo_r.shape[0], size=17, replace=False)
    out["seeded-17"] = [(int(lo_r[q]), int(lo_c[q])) for q in pick]
    ar, ac = np.nonzero(np.tril(s) != 0)
    out["every-entry"] = [(int(i), int(j)) for i, j in zip(ar, ac)]
    out["swapped"] = [(j, i) for i, j in out["seeded-17"][:5]]
    out["repeats"] = out["two-leaves"] + out["two-leaves"][::-1] + out["separator"] + out["two-leaves"][:1]
    return out


def changed(s, pairs):
    """s with new values at the pairs (each place once, whatever the list repeats)."""
    s2 = np.array(s)
    for i, j in {(max(i, j), min(i, j)) for i, j in pairs}:
        if i == j:
            s2[i, i] = s[i, i] + 0.25 * (1 + (i % 4))
        else:
            s2[i, j] = s2[j, i] = 0.75 * s[i, j]
    assert np.array_equal(s2, s2.astype(np.float32).astype(np.float64))
    return s2


def start_vertices(name, pairs):
    """Per pair the vertex that comes first in the new order: its front is where the entry lands."""
    pinv = _tree(name)["pinv"]
    return [i if pinv[i] < pinv[j] else j for i, j in pairs]


def rc(pairs):
    return [i for i, _ in pairs], [j for _, j in pairs]


def rhs(name, dtype):
    n = dense_system(name)[0]
    b = (np.arange(n) % 7 - 3.0) / 4.0
    return np.ascontiguousarray(b.astype(dtype))


def bits(f, name):
    """Everything the issue compares: l() (row_ptr, col, vals), solve(b), logdet(), inv_diag()."""
    rp, ci, v = f.l()._csr_arrays()
    x = f.solve(Dense.from_columns([rhs(name, f.dtype)]))
    return [np.asarray(rp), np.asarray(ci), np.asarray(v), np.asarray(x.get_col(0)), np.array([f.logdet()]),
            np.asarray(f.inv_diag())]


def fresh_bits(s, name, src, fdt):
    with cholesky_nd(dense_matrix(s, src), factor_dtype=fdt) as g:
        return bits(g, name)


# ---- no GPU: the places are where the docstring says -----------------------------


def test_the_groups_start_where_they_should():
    t, p, g = _tree("g11-leaf8"), _places("g11-leaf8"), groups("g11-leaf8")
    assert reach("g11-leaf8", start_vertices("g11-leaf8", g["leaf-edge"])) == set(path("g11-leaf8", p["leaf_a"]))
    assert t["level"][t["owner"][t["pinv"][start_vertices("g11-leaf8", g["separator"])[0]]]] > 0
    assert len(reach("g11-leaf8", start_vertices("g11-leaf8", g["every-entry"]))) == len(t["start"])
    assert "second-tile" in groups("g40-leaf256")
    tb = _tree("blocks")
    assert len(reach("blocks", start_vertices("blocks", groups("blocks")["seeded-17"]))) < len(tb["start"])
    n, s, _, _ = dense_system("g40-leaf256")
    s2 = changed(s, groups("g40-leaf256")["every-entry"])
    assert (np.abs(s2).sum(axis=1) - 2 * np.diag(s2) <= 0).all()  # still diagonally dominant


# ---- 1, 2: equality and the front counts ------------------------------------------


@gpu
@pytest.mark.parametrize("name,dt", CASES, ids=CASE_IDS)
def test_partial_equals_a_fresh_factor(monkeypatch, name, dt):
    dense_setup(monkeypatch, name)
    src, fdt = dt
    n, s, _, _ = dense_system(name)
    t = _tree(name)
    base0 = fresh_bits(s, name, src, fdt)
    with cholesky_nd(dense_matrix(s, src), factor_dtype=fdt) as f:
        for gname, pairs in groups(name).items():
            s2 = changed(s, pairs)
            rows, cols = rc(pairs)
            info = f.refactor_partial(dense_matrix(s2, src), rows, cols)
            want = len(reach(name, start_vertices(name, pairs)))
            assert (info.fronts, info.total_fronts, info.changed) == (want, len(t["start"]), len(pairs)), gname
            if gname == "every-entry":
                assert info.fronts == info.total_fronts
            assert_same(bits(f, name), fresh_bits(s2, name, src, fdt), gname)
            # and back: the same places named, the first matrix's values
            info = f.refactor_partial(dense_matrix(s, src), rows, cols)
            assert info.fronts == want
            assert_same(bits(f, name), base0, gname + " (back)")


@gpu
def test_blocks_other_component_is_not_counted(monkeypatch):
    dense_setup(monkeypatch, "blocks")
    n, s, _, _ = dense_system("blocks")
    t = _tree("blocks")
    pairs = groups("blocks")["seeded-17"]
    first = {int(x) for x in range(len(t["start"])) if t["end"][x] > t["start"][x]
             and t["perm"][t["start"][x]] < 144}  # fronts with a vertex of the first grid
    with cholesky_nd(dense_matrix(s, np.float64)) as f:
        info = f.refactor_partial(dense_matrix(changed(s, pairs), np.float64), *rc(pairs))
    active = reach("blocks", start_vertices("blocks", pairs))
    assert info.fronts == len(active) and not (active & first) and info.fronts < info.total_fronts


# ---- 3: only the named paths are re-run ---------------------------------------------


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=[f"{np.dtype(a).name}-factor-{np.dtype(b).name}" for a, b in DTYPES])
def test_only_the_named_paths_are_rerun(monkeypatch, dt):
    name = "g11-leaf8"
    dense_setup(monkeypatch, name)
    src, fdt = dt
    n, s, _, _ = dense_system(name)
    p = _places(name)
    ea, eb = (p["a"], p["a"]), (p["b"], p["b"])
    s2, s3 = changed(s, [ea, eb]), changed(s, [ea])
    with cholesky_nd(dense_matrix(s, src), factor_dtype=fdt) as f:
        f.refactor_partial(dense_matrix(s2, src), [ea[0]], [ea[1]])  # b's entry changed too, but is not named
        assert_same(bits(f, name), fresh_bits(s3, name, src, fdt), "a alone")
        f.refactor_partial(dense_matrix(s2, src), [eb[0]], [eb[1]])
        assert_same(bits(f, name), fresh_bits(s2, name, src, fdt), "then b")


# ---- 4: since= ----------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("name,dt", CASES, ids=CASE_IDS)
def test_since_finds_the_places(monkeypatch, name, dt):
    dense_setup(monkeypatch, name)
    src, fdt = dt
    n, s, _, _ = dense_system(name)
    t = _tree(name)
    a0 = dense_matrix(s, src)
    with cholesky_nd(a0, factor_dtype=fdt) as f:
        base0 = bits(f, name)
        for gname in ("two-leaves", "seeded-17", "every-entry"):
            pairs = groups(name)[gname]
            s2 = changed(s, pairs)
            a2 = dense_matrix(s2, src)
            info = f.refactor_partial(a2, since=a0)
            assert info.changed == int((np.tril(s2) != np.tril(s)).sum()) == len(set(pairs)), gname
            assert info.fronts == len(reach(name, start_vertices(name, pairs))) and info.total_fronts == len(t["start"])
            assert_same(bits(f, name), fresh_bits(s2, name, src, fdt), gname)
            assert f.refactor_partial(a0, since=a2).changed == info.changed
            assert_same(bits(f, name), base0, gname + " (back)")
        # a difference above the diagonal alone; the matrix itself
        i, j = next((i, j) for i, j in groups(name)["every-entry"] if i > j)
        up = np.array(s)
        up[j, i] = 0.5 * s[i, j]
        for other in (dense_matrix(up, src), a0):
            info = f.refactor_partial(other, since=a0)
            assert (info.fronts, info.changed) == (0, 0)
            assert_same(bits(f, name), base0, "no differing entry")


# ---- 5: sequences -----------------------------------------------------------------


@gpu
@pytest.mark.parametrize("name,dt", FEW, ids=FEW_IDS)
def test_sequences(monkeypatch, name, dt):
    dense_setup(monkeypatch, name)
    src, fdt = dt
    n, s, _, _ = dense_system(name)
    g = groups(name)
    s1 = changed(s, g["two-leaves"])
    s2 = changed(s1, g["separator"] + g["root"])
    s3 = changed(changed(s, g["every-entry"]), g["leaf-diagonal"])
    with cholesky_nd(dense_matrix(s, src), factor_dtype=fdt) as f:
        f.refactor_partial(dense_matrix(s1, src), *rc(g["two-leaves"]))
        f.refactor_partial(dense_matrix(s2, src), *rc(g["separator"] + g["root"]))  # partial after partial
        want = fresh_bits(s2, name, src, fdt)
        assert_same(bits(f, name), want, "partial after partial")
        f.refactor_partial(dense_matrix(s2, src), *rc(g["separator"] + g["root"]))  # a repeat
        assert_same(bits(f, name), want, "repeat")
        f.refactor(dense_matrix(changed(s, g["every-entry"]), src))
        f.refactor_partial(dense_matrix(s3, src), *rc(g["leaf-diagonal"]))  # partial after refactor
        assert_same(bits(f, name), fresh_bits(s3, name, src, fdt), "partial after refactor")


@gpu
def test_the_other_calls_see_the_new_factor(monkeypatch):
    name = "g11-leaf8"
    dense_setup(monkeypatch, name)
    n, s, _, _ = dense_system(name)
    g = groups(name)
    pairs = g["two-leaves"] + g["separator"]
    s2 = changed(s, pairs)
    a2 = dense_matrix(s2, np.float64)
    bs = np.zeros((n, 2))
    bs[_places(name)["a"], 0] = 1.0
    bs[_places(name)["sep"], 1] = -0.5
    rows = [_places(name)["last"], _places(name)["b"]]
    bd = Dense.from_columns([rhs(name, np.float64)])
    er, ec = rc(g["seeded-17"][:6])

    def calls(f):
        x = f.solve_sparse(b_csr(bs, np.float64), rows)
        xr, ri = f.solve_refined(a2, bd)
        out = [arr(x), np.asarray(f.inv_entries(er, ec)), np.asarray(xr.get_col(0)), ri.iters, ri.berr]
        lam, _, ei = f.eigsh(a2, 2)
        return out, lam, ei

    with cholesky_nd(dense_matrix(s, np.float64)) as f, cholesky_nd(a2) as fresh:
        f.refactor_partial(a2, *rc(pairs))
        got, lam, ei = calls(f)
        want, lam_w, ei_w = calls(fresh)
    assert_same(got, want, "solve_sparse / inv_entries / solve_refined")
    # eigsh by its own test: both converged, and each eigenvalue within the two residuals of the other's
    assert np.all(ei.converged) and np.all(ei_w.converged)
    assert np.all(np.abs(np.asarray(lam) - np.asarray(lam_w)) <= np.asarray(ei.resid) + np.asarray(ei_w.resid))


# ---- 6: refusals, the factor's bits unchanged -----------------------------------------


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=[f"{np.dtype(a).name}-factor-{np.dtype(b).name}" for a, b in DTYPES])
def test_refusals_leave_the_factor(monkeypatch, dt):
    name = "g11-leaf8"
    dense_setup(monkeypatch, name)
    src, fdt = dt
    other = np.float32 if src == np.float64 else np.float64
    n, s, _, _ = dense_system(name)
    g, p = groups(name), _places(name)
    pairs = g["two-leaves"]
    s2 = changed(s, pairs)
    a2 = dense_matrix(s2, src)

    def l_bits(f):
        return [np.asarray(x) for x in f.l()._csr_arrays()]

    with cholesky_nd(dense_matrix(s, src), factor_dtype=fdt) as f:
        before = l_bits(f)
        far = next((i, j) for i in range(n) for j in range(i) if s[i, j] == 0)
        with pytest.raises(_lib.BsmError, match="not stored") as e:  # a pair that is not stored
            f.refactor_partial(a2, [pairs[0][0], far[0], far[1]], [pairs[0][1], far[1], far[0]])
        assert e.value.code == _lib.BSM_ERR_INVALID and "2 of the 3" in str(e.value) and "pair 1" in str(e.value)
        assert_same(l_bits(f), before)
        with pytest.raises(MatErr) as e:  # an index >= n
            f.refactor_partial(a2, [pairs[0][0], n], [pairs[0][1], 0])
        assert e.value.kind == MatErrKind.OutOfBounds
        assert_same(l_bits(f), before)
        sp = np.array(s2)
        sp[far[0], far[1]] = sp[far[1], far[0]] = -0.25
        with pytest.raises(_lib.BsmError, match="nd factor refactor: nnz differs") as e:  # another pattern
            f.refactor_partial(dense_matrix(sp, src), *rc(pairs))
        assert e.value.code == _lib.BSM_ERR_INVALID
        sq = np.array(sp)  # the same nnz, another col
        drop = next((i, j) for i, j in g["every-entry"] if i != j and (i, j) not in pairs)
        sq[drop[0], drop[1]] = sq[drop[1], drop[0]] = 0.0
        with pytest.raises(_lib.BsmError, match="nd factor refactor: (row_ptr|col) differs") as e:
            f.refactor_partial(dense_matrix(sq, src), *rc(pairs))
        assert e.value.code == _lib.BSM_ERR_INVALID
        with pytest.raises(_lib.BsmError, match="nd factor refactor: dtype differs") as e:  # a wrong dtype
            f.refactor_partial(dense_matrix(s2, other), *rc(pairs))
        assert e.value.code == _lib.BSM_ERR_INVALID
        with pytest.raises(_lib.BsmError, match="nd factor refactor: dtype differs"):
            f.refactor_partial(dense_matrix(s2, other), since=dense_matrix(s, other))
        with pytest.raises(TypeError):  # the two matrices of a since= call differ in dtype: refused on the host
            f.refactor_partial(dense_matrix(s2, src), since=dense_matrix(s, other))
        assert_same(l_bits(f), before)
        # after update: refused until a refactor
        w = np.zeros((n, 1))
        w[p["a"], 0] = 0.5
        f.update(b_csr(w, src))
        after_update = l_bits(f)
        for kw in ({"rows": rc(pairs)[0], "cols": rc(pairs)[1]}, {"since": dense_matrix(s, src)},
                   {"rows": [], "cols": []}):
            with pytest.raises(_lib.BsmError, match="refactor first") as e:
                f.refactor_partial(a2, **kw)
            assert e.value.code == _lib.BSM_ERR_UNSUPPORTED
        assert_same(l_bits(f), after_update)
        f.refactor(dense_matrix(s, src))
        assert_same(l_bits(f), before)
        info = f.refactor_partial(a2, *rc(pairs))
        assert info.fronts == len(reach(name, start_vertices(name, pairs)))
        assert_same(bits(f, name), fresh_bits(s2, name, src, fdt), "after update and refactor")
        # nothing named: the checks run, nothing else does
        info = f.refactor_partial(a2, [], [])
        assert (info.fronts, info.total_fronts, info.changed) == (0, len(_tree(name)["start"]), 0)
        assert_same(bits(f, name), fresh_bits(s2, name, src, fdt), "nothing named")


# ---- 7: not positive definite -----------------------------------------------------------


@gpu
def test_not_positive_definite(monkeypatch):
    name = "g11-leaf8"
    dense_setup(monkeypatch, name)
    n, s, _, _ = dense_system(name)
    v = _places(name)["a"]
    bad = np.array(s)
    bad[v, v] = -1.0
    with cholesky_nd(dense_matrix(s, np.float64)) as f:
        good = bits(f, name)
        with pytest.raises(_lib.BsmError, match="cholesky: matrix is not positive definite") as e:
            f.refactor_partial(dense_matrix(bad, np.float64), [v], [v])
        assert e.value.code == _lib.BSM_ERR_UNSUPPORTED
        with pytest.raises(_lib.BsmError, match="holds no values") as e:
            f.solve(Dense.from_columns([rhs(name, np.float64)]))
        assert e.value.code == _lib.BSM_ERR_INVALID
        f.refactor(dense_matrix(s, np.float64))
        assert_same(bits(f, name), good, "restored")
        # a handle without values has no update blocks to pull: a partial call factors every front
        with pytest.raises(_lib.BsmError, match="not positive definite"):
            f.refactor_partial(dense_matrix(bad, np.float64), since=dense_matrix(s, np.float64))
        info = f.refactor_partial(dense_matrix(s, np.float64), [v], [v])
        assert info.fronts == info.total_fronts
        assert_same(bits(f, name), good, "restored by a partial call")


# ---- 8: the pipeline switches, each in a fresh child process ------------------------------


@gpu
@pytest.mark.parametrize("switch", ["BSM_ND_PLAIN=1", "BSM_ND_LAG=0", "BSM_ND_POISON=1"])
def test_pipeline_switches(switch):
    key, val = switch.split("=")
    env = dict(os.environ, **{key: val, "BSM_ND_LEAF": dense_system("g11-leaf8")[3]})
    r = subprocess.run([sys.executable, os.path.join(HERE, "nd_partial_worker.py"), "g11-leaf8"], capture_output=True,
                       text=True, timeout=240, env=env, cwd=HERE)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["equal"] and out["finite"], out
    if key == "BSM_ND_PLAIN":
        assert out["fronts"] == [out["total"]] * len(out["fronts"])  # the full refactor: every front
    else:
        assert out["fronts"] == out["expected"]
