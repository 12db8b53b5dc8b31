"""The constrained host analysis behind cholesky_nd(a, schur=idx)
(bsm_nd_analyse_last, csrc/nd_order.cpp): no device use, so these run on the
CPU. The given vertices become the root node's own columns, in ascending
order, over the ordinary bisection tree of the other vertices; everything the
multifrontal code relies on must still hold for that tree, and without a set
the plan must be the unconstrained one, array for array.

Systems: nd_support's g11-leaf8, g40-leaf64, blocks (two grids and nine
isolated vertices) and random, each with its BSM_ND_LEAF (64 where it has
none). The sets are the shapes the GPU tests use and the degenerate ones."""

import ctypes

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib
from basic_sparse_matrix_amd.solver import nd_analyse
from nd_support import POISSON, system

SYSTEMS = ["g11-leaf8", "g40-leaf64", "blocks", "random"]


def pattern(name):
    n, rp, ci, _, leaf = system(name)
    return n, rp, ci, int(leaf) if leaf is not None else 64


def sets_of(name):
    """{label: set}: one vertex, seven scattered ones, and a whole grid line (which disconnects the rest) or, for
    `blocks`, its isolated vertices with a few others."""
    n = system(name)[0]
    rng = np.random.default_rng(31)
    out = {"one": np.array([n // 3]), "seven": rng.choice(n, 7, replace=False)}
    if name in POISSON:
        g = POISSON[name][0]
        out["line"] = (g // 2) * g + np.arange(g)
    if name == "blocks":
        out["isolated"] = np.array([n - 1, 5, n - 9, 200])  # two of the nine isolated vertices among grid vertices
    return out


def symbolic_columns(n, later):
    """L's column structures of the ordered graph (tests/test_nd_analysis.py's, restated): struct(j) = j's later
    neighbours merged with struct(c) - {j} over j's elimination-tree children c."""
    struct = [set() for _ in range(n)]
    kids = [[] for _ in range(n)]
    for j in range(n):
        s = set(later[j])
        for c in kids[j]:
            s |= struct[c]
        s.discard(j)
        struct[j] = s
        if s:
            kids[min(s)].append(j)
    return struct


def check_constrained(n, rp, ci, leaf, idx):
    plan = nd_analyse(n, rp, ci, leaf, last=idx)
    m = len(idx)
    perm, start, end, parent, level = plan["perm"], plan["start"], plan["end"], plan["parent"], plan["level"]
    nn = len(start)
    assert np.array_equal(np.sort(perm), np.arange(n))
    assert np.array_equal(perm[n - m:], np.sort(np.asarray(idx, dtype=np.int64)))
    # the last node is the root: it owns [n - m, n), has an empty st and exactly one child (none when m == n)
    assert (start[-1], end[-1], parent[-1]) == (n - m, n, -1)
    assert len(plan["st"][-1]) == 0
    kids = np.nonzero(parent == nn - 1)[0]
    assert len(kids) == (1 if m < n else 0)
    assert np.count_nonzero(parent == -1) == 1
    if m < n:
        assert plan["slot"][kids[0]] == 0 and level[-1] == level[kids[0]] + 1
        assert np.all(level[:-1] < level[-1])  # alone on the top level
    # post-order, own columns tiling [0, n)
    assert start[0] == 0 and np.all(start[1:] == end[:-1]) and np.all(end >= start)
    for i in range(nn - 1):
        assert parent[i] > i and level[parent[i]] > level[i]
    # every node's st holds a plain symbolic elimination's rows, in that order
    pinv = np.empty(n, dtype=np.int64)
    pinv[perm] = np.arange(n)
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    cols = ci.astype(np.int64)
    off = rows != cols
    a, b = np.minimum(pinv[rows[off]], pinv[cols[off]]), np.maximum(pinv[rows[off]], pinv[cols[off]])
    later = [[] for _ in range(n)]
    for x, y in zip(a.tolist(), b.tolist()):
        later[x].append(y)
    struct = symbolic_columns(n, later)
    for i in range(nn):
        s = plan["st"][i]
        assert np.all(np.diff(s) > 0) and (len(s) == 0 or s[0] >= end[i])
        want = set()
        for j in range(start[i], end[i]):
            want |= {q for q in struct[j] if q >= end[i]}
        assert want <= set(s.tolist()), i
    return plan


def same_plan(p, q):
    return all(np.array_equal(p[k], q[k]) for k in ("perm", "start", "end", "parent", "level", "slot")) and \
        len(p["st"]) == len(q["st"]) and all(np.array_equal(x, y) for x, y in zip(p["st"], q["st"]))


@pytest.mark.parametrize("name", SYSTEMS)
def test_constrained_plans(name):
    n, rp, ci, leaf = pattern(name)
    for label, idx in sets_of(name).items():
        plan = check_constrained(n, rp, ci, leaf, idx)
        # the same set in another order: the same plan
        assert same_plan(plan, nd_analyse(n, rp, ci, leaf, last=idx[::-1].copy())), label
        assert same_plan(plan, nd_analyse(n, rp, ci, leaf, last=np.roll(idx, 3))), label


@pytest.mark.parametrize("name", SYSTEMS)
def test_no_set_is_the_unconstrained_plan(name):
    n, rp, ci, leaf = pattern(name)
    assert same_plan(nd_analyse(n, rp, ci, leaf), nd_analyse(n, rp, ci, leaf, last=np.zeros(0, dtype=np.uint64)))


@pytest.mark.parametrize("name", ["g11-leaf8", "blocks"])
def test_every_vertex_and_all_but_one(name):
    n, rp, ci, leaf = pattern(name)
    rng = np.random.default_rng(5)
    plan = check_constrained(n, rp, ci, leaf, rng.permutation(n))
    assert len(plan["start"]) == 1 and np.array_equal(plan["perm"], np.arange(n))
    rest = np.delete(np.arange(n), n // 2)
    plan = check_constrained(n, rp, ci, leaf, rng.permutation(rest))
    assert len(plan["start"]) == 2 and plan["perm"][0] == n // 2


def test_a_grid_line_leaves_two_components_under_one_child():
    n, rp, ci, leaf = pattern("g40-leaf64")
    plan = check_constrained(n, rp, ci, leaf, 20 * 40 + np.arange(40))
    nn = len(plan["start"])
    (kid,) = np.nonzero(plan["parent"] == nn - 1)[0]
    # no separator between the halves: the child owns no column and has both halves under it
    assert plan["end"][kid] == plan["start"][kid] and np.count_nonzero(plan["parent"] == kid) == 2


def test_bad_sets_are_refused():
    n, rp, ci, leaf = pattern("g11-leaf8")
    lib = _lib.load()
    nn, sl = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def rc(idx):
        lv = np.asarray(idx, dtype=np.uint64)
        return lib.bsm_nd_analyse_last(n, _lib.ptr(rp), _lib.ptr(ci), leaf, _lib.ptr(lv), lv.shape[0], None, None, 0,
                                       ctypes.byref(nn), None, 0, ctypes.byref(sl))

    assert rc([0, 5, 7]) == _lib.BSM_OK
    assert rc([0, n]) == _lib.BSM_ERR_INVALID
    assert rc([3, 5, 3]) == _lib.BSM_ERR_INVALID
    assert rc([2 ** 63, 1]) == _lib.BSM_ERR_INVALID
    assert lib.bsm_nd_analyse_last(n, _lib.ptr(rp), _lib.ptr(ci), leaf, None, 2, None, None, 0, ctypes.byref(nn), None,
                                   0, ctypes.byref(sl)) == _lib.BSM_ERR_INVALID


@pytest.mark.parametrize("name", ["g40-leaf64", "random"])
def test_eight_threads_equal_one(monkeypatch, name):
    n, rp, ci, leaf = pattern(name)
    idx = sets_of(name)["seven"]
    plans = []
    for t in ("1", "8"):
        monkeypatch.setenv("BSM_ND_THREADS", t)
        plans.append(nd_analyse(n, rp, ci, leaf, last=idx))
    assert same_plan(*plans)
