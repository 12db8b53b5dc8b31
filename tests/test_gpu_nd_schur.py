"""GPU tests of the Schur complement on a chosen set (cholesky_nd(a, schur=idx),
NdFactor.schur / schur_condense / schur_expand, device.nd_factor_schur*;
bsm_nd_factor_create_schur and bsm_nd_factor_schur*).

Shapes: nd_support's smallest systems that have each structure (one-pivot
fronts, several levels, a tree with a parent more than a level above a child,
fronts without pivots, an irregular tree), n <= 1600. Sets: one vertex, seven
scattered ones, a whole grid line (it disconnects the rest: the root's child
owns no column), on g40 two adjacent lines less ten vertices (m = 70, past one
64-tile, with gaps in the child's rows) and m = 129 (past two tiles), and on g5
all but one vertex and every vertex (no child at all).

Bounds. S against dense numpy in f64, S_ref = A_GG - W^T W with W = L_II^-1
A_IG and A the matrix as the factor saw it (rounded to f32 for an f32 factor):
componentwise |S - S_ref| <= 2 gamma_{n+2} (|A_GG| + |W|^T |W|), gamma_k = k u /
(1 - k u), u the factor dtype's unit roundoff: the standard bound of a Schur
complement computed by a partial Cholesky, doubled for the reference's own
rounding and the final conversion. L_GG L_GG^T (the last m rows and columns
of l()) against S with gamma_{m+2} in the same form, which shows that the root
front really is the set. The solver built from condense and expand, and solve
on a factor with a set, meet in backward error (omega_np) the figure
tests/test_gpu_nd_factor.py puts on a factor's solve for the dtype: TOL below,
restated from there."""

import functools

import numpy as np
import pytest
import scipy.linalg

import nd_support
from basic_sparse_matrix_amd import Csr, Dense, cholesky_nd
from nd_support import POISSON, coords, matrix, omega_np, same_bits, sym_dense, system

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TOL = {F64: 1e-10, F32: 2e-3}  # tests/test_gpu_nd_factor.py's
UNIT = {F64: 2.0 ** -53, F32: 2.0 ** -24}
PAIRS = [(F64, F64), (F32, F32), (F64, F32)]  # (matrix, factor)
PAIR_IDS = ["f64", "f32", "f32-of-f64"]
SYSTEMS = ["g5-leaf1", "g11-leaf8", "g40-leaf64", "blocks", "random"]


def gamma(k, u):
    return k * u / (1.0 - k * u)


@functools.lru_cache(maxsize=None)
def sets_of(name):
    n = system(name)[0]
    rng = np.random.default_rng(31)
    out = {"one": np.array([n // 3]), "seven": rng.choice(n, 7, replace=False)}
    if name in POISSON:
        g = POISSON[name][0]
        out["line"] = (g // 2) * g + np.arange(g)
    if name == "g40-leaf64":
        two = np.arange(19 * 40, 21 * 40)
        out["m70"] = rng.permutation(np.delete(two, rng.choice(80, 10, replace=False)))
        out["m129"] = np.arange(19 * 40, 19 * 40 + 129)
    if name == "g5-leaf1":
        out["n-1"] = rng.permutation(np.delete(np.arange(n), 12))
        out["n"] = rng.permutation(n)
    if name == "blocks":
        out["isolated"] = np.array([n - 1, 5, n - 9, 200])
    for v in out.values():
        v.setflags(write=False)
    return out


CASES = [(s, lab) for s in SYSTEMS for lab in sets_of(s)]
CASE_IDS = [f"{s}-{lab}" for s, lab in CASES]
SMALL = [("g5-leaf1", "n"), ("g11-leaf8", "line"), ("g40-leaf64", "m70"), ("blocks", "isolated"), ("random", "seven")]
SMALL_IDS = [f"{s}-{lab}" for s, lab in SMALL]


@functools.lru_cache(maxsize=None)
def seen_matrix(name, adt, fdt):
    """S as the library defines it (the stored lower triangle mirrored), dense f64, with the values as the factor saw
    them: the matrix's dtype, then the factor's."""
    v = np.asarray(system(name)[3]).astype(adt).astype(fdt)
    (s,) = nd_support._frozen(sym_dense(name, v))
    return s


@functools.lru_cache(maxsize=None)
def reference(name, label, adt, fdt):
    """(S_ref, the bound's magnitude |A_GG| + |W|^T |W|) in f64, in the set's own order."""
    A = seen_matrix(name, adt, fdt)
    idx = sets_of(name)[label]
    rest = np.setdiff1d(np.arange(A.shape[0]), idx)
    Agg = A[np.ix_(idx, idx)]
    if rest.size == 0:
        return nd_support._frozen(Agg.copy(), np.abs(Agg))
    L = np.linalg.cholesky(A[np.ix_(rest, rest)])
    W = scipy.linalg.solve_triangular(L, A[np.ix_(rest, idx)], lower=True)
    return nd_support._frozen(Agg - W.T @ W, np.abs(Agg) + np.abs(W).T @ np.abs(W))


def make(monkeypatch, name, label, adt, fdt, idx=None):
    nd_support.setup(monkeypatch, name)
    A = matrix(name, adt)
    idx = sets_of(name)[label] if idx is None else idx
    return A, idx, cholesky_nd(A, factor_dtype=None if adt == fdt else fdt, schur=idx)


def columns(n, k, dtype, seed=2001):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1.0, 1.0, n).astype(dtype) for _ in range(k)]


def as_array(d):
    return np.stack([np.asarray(d.get_col(j)) for j in range(d.get_dims().cols)], axis=1)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name,label", CASES, ids=CASE_IDS)
def test_schur_matrix(monkeypatch, name, label, pair):
    """S: exactly symmetric, the same bits twice and from the device call, the set reversed gives S reversed, m = n
    gives the matrix itself, and the two componentwise bounds of the module's docstring."""
    from basic_sparse_matrix_amd import device

    adt, fdt = pair
    n = system(name)[0]
    A, idx, f = make(monkeypatch, name, label, adt, fdt)
    m = len(idx)
    with f:
        assert np.array_equal(f.schur_index, idx) and f.dtype == np.dtype(fdt)
        perm = f.perm
        assert np.array_equal(np.sort(perm), np.arange(n)) and np.array_equal(perm[n - m:], np.sort(idx))
        S = f.schur(A)
        assert S.shape == (m, m) and S.dtype == np.dtype(fdt)
        assert same_bits(S, np.ascontiguousarray(S.T))
        assert same_bits(S, f.schur(A))
        assert same_bits(np.ascontiguousarray(S), device.nd_factor_schur(f, A).cpu().numpy())
        l = f.l()
        L = nd_support.dense_of(l.row_index, l.col_index, l.v, n)
    _, _, fr = make(monkeypatch, name, label, adt, fdt, idx=idx[::-1].copy())
    with fr:
        assert same_bits(np.ascontiguousarray(fr.schur(A)), np.ascontiguousarray(S[::-1, ::-1]))
    S64 = S.astype(F64)
    u = UNIT[fdt]
    if m == n:
        assert same_bits(np.ascontiguousarray(S), seen_matrix(name, adt, fdt)[np.ix_(idx, idx)].astype(fdt))
    ref, mag = reference(name, label, adt, fdt)
    err = np.abs(S64 - ref)
    bound = 2.0 * gamma(n + 2, u) * mag
    print(f"{name} {label}: max |S - S_ref| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3e}")
    assert np.all(err <= bound)
    o = np.argsort(idx)
    Lg = L[n - m:, n - m:]
    Ss = S64[np.ix_(o, o)]
    err = np.abs(Lg @ Lg.T - Ss)
    bound = 2.0 * gamma(m + 2, u) * (np.abs(Ss) + np.abs(Lg) @ np.abs(Lg).T)
    print(f"{name} {label}: max |L_GG L_GG^T - S| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3e}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name,label", CASES, ids=CASE_IDS)
def test_condense_expand(monkeypatch, name, label, pair):
    """expand(b, solve(b)[idx]) is solve(b) bit for bit on every row, for k = 1, 3 and 33 (the same kernels on the
    same inputs in the same order); and condense, a dense numpy solve of S x_G = g in f64, expand is a solver whose
    backward error, like solve's own on this factor, is within TOL."""
    adt, fdt = pair
    n = system(name)[0]
    A, idx, f = make(monkeypatch, name, label, adt, fdt)
    Sd = sym_dense(name, np.asarray(system(name)[3]).astype(adt))
    with f:
        for k in (1, 3, 33):
            cols = columns(n, k, fdt)
            b = Dense.from_columns(cols)
            x = as_array(f.solve(b))
            xe = as_array(f.schur_expand(b, np.ascontiguousarray(x[idx])))
            assert same_bits(xe, x), k
        S = f.schur(A).astype(F64)
        g = as_array(f.schur_condense(b))
        assert g.shape == (len(idx), 33) and g.dtype == np.dtype(fdt)
        xg = np.linalg.solve(S, g.astype(F64)).astype(fdt)
        x2 = as_array(f.schur_expand(b, Dense.from_columns([np.ascontiguousarray(xg[:, j]) for j in range(33)])))
    worst = [0.0, 0.0]
    for j in range(33):
        bj = cols[j].astype(F64)
        worst = [max(worst[0], omega_np(Sd, x2[:, j], bj)), max(worst[1], omega_np(Sd, x[:, j], bj))]
    print(f"{name} {label}: worst omega, condense + expand {worst[0]:.3e}, solve {worst[1]:.3e}")
    assert worst[0] <= TOL[fdt] and worst[1] <= TOL[fdt]


@pytest.mark.parametrize("name,label", SMALL, ids=SMALL_IDS)
def test_device_calls_equal_host_calls(monkeypatch, name, label):
    import torch

    from basic_sparse_matrix_amd import device

    n = system(name)[0]
    A, idx, f = make(monkeypatch, name, label, F64, F64)
    with f:
        b = Dense.from_columns(columns(n, 3, F64))
        bt = torch.from_numpy(as_array(b)).cuda()
        g = as_array(f.schur_condense(b))
        assert same_bits(device.nd_factor_schur_condense(f, bt).cpu().numpy(), g)
        xg = np.ascontiguousarray(np.linalg.solve(f.schur(A), g))
        x = as_array(f.schur_expand(b, xg))
        assert same_bits(device.nd_factor_schur_expand(f, bt, torch.from_numpy(xg).cuda()).cpu().numpy(), x)
        b1 = torch.from_numpy(np.ascontiguousarray(as_array(b)[:, 0])).cuda()  # (n,): one column
        assert same_bits(device.nd_factor_schur_condense(f, b1).cpu().numpy(), np.ascontiguousarray(g[:, 0]))


@pytest.mark.parametrize("name,label", SMALL, ids=SMALL_IDS)
def test_refactor_keeps_the_set(monkeypatch, name, label):
    """After refactor(a2), and after refactor_partial, schur(a2) has the bits of a fresh cholesky_nd(a2, schur=idx)'s,
    and so has condense."""
    n, _, _, v, _ = system(name)
    r, c = coords(name)
    A, idx, f = make(monkeypatch, name, label, F64, F64)
    rows = np.unique(np.concatenate([idx[:2], [0, n // 2]]))
    v2 = np.asarray(v).copy()
    v2[np.isin(r, rows) & (r == c)] *= 1.5
    A2, A3 = matrix(name, F64, v2), matrix(name, F64, 2.0 * v2)
    b = Dense.from_columns(columns(n, 2, F64))
    with f:
        f.refactor_partial(A2, rows, rows)
        with cholesky_nd(A2, schur=idx) as fresh:
            assert same_bits(f.schur(A2), fresh.schur(A2))
            assert same_bits(as_array(f.schur_condense(b)), as_array(fresh.schur_condense(b)))
        f.refactor(A3)
        assert np.array_equal(f.schur_index, idx)
        with cholesky_nd(A3, schur=idx) as fresh:
            assert same_bits(f.schur(A3), fresh.schur(A3))
            assert same_bits(as_array(f.schur_condense(b)), as_array(fresh.schur_condense(b)))


def test_state_and_refusals(monkeypatch):
    name = "g11-leaf8"
    n = system(name)[0]
    A, idx, f = make(monkeypatch, name, "line", F64, F64)
    b = Dense.from_columns(columns(n, 2, F64))
    w = np.zeros((n, 1))
    w[7, 0] = 0.5  # a diagonal column: always inside the pattern
    rp, ci, wv = nd_support.csr_arrays(w)
    W = Csr.from_csr_arrays((n, 1), rp, ci, wv)
    with f:
        S = f.schur(A)
        xg = np.zeros((len(idx), 2))
        for change in (f.update, f.downdate):
            change(W)
            for call in (lambda: f.schur(A), lambda: f.schur_condense(b), lambda: f.schur_expand(b, xg)):
                with pytest.raises(Exception, match="refactor first"):
                    call()
            f.solve(b)  # the factor itself is fine
            f.refactor(A)
            assert same_bits(f.schur(A), S)
        other = nd_support.dense_matrix(sym_dense(name, system(name)[3]) + np.eye(n, k=5) + np.eye(n, k=-5), F64)
        with pytest.raises(Exception, match="differs"):
            f.schur(other)
        with pytest.raises(Exception, match="n differs"):
            f.schur(matrix("g5-leaf1", F64))
        with pytest.raises(Exception):  # Dense of another dtype, another row count
            f.schur_condense(Dense.from_columns(columns(n, 1, F32)))
        with pytest.raises(Exception):
            f.schur_condense(Dense.from_columns(columns(n + 1, 1, F64)))
        with pytest.raises(Exception):
            f.schur_expand(b, np.zeros((len(idx) + 1, 2)))
    with cholesky_nd(A) as plain:
        assert plain.schur_index.size == 0
        for call in (lambda: plain.schur(A), lambda: plain.schur_condense(b), lambda: plain.schur_expand(b, xg)):
            with pytest.raises(Exception, match="without a Schur set"):
                call()
    with cholesky_nd(A, schur=[]) as none:  # an empty set is no set: the unconstrained factor
        assert none.schur_index.size == 0 and np.array_equal(none.perm, plain_perm(A))
    for bad, what in (([1, n], r"idx\[1\]"), ([4, 9, 4], "repeats")):
        with pytest.raises(Exception, match=what):
            cholesky_nd(A, schur=bad)


@pytest.mark.parametrize("name,label", [("g11-leaf8", "line"), ("g40-leaf64", "m70")], ids=["g11-line", "g40-m70"])
def test_other_methods_on_a_factor_with_a_set(monkeypatch, name, label):
    """It is a factor of P A P^T with another P: logdet and the selected inverse agree with an unconstrained factor's
    to rounding (1e-10 relative, TOL's f64 figure: other elimination orders of a well-conditioned matrix), the sparse
    solve equals its own dense solve, and the refined and pcg solves converge."""
    n = system(name)[0]
    A, idx, f = make(monkeypatch, name, label, F64, F64)
    b = Dense.from_columns(columns(n, 2, F64))
    with f, cholesky_nd(A) as plain:
        assert abs(f.logdet() - plain.logdet()) <= TOL[F64] * abs(plain.logdet())
        d, dp = f.inv_diag(), plain.inv_diag()
        assert np.max(np.abs(d - dp)) <= TOL[F64] * np.max(np.abs(dp))
        rows = np.concatenate([idx[:3], [0, n - 1]])
        blk = f.inv_block(rows, idx[:2])
        unit = np.zeros((n, 2))
        unit[idx[0], 0] = unit[idx[1], 1] = 1.0
        z = as_array(f.solve(Dense.from_columns([unit[:, 0].copy(), unit[:, 1].copy()])))
        assert np.array_equal(blk, z[rows])
        _, info = f.solve_refined(A, b)
        assert info.converged.all()
        _, info = f.solve_pcg(A, b)
        assert info.converged.all() and not info.breakdown.any()


def plain_perm(A):
    with cholesky_nd(A) as f:
        return f.perm


def test_plan_caches_never_mix(monkeypatch):
    """One handle, BSM_ND_SHARED=1: an unconstrained factor, one with a set, an unconstrained one again; the first
    and third have the same perm (the constrained plan went into neither cache), the second ends in the sorted set;
    two sets on one pattern each get their own plan; and a new handle of the pattern gets the unconstrained plan from
    the shared cache."""
    from basic_sparse_matrix_amd import _lib

    name = "g40-leaf64"
    monkeypatch.setenv("BSM_ND_SHARED", "1")
    nd_support.setup(monkeypatch, name)
    _lib.nd_cache_clear()
    n = system(name)[0]
    A = matrix(name, F64)
    ia, ib = sets_of(name)["line"], sets_of(name)["m70"]
    with cholesky_nd(A) as f1, cholesky_nd(A, schur=ia) as f2, cholesky_nd(A) as f3, \
            cholesky_nd(A, schur=ib) as f4, cholesky_nd(matrix(name, F64)) as f5, \
            cholesky_nd(matrix(name, F64), schur=ia) as f6:
        p1, p2, p3, p4, p5, p6 = (f.perm for f in (f1, f2, f3, f4, f5, f6))
        assert np.array_equal(p1, p3) and np.array_equal(p1, p5)
        assert np.array_equal(p2[n - len(ia):], np.sort(ia)) and np.array_equal(p4[n - len(ib):], np.sort(ib))
        assert not np.array_equal(p1[n - len(ia):], np.sort(ia))
        assert np.array_equal(p2, p6)
        assert f1.schur_index.size == 0 and f3.schur_index.size == 0 and f5.schur_index.size == 0
        b = Dense.from_columns(columns(n, 2, F64))
        assert same_bits(as_array(f1.solve(b)), as_array(f3.solve(b)))
        assert same_bits(f2.schur(A), f6.schur(A))
    assert _lib.nd_cache_info()["entries"] == 1


ENVS = [{"BSM_ND_PLAIN": "1"}, {"BSM_ND_FWD_TILES": "0", "BSM_ND_BWD_TILES": "0"},
        {"BSM_ND_FWD_TILES": "1", "BSM_ND_BWD_TILES": "1"}, {"BSM_ND_FWD_TILES": "0", "BSM_ND_BWD_TILES": "1"},
        {"BSM_ND_POISON": "1"}]


@pytest.mark.parametrize("name,label", SMALL[1:4], ids=SMALL_IDS[1:4])
def test_pipelines_give_the_same_bits(monkeypatch, name, label):
    """The plain pipeline (which also leaves the update blocks in place: nd_extend2 only reads them), the solves by
    tiles on no level and on every level, and fronts poisoned before the factorisation: S, g and x as by default."""
    n = system(name)[0]
    b = Dense.from_columns(columns(n, 3, F64))

    def run():
        A, idx, f = make(monkeypatch, name, label, F64, F64)
        with f:
            S = f.schur(A)
            g = as_array(f.schur_condense(b))
            x = as_array(f.schur_expand(b, np.linalg.solve(S, g)))
        return S, g, x

    want = run()
    for env in ENVS:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            got = run()
        for w, g_, what in zip(want, got, ("S", "g", "x")):
            assert same_bits(w, g_), (env, what)
