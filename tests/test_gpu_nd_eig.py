"""GPU tests of the smallest eigenpairs by block shift-invert Lanczos on a kept
nd factor (NdFactor.eigsh, device.nd_factor_eigsh, bsm_nd_factor_eigsh).

The systems are nd_support.py's, as in test_gpu_nd_pcg.py: one-pivot fronts
(g5-leaf1), several levels (g11-leaf8), multi-tile fronts (g40-leaf256), fronts
without pivots (blocks) and an irregular tree (random). The reference is
np.linalg.eigvalsh / eigh of the dense S (the stored entries with column <=
row, mirrored). nev = 6 and block = 4 throughout; ncv = 160 for `random`, 60
for the others and 24 for g5 (n = 25).

Bounds, with tol the default (2^-26 for an f64 matrix, 2^-12 for an f32 one)
and N = ||S||inf. A pair whose estimate is at or below tol has a true residual
resid <= tol N up to rounding (S y - lam y = -lam S (A^-1 y - theta y)): held
to 2 tol N. resid recomputed here in longdouble is held to twice the reported
one plus (m + 2) 2^-53 N, the rounding bound of the device's f64 product (m the
longest row of S). |lam_i - ref_i| <= resid_i + 4 n 2^-53 N against the i-th
smallest reference value IN ORDER: Weyl's bound for a residual, plus the
rounding of eigvalsh itself; a missed copy of a multiple eigenvalue shifts the
list and breaks it. ||Y^T Y - I||max <= 2 tol: converged Ritz vectors of
different eigenvalues are orthogonal to the order of the residuals. The step
counts are held to this file's numpy emulation of the loop, with
np.linalg.cholesky in the factor's dtype as the factor, plus 2: the slack of
test_gpu_nd_pcg.py, for the same reason (the nd factor sums in another order
than the dense one)."""

import functools

import numpy as np
import pytest

from basic_sparse_matrix_amd import Csr, Dense, EigInfo, MatErr, _lib, cholesky_nd
from nd_support import _scale, assert_same, cols_of, coords, matrix, same_bits, setup, start_block, sym_dense, system

pytestmark = pytest.mark.gpu

SYSTEMS = ["g5-leaf1", "g11-leaf8", "g40-leaf256", "blocks", "random"]
NCV = {"g5-leaf1": 24, "g11-leaf8": 60, "g40-leaf256": 60, "blocks": 60, "random": 160}
F32, F64 = np.float32, np.float64
NEV, BLOCK = 6, 4
TOL64, TOL32 = 2.0 ** -26, 2.0 ** -12
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _truth(name, dtype=F64):
    """(S dense f64 of the values rounded to dtype, ||S||inf, m, eigenvalues ascending, eigenvectors)."""
    S = sym_dense(name, system(name)[3].astype(dtype))
    S.setflags(write=False)
    w, z = np.linalg.eigh(S)
    return S, float(np.abs(S).sum(axis=1).max()), int((S != 0).sum(axis=1).max()), w, z


def parts(lam, y, info):
    return [lam] + (cols_of(y) if y is not None else []) + [info.resid, info.converged,
                                                           np.array([info.steps, info.ncv_used, info.exhausted,
                                                                     info.inexact])]


def assert_pairs(name, lam, y, info, tol, what, dtype=F64, count=NEV):
    """The bounds of the module docstring on the first `count` pairs."""
    S, N, m, ref, _ = _truth(name, dtype)
    n = S.shape[0]
    assert isinstance(info, EigInfo) and info.tol == tol and lam.dtype == np.float64
    Y = np.stack([np.asarray(c, np.float64) for c in cols_of(y)[:count]], axis=1)
    L = np.longdouble
    R = np.asarray(S, L) @ np.asarray(Y, L) - np.asarray(Y, L) * np.asarray(lam[:count], L)
    true = np.sqrt((R * R).sum(axis=0)) / np.sqrt((np.asarray(Y, L) ** 2).sum(axis=0))
    orth = np.abs(Y.T @ Y - np.eye(count)).max()
    print(f"{what} {name}: steps {info.steps} ncv_used {info.ncv_used} orth {orth:.3e}")
    for i in range(count):
        print(f"  pair {i}: lam {lam[i]:.16e} ref {ref[i]:.16e} resid {info.resid[i]:.3e} longdouble {float(true[i]):.3e}")
    assert np.all(np.diff(lam[:count]) >= 0)
    for i in range(count):
        assert info.converged[i]
        assert info.resid[i] <= 2 * tol * N
        assert float(true[i]) <= 2 * info.resid[i] + (m + 2) * U * N
        assert abs(lam[i] - ref[i]) <= info.resid[i] + 4 * n * U * N
    assert orth <= 2 * tol


# ---- the loop, emulated: np.linalg.cholesky in the factor's dtype stands for the factor -------


@functools.lru_cache(maxsize=None)
def emulated_steps(name, fdtype, ncv, tol=TOL64, nev=NEV, block=BLOCK):
    """The Lanczos steps a numpy run of the library's loop takes."""
    from scipy.linalg import solve_triangular

    S, N, m, _, _ = _truth(name)
    n = S.shape[0]
    Lf = np.linalg.cholesky(S.astype(fdtype))
    rtol = (m + 2) * U

    def minv(v):
        s = _scale(v)
        y = solve_triangular(Lf, (v / s).astype(fdtype), lower=True)
        return s * solve_triangular(Lf.T, y, lower=False).astype(np.float64)

    def op(b):  # the refined solve, column by column
        x = minv(b)
        for _ in range(5):
            r = b - S @ x
            if np.abs(r).max() / (N * np.abs(x).max() + np.abs(b).max()) <= rtol:
                break
            x = x + minv(r)
        return x

    def cholqr2(W, norm2):
        G = W.T @ W
        try:
            R1 = np.linalg.cholesky(G).T
        except np.linalg.LinAlgError:
            return None
        if np.any(np.diag(R1) ** 2 <= 2.0 ** -50 * norm2):
            return None
        W = W @ np.linalg.inv(R1)
        R2 = np.linalg.cholesky(W.T @ W).T
        return W @ np.linalg.inv(R2), R2 @ R1

    W = start_block(n, block)
    V, _ = cholqr2(W, (W * W).sum(axis=0))
    T = np.zeros((ncv, ncv))
    steps = 0
    while True:
        j = steps
        W = np.stack([op(V[:, j * block + c]) for c in range(block)], axis=1)
        norm2 = (W * W).sum(axis=0)
        a = np.zeros((block, block))
        for _ in range(2):
            C = V.T @ W
            W = W - V @ C
            a += C[-block:]
        o = j * block
        T[o:o + block, o:o + block] = 0.5 * (a + a.T)
        steps += 1
        mm = steps * block
        q = cholqr2(W, norm2)
        if q is None:
            return steps
        Wn, B = q
        if mm >= nev:
            th, s = np.linalg.eigh(T[:mm, :mm])
            est = [np.linalg.norm(B @ s[mm - block:, mm - 1 - i]) / abs(th[mm - 1 - i]) for i in range(nev)]
            if max(est) <= tol:
                return steps
        if mm + block > ncv:
            return steps
        T[mm:mm + block, o:o + block] = B
        T[o:o + block, mm:mm + block] = B.T
        V = np.concatenate([V, Wn], axis=1)


# ---- convergence and accuracy ------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _default_run(name, fdtype):
    """(lam, Dense, info) of the default call on the f64 matrix; the caller has set BSM_ND_LEAF."""
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=fdtype) as f:
        return f.eigsh(A, NEV, block=BLOCK, ncv=NCV[name])


@pytest.mark.parametrize("fdtype", [F64, F32], ids=["f64-factor", "f32-factor"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_smallest_pairs_of_an_f64_matrix(monkeypatch, name, fdtype):
    setup(monkeypatch, name)
    lam, y, info = _default_run(name, fdtype)
    assert y.dtype == np.dtype(F64) and y.get_dims().cols == NEV and y.get_dims().rows == system(name)[0]
    assert not info.inexact
    assert_pairs(name, lam, y, info, TOL64, f"{np.dtype(fdtype).name} factor")


@pytest.mark.parametrize("fdtype", [F64, F32], ids=["f64-factor", "f32-factor"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_steps_are_the_emulations(monkeypatch, name, fdtype):
    setup(monkeypatch, name)
    _, _, info = _default_run(name, fdtype)
    emu = emulated_steps(name, fdtype, NCV[name])
    print(f"{name} {np.dtype(fdtype).name} factor: steps {info.steps}, emulation {emu}")
    assert info.steps <= emu + 2
    assert info.ncv_used == info.steps * BLOCK


def test_f32_matrix_with_an_f32_factor(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    A = matrix(name, F32)
    with cholesky_nd(A) as f:
        lam, y, info = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[name])
    assert y.dtype == np.dtype(F32)
    assert_pairs(name, lam, y, info, TOL32, "f32 matrix", dtype=F32)


# ---- bits --------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["g11-leaf8", "random"])
def test_calls_repeat_and_v0_restates_the_seed(monkeypatch, name):
    setup(monkeypatch, name)
    n = system(name)[0]
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        want = parts(*f.eigsh(A, NEV, block=BLOCK, ncv=NCV[name], seed=3))
        assert_same(parts(*f.eigsh(A, NEV, block=BLOCK, ncv=NCV[name], seed=3)), want)
        v0 = start_block(n, BLOCK, seed=3)
        got = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[name], v0=Dense.from_columns([v0[:, c].copy() for c in range(BLOCK)]))
        assert_same(parts(*got), want)
        other = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[name], seed=4)  # another start: the same values, other bits
        assert not same_bits(other[0], want[0])
        assert np.abs(other[0] - want[0]).max() <= 2 * TOL64 * _truth(name)[1]


def test_the_upper_triangle_is_ignored(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    r, c = coords(name)
    v = system(name)[3]
    junk = np.where(c > r, 1e6 * (1.0 + np.arange(v.size)), v)
    with cholesky_nd(matrix(name, F64), factor_dtype=F32) as f:
        want = parts(*f.eigsh(matrix(name, F64), NEV, block=BLOCK, ncv=NCV[name]))
        assert_same(parts(*f.eigsh(matrix(name, F64, junk), NEV, block=BLOCK, ncv=NCV[name])), want)


@pytest.mark.parametrize("env", [{}, {"BSM_ND_FWD_TILES": "1", "BSM_ND_BWD_TILES": "1"}, {"BSM_ND_PLAIN": "1"}],
                         ids=["default", "tiles", "plain"])
def test_device_call_and_switches_have_the_default_host_calls_bits(monkeypatch, env):
    import torch

    from basic_sparse_matrix_amd import device

    name = "g40-leaf256"
    setup(monkeypatch, name)
    n = system(name)[0]
    want = parts(*_default_run(name, F32))  # made (or to be made now) without the switches
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        assert_same(parts(*f.eigsh(A, NEV, block=BLOCK, ncv=NCV[name])), want)
        lam, out, info = device.nd_factor_eigsh(f, A, NEV, block=BLOCK, ncv=NCV[name])
        assert tuple(out.shape) == (n, NEV) and out.is_cuda
        got = out.cpu().numpy()
        assert_same([lam] + [np.ascontiguousarray(got[:, j]) for j in range(NEV)]
                    + parts(lam, None, info)[1:], want)
        mine = torch.full((n, NEV), 7.0, dtype=torch.float64, device="cuda")
        v0 = torch.from_numpy(start_block(n, BLOCK)).cuda().contiguous()
        lam2, same, info2 = device.nd_factor_eigsh(f, A, NEV, block=BLOCK, ncv=NCV[name], v0=v0, out=mine)
        assert same is mine
        got = mine.cpu().numpy()
        assert_same([lam2] + [np.ascontiguousarray(got[:, j]) for j in range(NEV)]
                    + parts(lam2, None, info2)[1:], want)
        lam3, none, info3 = device.nd_factor_eigsh(f, A, NEV, block=BLOCK, ncv=NCV[name], vectors=False)
        assert none is None
        assert_same(parts(lam3, None, info3), [want[0]] + want[1 + NEV:])
        with pytest.raises(TypeError):
            device.nd_factor_eigsh(f, A, NEV, out=torch.zeros((n, NEV), dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            device.nd_factor_eigsh(f, A, NEV, out=torch.zeros((n, NEV + 1), dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            device.nd_factor_eigsh(f, A, NEV, v0=torch.zeros((n, BLOCK), dtype=torch.float64))


# ---- multiplicity, exhaustion, edges ------------------------------------------------------------


def test_multiplicity_three_is_found_block_times_at_most(monkeypatch):
    """Documented behaviour: three copies of the 7 x 7-grid Poisson matrix have every eigenvalue three times;
    block = 2 sees two copies of the smallest, block = 4 all three. nev = 3 is the smallest count that tells the
    two apart, and it stops the block = 2 run soon after its pairs have converged. The limit holds in exact
    arithmetic only: with nev = 6 that run goes on for 24 steps (its last pairs lie higher in the spectrum), and
    by then rounding has let the third copy in and it is returned too (measured: lam = 0.30448187 three times,
    resid 2e-15 .. 1e-14)."""
    name = "triple"
    nev = 3
    S, N, _, ref, _ = _truth(name)
    assert abs(ref[2] - ref[0]) <= 8 * U * N and ref[3] - ref[2] > 0.1  # the smallest, three times
    A = matrix(name, F64)
    with cholesky_nd(A) as f:
        for block, copies in ((2, 2), (4, 3)):
            lam, y, info = f.eigsh(A, nev, block=block, ncv=60)
            print(f"block {block}: steps {info.steps} lam {lam} resid {info.resid}")
            assert info.converged.all()
            assert np.all(info.resid <= 2 * TOL64 * N)
            assert int((np.abs(lam - ref[0]) <= 2 * TOL64 * N).sum()) == copies
            for i in range(nev):  # every value returned is an eigenvalue
                assert np.abs(ref - lam[i]).min() <= info.resid[i] + 4 * S.shape[0] * U * N


def test_exhausted_on_an_invariant_start_block(monkeypatch):
    name = "g5-leaf1"
    setup(monkeypatch, name)
    S, N, m, ref, z = _truth(name)
    n = S.shape[0]
    pick = [0, 3, 7, 12]  # simple eigenvalues of the 5 x 5 grid and others: four exact eigenvectors, mixed
    mix = np.array([[1.0, 0.5, 0.0, 0.0], [0.0, 1.0, 0.5, 0.0], [0.0, 0.0, 1.0, 0.5], [0.25, 0.0, 0.0, 1.0]])
    v0 = z[:, pick] @ mix
    A = matrix(name, F64)
    with cholesky_nd(A) as f:
        lam, y, info = f.eigsh(A, NEV, block=BLOCK, ncv=24, v0=Dense.from_columns([v0[:, c].copy() for c in range(4)]))
    print(f"steps {info.steps} ncv_used {info.ncv_used} lam {lam} resid {info.resid}")
    assert info.exhausted and info.steps == 1 and info.ncv_used == 4
    assert np.isnan(lam[4:]).all() and np.isnan(info.resid[4:]).all() and not info.converged[4:].any()
    assert not any(np.asarray(y.get_col(j)).any() for j in (4, 5))
    assert info.converged[:4].all()
    assert np.all(info.resid[:4] <= 64 * n * U * N)  # rounding level: the space is invariant
    assert np.abs(lam[:4] - np.sort(ref[pick])).max() <= 64 * n * U * N


def test_edge_cases(monkeypatch):
    name = "g11-leaf8"
    setup(monkeypatch, name)
    S, N, m, ref, _ = _truth(name)
    n = S.shape[0]
    A = matrix(name, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        lam, y, info = f.eigsh(A, 1, block=1)  # one pair, one vector at a time
        assert info.converged.all() and abs(lam[0] - ref[0]) <= info.resid[0] + 4 * n * U * N
        assert info.resid[0] <= 2 * TOL64 * N and y.get_dims().cols == 1
        want = parts(*f.eigsh(A, NEV, block=BLOCK, ncv=NCV[name]))
        lam_only, none, info_only = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[name], vectors=False)  # values only
        assert none is None
        assert_same(parts(lam_only, None, info_only), [want[0]] + want[1 + NEV:])
        # a basis too small to converge: true residuals, and a second call from the first one's vectors converges
        lam1, y1, info1 = f.eigsh(A, NEV, block=BLOCK, ncv=8)
        print(f"ncv 8: resid {info1.resid}")
        assert info1.ncv_used == 8 and info1.steps == 2 and not info1.exhausted and not info1.converged.all()
        Y1 = np.stack(cols_of(y1), axis=1)
        true = np.linalg.norm(S @ Y1 - Y1 * lam1, axis=0) / np.linalg.norm(Y1, axis=0)
        assert np.all(np.abs(true - info1.resid) <= 1e-3 * info1.resid + (m + 2) * U * N)
        lam2, y2, info2 = f.eigsh(A, NEV, block=BLOCK, ncv=100, v0=Dense.from_columns(cols_of(y1)[:BLOCK]))
        assert info2.converged.all()
        assert_pairs(name, lam2, y2, info2, TOL64, "second call")
        with pytest.raises(MatErr, match="IncorrectDimensions"):
            f.eigsh(matrix("g5-leaf1", F64), NEV)
        with pytest.raises(MatErr, match="IncorrectDimensions"):
            f.eigsh(A, NEV, v0=Dense.from_columns([np.ones(n + 1)] * BLOCK))
        with pytest.raises(TypeError):
            f.eigsh(A, NEV, v0=Dense.from_columns([np.ones(n, dtype=F32)] * BLOCK))
        with pytest.raises(TypeError):
            f.eigsh(matrix(name, np.int32, np.ones(system(name)[3].size)), NEV)
        with pytest.raises(ValueError, match="ncv"):
            f.eigsh(A, NEV, ncv=n + 4)
        bad = system(name)[3].copy()
        r, c = coords(name)
        e = int(np.nonzero((r == n // 2) & (c == n // 2))[0][0])
        bad[e] = -bad[e]
        with pytest.raises(_lib.BsmError):
            f.refactor(matrix(name, F64, bad))  # not positive definite: the handle holds no factor
        with pytest.raises(_lib.BsmError, match="refactor first"):
            f.eigsh(A, NEV)
    E = Csr.from_csr_arrays((0, 0), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0))
    with cholesky_nd(E, factor_dtype=F32) as f:  # n = 0
        lam, y, info = f.eigsh(E, NEV)
        assert lam.size == 0 and y.get_dims().cols == 0 and info.resid.size == 0 and info.steps == 0
