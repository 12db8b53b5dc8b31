"""GPU tests of the generalised problem S y = lam S_M y by block shift-invert
Lanczos on a kept nd factor (NdFactor.eigsh(m=...), device.nd_factor_eigsh(m=...),
bsm_nd_factor_eigsh_gen).

The Poisson systems are nd_support.py's: A is the 5-point
Poisson matrix of a g x g grid with the consistent mass matrix kron(M1, M1), M1
= tridiag(1/6, 4/6, 1/6) (a 9-point pattern on a 5-point A): one-pivot fronts
(g9-leaf1), several levels (g11-leaf8), multi-tile fronts (g40-leaf256); and an
irregular tree (random) with a random diagonally dominant M of another pattern.
The reference is scipy.linalg.eigh(S, S_M) of the dense matrices (the stored
entries with column <= row, mirrored). nev = 6 and block = 4 unless a case says
otherwise.

Bounds, with tol the default (2^-26 for an f64 matrix, 2^-12 for an f32 one),
N, N_M the inf-norms of S and S_M, m_S, m_M their longest rows, mu the
eigenvalues of S_M and u = 2^-53. With e = A^-1 S_M y - theta y, S y - lam S_M
y = -lam S e and ||e||_M = est theta ||y||_M, so a pair whose estimate is at or
below tol has resid <= tol N sqrt(mu_max / mu_min) up to rounding: held to
twice that. resid recomputed here in longdouble is held to twice the reported
one plus ((m_S + 2) N + |lam| (m_M + 2) N_M) u, the rounding bound of the
device's two f64 products. |lam_i - ref_i| <= resid_i ||y_i||2 / sqrt(mu_min) +
4 n u (N + ref_nev N_M) / mu_min against the i-th reference value IN ORDER: the
residual bound in the M^-1 norm plus the rounding of the dense reference; a
missed copy of a multiple eigenvalue shifts the list and breaks it. ||Y^T S_M Y
- I||max <= 2 tol. EigInfo.converged is the normwise backward error test resid
<= 2 tol (N + |lam| N_M) on a finite lam. The step counts are held to this
file's numpy emulation of the loop, with np.linalg.cholesky in the factor's
dtype as the factor, plus 2: the slack of test_gpu_nd_eig.py, for the same
reason (the nd factor sums in another order than the dense one)."""

import functools

import numpy as np
import pytest

import nd_support
from basic_sparse_matrix_amd import Csr, Dense, EigInfo, MatErr, _lib, cholesky_nd
from nd_support import _scale, assert_same, cols_of, csr_arrays, same_bits, start_block

pytestmark = pytest.mark.gpu

POISSON = ["g9-leaf1", "g11-leaf8", "g40-leaf256"]
SYSTEMS = POISSON + ["random"]
NCV = {"g9-leaf1": 80, "g11-leaf8": 60, "g40-leaf256": 60, "random": 160}
F32, F64 = np.float32, np.float64
NEV, BLOCK = 6, 4
TOL64, TOL32 = 2.0 ** -26, 2.0 ** -12
U = 2.0 ** -53
G11 = "g11-leaf8"


def _random_spd(seed, density, shift):
    rng = np.random.default_rng(seed)
    n = 300
    a = np.zeros((n, n))
    mask = rng.random((n, n)) < density
    vals = rng.uniform(-1.0, 1.0, (n, n))
    a[mask] = vals[mask]
    a = np.tril(a, -1)
    a = a + a.T
    a[np.arange(n), np.arange(n)] = np.abs(a).sum(axis=1) + shift(rng, n)
    return a


@functools.lru_cache(maxsize=None)
def _system(name):
    """(n, rp, ci, v as f64, leaf or None) of A, built once. `random` is this file's own: its diagonal is the row sum
    plus (1 + r) where nd_support's is (the row sum plus 1) plus r, so the two matrices differ in the last bit."""
    if name in POISSON:
        return nd_support.system(name)
    a = _random_spd(7, 0.02, lambda rng, n: 1.0 + rng.random(n))  # an irregular tree
    rp, ci, v = csr_arrays(a)
    return a.shape[0], rp, ci, v, None


@functools.lru_cache(maxsize=None)
def _mass(name, kind="consistent"):
    """(rp, ci, v as f64) of the mass matrix M that goes with system `name`."""
    n = _system(name)[0]
    if kind == "lumped":
        return csr_arrays(np.diag(np.random.default_rng(3).uniform(0.5, 2.0, n)))
    if kind == "identity":
        return csr_arrays(np.eye(n))
    if kind == "four":
        return csr_arrays(4.0 * np.eye(n))
    if kind == "minus":
        return csr_arrays(-np.eye(n))
    if name in POISSON:
        g = nd_support.POISSON[name][0]
        m1 = (np.diag(np.full(g, 4.0)) + np.diag(np.ones(g - 1), 1) + np.diag(np.ones(g - 1), -1)) / 6.0
        return csr_arrays(np.kron(m1, m1))
    return csr_arrays(_random_spd(11, 0.01, lambda rng, n: rng.uniform(0.5, 2.0, n)))


def _mirror(n, rp, ci, v, dtype):
    r = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    c = ci.astype(np.int64)
    low = np.zeros((n, n))
    keep = c <= r
    low[r[keep], c[keep]] = np.asarray(v).astype(dtype).astype(np.float64)[keep]
    out = low + np.tril(low, -1).T
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _truth(name, kind="consistent", dtype=F64):
    """S and S_M dense (of the values rounded to dtype), their inf-norms and longest rows, mu_min, mu_max and the
    generalised eigenvalues ascending."""
    from scipy.linalg import eigh

    n, rp, ci, v, _ = _system(name)
    S = _mirror(n, rp, ci, v, dtype)
    SM = _mirror(n, *_mass(name, kind), dtype)
    mu = np.linalg.eigvalsh(SM)
    return dict(S=S, SM=SM, n=n, N=float(np.abs(S).sum(axis=1).max()), NM=float(np.abs(SM).sum(axis=1).max()),
                mS=int((S != 0).sum(axis=1).max()), mM=int((SM != 0).sum(axis=1).max()), mu_min=float(mu[0]),
                mu_max=float(mu[-1]), ref=eigh(S, SM, eigvals_only=True))


def setup(monkeypatch, name):
    leaf = _system(name)[4]
    if leaf is not None:
        monkeypatch.setenv("BSM_ND_LEAF", leaf)


def matrix(name, dtype, v=None):
    """A fresh Csr (a fresh device handle) of A's pattern, with the system's values or v."""
    n, rp, ci, v0, _ = _system(name)
    return Csr.from_csr_arrays((n, n), rp, ci, np.asarray(v0 if v is None else v).astype(dtype))


def mass(name, dtype, kind="consistent"):
    n = _system(name)[0]
    rp, ci, v = _mass(name, kind)
    return Csr.from_csr_arrays((n, n), rp, ci, np.asarray(v).astype(dtype))


def parts(lam, y, info):
    return [lam] + (cols_of(y) if y is not None else []) + [info.resid, info.converged,
                                                           np.array([info.steps, info.ncv_used, info.exhausted,
                                                                     info.inexact])]


def assert_pairs(name, kind, lam, y, info, tol, what, dtype=F64, count=NEV):
    """The bounds of the module docstring on the `count` pairs of a run that asked for `count`."""
    t = _truth(name, kind, dtype)
    S, SM, n, N, NM = t["S"], t["SM"], t["n"], t["N"], t["NM"]
    ref = t["ref"]
    assert isinstance(info, EigInfo) and info.tol == tol and lam.dtype == np.float64 and lam.shape == (count,)
    Y = np.stack([np.asarray(c, np.float64) for c in cols_of(y)[:count]], axis=1)
    L = np.longdouble
    YL = np.asarray(Y, L)
    R = np.asarray(S, L) @ YL - (np.asarray(SM, L) @ YL) * np.asarray(lam, L)
    ynorm = np.sqrt((YL * YL).sum(axis=0))
    true = np.sqrt((R * R).sum(axis=0)) / ynorm
    orth = np.abs(Y.T @ SM @ Y - np.eye(count)).max()
    kappa = t["mu_max"] / t["mu_min"]
    print(f"{what} {name} {kind}: steps {info.steps} ncv_used {info.ncv_used} orth {orth:.3e} kappa(S_M) {kappa:.3f} "
          f"resid bound {2 * tol * N * np.sqrt(kappa):.3e}")
    for i in range(count):
        print(f"  pair {i}: lam {lam[i]:.16e} ref {ref[i]:.16e} resid {info.resid[i]:.3e} "
              f"longdouble {float(true[i]):.3e}")
    assert np.all(np.diff(lam) >= 0)
    assert not info.exhausted and not info.inexact
    for i in range(count):
        assert info.resid[i] <= 2 * tol * N * np.sqrt(kappa)
        assert float(true[i]) <= 2 * info.resid[i] + ((t["mS"] + 2) * N + abs(lam[i]) * (t["mM"] + 2) * NM) * U
        assert abs(lam[i] - ref[i]) <= (info.resid[i] * float(ynorm[i]) / np.sqrt(t["mu_min"])
                                        + 4 * n * U * (N + ref[count - 1] * NM) / t["mu_min"])
        assert bool(info.converged[i]) == bool(np.isfinite(lam[i]) and info.resid[i] <= 2 * tol * (N + abs(lam[i]) * NM))
        assert info.converged[i]
    assert orth <= 2 * tol


def c_info(f, A, M, nev, block, ncv, tol=0.0, seed=0):
    """(rc, lam, resid, info[4]) of bsm_nd_factor_eigsh_gen, values only; M may be None (a NULL m)."""
    lib = _lib.load()
    lam, resid, info = np.full(nev, 7.0), np.full(nev, 7.0), np.full(4, 7, dtype=np.uint32)
    rc = lib.bsm_nd_factor_eigsh_gen(f._h(), A._device().handle, M._device().handle if M is not None else None, nev,
                                     block, ncv, tol, seed, None, _lib.ptr(lam), None, _lib.ptr(resid),
                                     _lib.ptr(info))
    return rc, lam, resid, info


# ---- the loop in the S_M inner product, emulated: np.linalg.cholesky in the factor's dtype as the factor ----


@functools.lru_cache(maxsize=None)
def emulated_steps(name, kind, fdtype, ncv, tol=TOL64, nev=NEV, block=BLOCK, dtype=F64):
    """The Lanczos steps a numpy run of the library's generalised loop takes (dtype: a's and m's)."""
    from scipy.linalg import solve_triangular

    t = _truth(name, kind, dtype)
    S, SM, n, N = t["S"], t["SM"], t["n"], t["N"]
    Lf = np.linalg.cholesky(S.astype(fdtype))
    rtol = (t["mS"] + 2) * U

    def minv(v):
        s = _scale(v)
        y = solve_triangular(Lf, (v / s).astype(fdtype), lower=True)
        return s * solve_triangular(Lf.T, y, lower=False).astype(np.float64)

    def op(b):  # the refined solve, column by column, the block passed in a's dtype
        b = b.astype(dtype).astype(np.float64)
        x = minv(b)
        for _ in range(5):
            r = b - S @ x
            if np.abs(r).max() / (N * np.abs(x).max() + np.abs(b).max()) <= rtol:
                break
            x = x + minv(r)
        return x.astype(dtype).astype(np.float64)

    def cholqr2(W, norm2):
        try:
            R1 = np.linalg.cholesky(W.T @ SM @ W).T
        except np.linalg.LinAlgError:
            return None
        if np.any(np.diag(R1) ** 2 <= 2.0 ** -50 * norm2):
            return None
        W = W @ np.linalg.inv(R1)
        R2 = np.linalg.cholesky(W.T @ SM @ W).T
        return W @ np.linalg.inv(R2), R2 @ R1

    W = start_block(n, block, 0, dtype).astype(np.float64)
    V, _ = cholqr2(W, np.einsum("ij,ij->j", W, SM @ W))
    T = np.zeros((ncv, ncv))
    steps = 0
    while True:
        j = steps
        Uj = SM @ V[:, j * block:(j + 1) * block]
        W = np.stack([op(Uj[:, c]) for c in range(block)], axis=1)
        norm2 = np.einsum("ij,ij->j", W, SM @ W)
        a = np.zeros((block, block))
        for _ in range(2):
            C = V.T @ (SM @ W)
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


def assert_steps(info, emu, block, what):
    print(f"{what}: steps {info.steps}, emulation {emu}")
    assert info.steps <= emu + 2
    assert info.ncv_used == info.steps * block


# ---- convergence and accuracy ------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _default_run(name, fdtype):
    """(lam, Dense, info, C info) of the default call on the f64 matrices; the caller has set BSM_ND_LEAF."""
    A, M = matrix(name, F64), mass(name, F64)
    with cholesky_nd(A, factor_dtype=fdtype) as f:
        return f.eigsh(A, NEV, block=BLOCK, ncv=NCV[name], m=M) + (c_info(f, A, M, NEV, BLOCK, NCV[name]),)


@pytest.mark.parametrize("fdtype", [F64, F32], ids=["f64-factor", "f32-factor"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_smallest_pairs_with_a_consistent_mass_matrix(monkeypatch, name, fdtype):
    setup(monkeypatch, name)
    lam, y, info, (rc, clam, cresid, cinfo) = _default_run(name, fdtype)
    assert y.dtype == np.dtype(F64) and y.get_dims().cols == NEV and y.get_dims().rows == _system(name)[0]
    assert_pairs(name, "consistent", lam, y, info, TOL64, f"{np.dtype(fdtype).name} factor")
    assert rc == 0 and same_bits(clam, lam) and same_bits(cresid, info.resid)
    assert list(cinfo) == [info.steps, info.ncv_used, NEV, 0]  # info[2] == nev: every estimate is at or below tol
    assert_steps(info, emulated_steps(name, "consistent", fdtype, NCV[name]), BLOCK, f"{name} {np.dtype(fdtype).name}")


@pytest.mark.parametrize("fdtype", [F64, F32], ids=["f64-factor", "f32-factor"])
def test_lumped_mass(monkeypatch, fdtype):
    setup(monkeypatch, G11)
    A, M = matrix(G11, F64), mass(G11, F64, "lumped")
    with cholesky_nd(A, factor_dtype=fdtype) as f:
        lam, y, info = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], m=M)
    assert_pairs(G11, "lumped", lam, y, info, TOL64, "lumped")
    assert_steps(info, emulated_steps(G11, "lumped", fdtype, NCV[G11]), BLOCK, "lumped")


@pytest.mark.parametrize("kind,factor", [("identity", 1.0), ("four", 4.0)])
def test_a_multiple_of_the_identity_gives_eigsh_without_m(monkeypatch, kind, factor):
    setup(monkeypatch, G11)
    t = _truth(G11, kind)
    A, M = matrix(G11, F64), mass(G11, F64, kind)
    with cholesky_nd(A) as f:
        lam, y, info = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], m=M)
        lam0, _, info0 = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11])
    assert_pairs(G11, kind, lam, y, info, TOL64, kind)
    for i in range(NEV):
        print(f"  {kind} pair {i}: {factor} lam {factor * lam[i]:.16e} plain {lam0[i]:.16e}")
        assert abs(factor * lam[i] - lam0[i]) <= info.resid[i] + info0.resid[i] + 4 * t["n"] * U * t["N"]


def test_f32_matrices_with_an_f32_factor(monkeypatch):
    setup(monkeypatch, G11)
    A, M = matrix(G11, F32), mass(G11, F32)
    with cholesky_nd(A) as f:
        lam, y, info = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], m=M)
    assert y.dtype == np.dtype(F32) and info.tol == TOL32
    assert_pairs(G11, "consistent", lam, y, info, TOL32, "f32 matrices", dtype=F32)
    assert_steps(info, emulated_steps(G11, "consistent", F32, NCV[G11], tol=TOL32, dtype=F32), BLOCK, "f32 matrices")


@pytest.mark.parametrize("fdtype", [F64, F32], ids=["f64-factor", "f32-factor"])
def test_one_pair_one_vector_at_a_time(monkeypatch, fdtype):
    setup(monkeypatch, G11)
    A, M = matrix(G11, F64), mass(G11, F64)
    with cholesky_nd(A, factor_dtype=fdtype) as f:
        lam, y, info = f.eigsh(A, 1, block=1, ncv=NCV[G11], m=M)
    assert y.get_dims().cols == 1
    assert_pairs(G11, "consistent", lam, y, info, TOL64, "block 1", count=1)
    assert_steps(info, emulated_steps(G11, "consistent", fdtype, NCV[G11], nev=1, block=1), 1, "block 1")


# ---- bits --------------------------------------------------------------------------------------


def test_calls_repeat_v0_restates_the_seed_and_values_only(monkeypatch):
    setup(monkeypatch, G11)
    n = _system(G11)[0]
    A, M = matrix(G11, F64), mass(G11, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        want = parts(*f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], seed=3, m=M))
        assert_same(parts(*f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], seed=3, m=M)), want)
        v0 = start_block(n, BLOCK, seed=3)
        got = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], m=M,
                      v0=Dense.from_columns([v0[:, c].copy() for c in range(BLOCK)]))
        assert_same(parts(*got), want)
        lam_only, none, info_only = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], seed=3, m=M, vectors=False)
        assert none is None
        assert_same(parts(lam_only, None, info_only), [want[0]] + want[1 + NEV:])
        other = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], seed=4, m=M)  # another start: the same values, other bits
        assert not same_bits(other[0], want[0])


def test_the_upper_triangle_of_m_is_ignored(monkeypatch):
    setup(monkeypatch, G11)
    n = _system(G11)[0]
    rp, ci, v = _mass(G11)
    r = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    junk = np.where(ci.astype(np.int64) > r, 1e6 * (1.0 + np.arange(v.size)), v)
    A = matrix(G11, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        want = parts(*f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], m=mass(G11, F64)))
        got = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], m=Csr.from_csr_arrays((n, n), rp, ci, junk))
        assert_same(parts(*got), want)


@functools.lru_cache(maxsize=None)
def _g11_f32_factor_run():
    A, M = matrix(G11, F64), mass(G11, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        return f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], m=M)


@pytest.mark.parametrize("env", [{}, {"BSM_ND_FWD_TILES": "1", "BSM_ND_BWD_TILES": "1"}, {"BSM_ND_PLAIN": "1"}],
                         ids=["default", "tiles", "plain"])
def test_device_call_and_switches_have_the_default_host_calls_bits(monkeypatch, env):
    import torch

    from basic_sparse_matrix_amd import device

    setup(monkeypatch, G11)
    n = _system(G11)[0]
    want = parts(*_g11_f32_factor_run())  # made (or to be made now) without the switches
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    A, M = matrix(G11, F64), mass(G11, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        assert_same(parts(*f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], m=M)), want)
        mine = torch.full((n, NEV), 7.0, dtype=torch.float64, device="cuda")
        v0 = torch.from_numpy(start_block(n, BLOCK)).cuda().contiguous()
        lam, same, info = device.nd_factor_eigsh(f, A, NEV, block=BLOCK, ncv=NCV[G11], v0=v0, out=mine, m=M)
        assert same is mine
        got = mine.cpu().numpy()
        assert_same([lam] + [np.ascontiguousarray(got[:, j]) for j in range(NEV)] + parts(lam, None, info)[1:], want)
        lam3, none, info3 = device.nd_factor_eigsh(f, A, NEV, block=BLOCK, ncv=NCV[G11], vectors=False, m=M)
        assert none is None
        assert_same(parts(lam3, None, info3), [want[0]] + want[1 + NEV:])


def test_a_null_m_is_eigsh(monkeypatch):
    setup(monkeypatch, G11)
    A = matrix(G11, F64)
    with cholesky_nd(A, factor_dtype=F32) as f:
        lam, _, info = f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11])
        rc, clam, cresid, cinfo = c_info(f, A, None, NEV, BLOCK, NCV[G11])
    assert rc == 0 and same_bits(clam, lam) and same_bits(cresid, info.resid)
    assert list(cinfo)[:2] == [info.steps, info.ncv_used]


# ---- a mass matrix that is not positive definite, and the argument errors -----------------------


def test_m_not_positive_definite_and_bad_arguments(monkeypatch):
    setup(monkeypatch, G11)
    n = _system(G11)[0]
    A = matrix(G11, F64)
    empty = Csr.from_csr_arrays((n, n), np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0))
    with cholesky_nd(A, factor_dtype=F32) as f:
        for bad in (mass(G11, F64, "minus"), empty):
            with pytest.raises(_lib.BsmError, match="not positive definite"):
                f.eigsh(A, NEV, block=BLOCK, ncv=NCV[G11], m=bad)
            rc, lam, resid, info = c_info(f, A, bad, NEV, BLOCK, NCV[G11])
            assert rc == _lib.BSM_ERR_UNSUPPORTED and "not positive definite" in _lib.last_error()
            assert np.all(lam == 7.0) and np.all(resid == 7.0) and np.all(info == 7)
        lib = _lib.load()  # the vectors too keep their sentinel values
        lam, resid, info = np.full(NEV, 7.0), np.full(NEV, 7.0), np.full(4, 7, dtype=np.uint32)
        ycols = [np.full(n, 7.0) for _ in range(NEV)]
        minus = mass(G11, F64, "minus")
        rc = lib.bsm_nd_factor_eigsh_gen(f._h(), A._device().handle, minus._device().handle, NEV,
                                         BLOCK, NCV[G11], 0.0, 0, None, _lib.ptr(lam), _lib.ptr_array(ycols),
                                         _lib.ptr(resid), _lib.ptr(info))
        assert rc == _lib.BSM_ERR_UNSUPPORTED
        assert np.all(lam == 7.0) and np.all(resid == 7.0) and np.all(info == 7)
        assert all(np.all(c == 7.0) for c in ycols)
        with pytest.raises(TypeError, match="m "):
            f.eigsh(A, NEV, m=mass(G11, F32))
        with pytest.raises(TypeError, match="m "):
            f.eigsh(A, NEV, m=mass(G11, np.int32, "identity"))
        with pytest.raises(MatErr, match="IncorrectDimensions"):
            f.eigsh(A, NEV, m=mass("g9-leaf1", F64))
        # the library's own checks, behind the host-side ones
        rc, lam, resid, info = c_info(f, A, mass(G11, F32), NEV, BLOCK, NCV[G11])
        assert rc == _lib.BSM_ERR_INVALID and "dtype" in _lib.last_error()
        rc, lam, resid, info = c_info(f, A, mass("g9-leaf1", F64), NEV, BLOCK, NCV[G11])
        assert rc == _lib.BSM_ERR_DIMENSIONS
        assert np.all(lam == 7.0) and np.all(resid == 7.0) and np.all(info == 7)
