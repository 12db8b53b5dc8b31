"""Linear solver of the reference crate (src/lib.rs:11-65), on the GPU.

``solve(a, b)`` = cholesky_decomp -> transpose -> forward_substitution ->
backward_substitution, with the reference's exact operation order
(DESIGN.md "Solver"). The reference is ``f32``-only; ``f64`` is accepted as
this build's addition.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .dense import Dense
from .sparse import Csr, _raise_for
from .util import MatErr, MatErrKind, Panic

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _check_types(m: Csr, d: Dense, what: str):
    if m.dtype not in _FLOATS or d.dtype != m.dtype:
        raise TypeError(f"{what}: needs Csr<f32>/Dense<f32> (or f64), got {m.dtype}/{d.dtype}")


def _run(fn_name: str, m: Csr, rhs: Dense) -> Dense:
    dims = rhs.get_dims()
    n, k = dims.rows, dims.cols
    if m.dims.rows < n:
        raise Panic("index out of bounds: matrix has fewer rows than the right-hand side")
    b_cols = []
    for j in range(k):
        c = np.ascontiguousarray(rhs.get_col(j))
        if c.shape[0] < n:  # b.get_col(c)[row] / y.get_col(c)[row] for every row < n (lib.rs:33, :54)
            raise Panic(f"index out of bounds: the len is {c.shape[0]} but the index is {c.shape[0]}")
        b_cols.append(np.ascontiguousarray(c[:n]))
    dev = m._device()
    lib = _lib.require_device()
    out = Dense.new_default_with_dims(k, n, dtype=m.dtype)
    _raise_for(getattr(lib, fn_name)(dev.handle, k, n, _lib.ptr_array(b_cols), _lib.ptr_array(out.data)))
    return out


def forward_substitution(l: Csr, b: Dense) -> Dense:
    """lib.rs:28-46: solve L y = b (diagonal = LAST stored entry of each row)."""
    _check_types(l, b, "forward_substitution")
    return _run("bsm_forward_substitution", l, b)


def backward_substitution(l_star: Csr, y: Dense) -> Dense:
    """lib.rs:49-65: solve L* x = y (diagonal = FIRST stored entry of each row)."""
    _check_types(l_star, y, "backward_substitution")
    return _run("bsm_backward_substitution", l_star, y)


def solve(a: Csr, b: Dense, *, order: str = "reference") -> Dense:
    """lib.rs:11-24. Non-square ``a`` panics (``cholesky_decomp().unwrap()``).

    ``order="reference"`` (default) keeps the reference's operation order:
    bit-exact. ``order="blocked"`` reassociates the two triangular solves
    (64-row blocks, precomputed inverse diagonal blocks; ``bsm_solve_blocked``):
    not bit-exact, within the north star's 1e-6 relative f64 tolerance, and
    ~100x faster on C5's triangular solves. This keyword is this build's
    addition; the reference has one order.

    ``order="nd"`` factors P A P^T instead, P a nested-dissection order of
    A's graph (``bsm_solve_nd``: the host bisects the graph, the device
    factors the separator tree's dense fronts level by level): a wide
    elimination tree with far fewer flops than the band on 2-D meshes; also
    within the 1e-6 relative f64 tolerance, not bit-exact."""
    _check_types(a, b, "solve")
    if a.dims.rows != a.dims.cols:
        raise Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix")
    fns = {"reference": "bsm_solve", "blocked": "bsm_solve_blocked", "nd": "bsm_solve_nd"}
    if order not in fns:
        raise ValueError(f"solve: order must be 'reference', 'blocked' or 'nd', got {order!r}")
    return _run(fns[order], a, b)


ND_SYSTEMS = {"A": 0, "L": 1, "Lt": 2}  # BSM_ND_SYS_A / _L / _LT


def nd_system_code(system: str) -> int:
    if system not in ND_SYSTEMS:
        raise ValueError(f"NdFactor.solve: system must be 'A', 'L' or 'Lt', got {system!r}")
    return ND_SYSTEMS[system]


def _check_factorable(a: Csr, what: str):
    if a.dtype not in _FLOATS:
        raise TypeError(f"{what}: needs Csr<f32> (or f64), got {a.dtype}")
    if a.dims.rows != a.dims.cols:
        raise Panic("called `Result::unwrap()` on an `Err` value: NonSquareMatrix")


@dataclass
class RefineInfo:
    """What a refined solve reports per right-hand column: the corrections
    made, the backward error of the returned iterate, whether it is at or
    below ``tol``, and the ``tol`` that was used."""

    iters: np.ndarray  # uint32 [k]
    berr: np.ndarray  # float64 [k]
    converged: np.ndarray  # bool [k]
    tol: float


@dataclass
class PartialInfo:
    """What ``NdFactor.refactor_partial`` reports: the fronts factored again,
    the fronts in the plan, and the changed entries (as named, or as found
    with ``since=``)."""

    fronts: int
    total_fronts: int
    changed: int


@dataclass
class PcgInfo:
    """What a pcg solve reports per right-hand column: the CG steps made, the
    backward error of the returned ``x`` (of its true residual), whether it
    is at or below ``tol``, whether the column broke down (``S`` or the
    factor not positive definite), and the ``tol`` that was used."""

    iters: np.ndarray  # uint32 [k]
    berr: np.ndarray  # float64 [k]
    converged: np.ndarray  # bool [k]
    breakdown: np.ndarray  # bool [k]
    tol: float


@dataclass
class EigInfo:
    """What ``eigsh`` reports: the Lanczos steps made, the basis columns used,
    the true residuals ``||S y - lam y||2 / ||y||2`` per pair, which pairs
    have converged (a finite ``lam`` whose true residual is within ``2 tol
    ||S||inf``, the bound a pair with ``est <= tol`` meets with a factor of
    two for rounding), whether the block lost rank (the Krylov space is
    invariant), whether a solve ended above the refined solve's ``tol``, and
    the ``tol`` that was used."""

    steps: int
    ncv_used: int
    resid: np.ndarray  # float64 [nev]
    converged: np.ndarray  # bool [nev]
    exhausted: bool
    inexact: bool
    tol: float


def refine_default_tol(a: Csr) -> float:
    """``(m + 2) 2^-53`` with ``m`` the longest row of ``a``'s lower triangle
    mirrored: the rounding bound of the f64 residual itself, the library's
    default for ``tol == 0``."""
    rp, ci, _ = a._csr_arrays()
    n = a.dims.rows
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    cols = ci.astype(np.int64)
    m = np.bincount(rows[cols <= rows], minlength=n) + np.bincount(cols[cols < rows], minlength=n)
    return float((int(m.max()) if n else 0) + 2) * 2.0 ** -53


def check_refine_args(a: Csr, b_dtype, max_iter, tol, what: str) -> None:
    """The host-side checks the refined solves share."""
    if a.dtype not in _FLOATS:
        raise TypeError(f"{what}: needs Csr<f32> (or f64), got {a.dtype}")
    if np.dtype(b_dtype) != a.dtype:
        raise TypeError(f"{what}: b must have a's dtype {a.dtype}, got {np.dtype(b_dtype)}")
    if int(max_iter) != max_iter or max_iter < 0:
        raise ValueError(f"{what}: max_iter must be an integer >= 0, got {max_iter!r}")
    if tol is not None and not tol > 0:  # a NaN is refused here too
        raise ValueError(f"{what}: tol must be > 0 (None = the default), got {tol!r}")


def sym_norm_inf(a: Csr, dev=None) -> float:
    """``||S||inf`` of ``a``'s lower triangle mirrored, computed once per
    device handle when one is given."""
    if dev is not None and dev.sym_norm_inf is not None:
        return dev.sym_norm_inf
    rp, ci, v = a._csr_arrays()
    n = a.dims.rows
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    cols = ci.astype(np.int64)
    av = np.abs(np.asarray(v, dtype=np.float64))
    low, strict = cols <= rows, cols < rows
    sums = np.bincount(rows[low], weights=av[low], minlength=n) + np.bincount(cols[strict], weights=av[strict],
                                                                               minlength=n)
    out = float(sums.max()) if n else 0.0
    if dev is not None:
        dev.sym_norm_inf = out
    return out


EIG_MAX_BLOCK = 32
EIG_DEFAULT_NCV = 128


def check_eig_args(a: Csr, n: int, nev, block, ncv, tol, seed, what: str) -> tuple[int, float]:
    """The host-side checks ``eigsh`` and ``device.nd_factor_eigsh`` share;
    returns the basis size and the ``tol`` in use."""
    if a.dtype not in _FLOATS:
        raise TypeError(f"{what}: needs Csr<f32> (or f64), got {a.dtype}")
    if a.dims.rows != n or a.dims.cols != n:
        raise MatErr(MatErrKind.IncorrectDimensions)
    if int(nev) != nev or nev < 1:
        raise ValueError(f"{what}: nev must be an integer >= 1, got {nev!r}")
    if int(block) != block or not 1 <= block <= EIG_MAX_BLOCK:
        raise ValueError(f"{what}: block must be an integer in 1..{EIG_MAX_BLOCK}, got {block!r}")
    if ncv is not None and (int(ncv) != ncv or ncv < 1):
        raise ValueError(f"{what}: ncv must be an integer >= 1 (None = min(n, {EIG_DEFAULT_NCV})), got {ncv!r}")
    if tol is not None and not tol > 0:  # a NaN is refused here too
        raise ValueError(f"{what}: tol must be > 0 (None = the default), got {tol!r}")
    if int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{what}: seed must be an integer in 0..2^64-1, got {seed!r}")
    m = (min(n, EIG_DEFAULT_NCV) if ncv is None else int(ncv)) // int(block) * int(block)
    if n and not nev <= m <= n:
        raise ValueError(f"{what}: ncv (rounded down to a multiple of block: {m}) must be in nev..n = {nev}..{n}")
    return m, float(tol) if tol is not None else (2.0 ** -26 if a.dtype == np.float64 else 2.0 ** -12)


def check_eig_mass(a: Csr, m: Csr, n: int, what: str) -> None:
    """The host-side checks of ``eigsh``'s mass matrix ``m`` against ``a``."""
    if not isinstance(m, Csr):
        raise TypeError(f"{what}: m must be a Csr, got {type(m).__name__}")
    if m.dtype != a.dtype:
        raise TypeError(f"{what}: m must have a's dtype {a.dtype}, got {m.dtype}")
    if m.dims.rows != n or m.dims.cols != n:
        raise MatErr(MatErrKind.IncorrectDimensions)


def eig_info(a: Csr, dev, lam, resid, info, tol_used, m: Csr | None = None, mdev=None) -> EigInfo:
    """``EigInfo`` of a call's results. ``converged`` is ``resid <= 2 tol
    ||S||inf`` on a finite ``lam``; with a mass matrix ``m`` it is the
    normwise backward error test ``resid <= 2 tol (||S||inf + |lam|
    ||S_M||inf)``."""
    bound = 2.0 * tol_used * sym_norm_inf(a, dev)
    if m is not None:
        with np.errstate(invalid="ignore"):
            bound = 2.0 * tol_used * (sym_norm_inf(a, dev) + np.abs(lam) * sym_norm_inf(m, mdev))
    with np.errstate(invalid="ignore"):
        conv = np.isfinite(lam) & (resid <= bound)
    return EigInfo(int(info[0]), int(info[1]), resid, conv, bool(info[3] & 1), bool(info[3] & 2), tol_used)


def refine_tol_in_use(a: Csr, dev, tol) -> float:
    """``tol``, or the default for ``a``, computed once per device handle."""
    if tol is not None:
        return float(tol)
    if dev.refine_tol is None:
        dev.refine_tol = refine_default_tol(a)
    return dev.refine_tol


class NdFactor:
    """The nested-dissection Cholesky factor of ``P A P^T``, kept on the
    device (``bsm_nd_factor``): factor once with :func:`cholesky_nd`, then
    ``solve`` as often as wanted (``A``, ``L`` or ``L^T``), read ``L`` or
    ``logdet()`` out, and ``refactor`` new values of the same pattern in
    place (``refactor_partial`` where only a few entries changed;
    ``device.nd_factor_solve`` solves on device tensors), and read the
    selected inverse (``inv_diag()``, ``inv_entries()``, ``inv_on()``:
    ``A^-1`` on the pattern of ``L + L^T``). ``solve_refined`` refines a
    solve with f64 residuals and reports its backward error, ``solve_pcg``
    uses the factor as the preconditioner of conjugate gradients; the factor's
    dtype may be chosen apart from the matrix's
    (``cholesky_nd(a, factor_dtype=...)``). ``refactor_values`` refactors from
    a device tensor of values, and ``autograd.nd_solve`` / ``autograd.nd_logdet``
    differentiate the solve and the log-determinant. A factor made with
    ``cholesky_nd(a, schur=idx)`` also gives the Schur complement on those
    vertices (``schur``, ``schur_condense``, ``schur_expand``). The handle owns its
    numeric storage (``nbytes``; ~5.6 GB at C5 in f64) until ``close()``, the
    end of a ``with`` block, or garbage collection. This build's addition."""

    __slots__ = ("handle", "n", "dtype", "src_dtype", "_pattern_nnz", "_epoch", "_vals_key", "_vals_ref",
                 "_grad_weights")

    def __init__(self, handle: int, src_dtype=None):
        lib = _lib.load()
        self.handle = handle
        n, d = ctypes.c_uint64(), ctypes.c_int()
        _lib.check(lib.bsm_nd_factor_info(handle, ctypes.byref(n), ctypes.byref(d), None, None))
        self.n = n.value
        self.dtype = _lib.CODE_DTYPES[d.value]
        # the factored matrix's dtype (update / downdate take W in it)
        self.src_dtype = self.dtype if src_dtype is None else np.dtype(src_dtype)
        nnz = ctypes.c_uint64()
        _lib.check(lib.bsm_nd_factor_pattern_info(handle, ctypes.byref(nnz), None))
        self._pattern_nnz = nnz.value
        self._epoch = 0  # counts the calls that rewrite the factor (autograd.py: a backward after one is refused)
        self._vals_key = None  # refactor_values' record of the device values this is the factor of
        self._vals_ref = None  # ... and those values, kept so that their address stays theirs
        self._grad_weights = None  # autograd.nd_logdet's 0 / 1 / 2 per stored entry, built once

    @property
    def pattern_nnz(self) -> int:
        """Stored entries of the factored pattern (both triangles): the length
        of ``refactor_values``' ``vals`` and of ``device.nd_factor_inv_pattern``'s
        result (``bsm_nd_factor_pattern_info``). It never changes."""
        return self._pattern_nnz

    def _bump_epoch(self) -> None:
        self._epoch = getattr(self, "_epoch", 0) + 1
        self._vals_key = self._vals_ref = None

    def refactor_values(self, vals) -> None:
        """``refactor`` from a device tensor of values in the factored
        pattern's storage order: ``device.nd_factor_refactor_values(self,
        vals)``, which needs torch."""
        from .device import nd_factor_refactor_values

        nd_factor_refactor_values(self, vals)

    def _h(self) -> int:
        if not self.handle:
            raise ValueError("NdFactor: used after close()")
        return self.handle

    def solve(self, b: Dense, *, system: str = "A") -> Dense:
        """``x = A^-1 b`` for the columns of ``b``: the forward and backward
        passes only. Column ``j`` has the bits of ``solve(a, b, order="nd")``'s
        (for one column: of that solve with ``BSM_ND_FOLD=0``).

        ``system="L"`` solves ``L y = b`` (the forward pass alone) and
        ``system="Lt"`` solves ``L^T x = y`` (the backward pass alone), with
        ``b``, ``y`` and ``x`` in the NEW order (``perm``, ``l()``): nothing
        is permuted, so ``x[perm] = Lt(L(b[perm]))`` has the bits of
        ``system="A"``."""
        sys_code = nd_system_code(system)
        dims = b.get_dims()
        n, k = dims.rows, dims.cols
        if k and b.dtype != self.dtype:
            raise TypeError(f"NdFactor.solve: needs Dense<{self.dtype}>, got {b.dtype}")
        b_cols = []
        for j in range(k):
            c = np.ascontiguousarray(b.get_col(j))
            if c.shape[0] < n:
                raise Panic(f"index out of bounds: the len is {c.shape[0]} but the index is {c.shape[0]}")
            b_cols.append(np.ascontiguousarray(c[:n]))
        lib = _lib.require_device()
        out = Dense.new_default_with_dims(k, n, dtype=self.dtype)
        _raise_for(lib.bsm_nd_factor_solve_system(self._h(), sys_code, k, n, _lib.ptr_array(b_cols),
                                                  _lib.ptr_array(out.data)))
        return out

    def solve_refined(self, a: Csr, b: Dense, *, max_iter: int = 5, tol: float | None = None):
        """Iterative refinement on this factor (``bsm_nd_factor_solve_refined``):
        ``x_0 = M^-1 b`` by the factor, then up to ``max_iter`` corrections
        from residuals ``b - S x`` formed in f64, each column on its own.
        ``a`` is the system's matrix (f32 or f64; its lower triangle mirrored,
        as the factor reads it), ``b`` a ``Dense`` of ``a``'s dtype; the factor
        may have either dtype, and ``a`` may be the factored matrix or one
        near it. Returns ``(x, RefineInfo)``: ``x`` of ``a``'s dtype, the
        iterate with the smallest backward error ``berr``, after ``iters``
        corrections. ``tol=None`` is the default ``(m + 2) 2^-53``, ``m`` the
        longest row of the mirrored matrix. An f32 factor of an f64 matrix
        (``cholesky_nd(a, factor_dtype=np.float32)``) reaches f64 backward
        error in two or three corrections."""
        h = self._h()
        dims = b.get_dims()
        n, k = dims.rows, dims.cols
        check_refine_args(a, b.dtype if k else a.dtype, max_iter, tol, "NdFactor.solve_refined")
        if a.dims.rows != self.n or a.dims.cols != self.n or n != self.n:
            raise MatErr(MatErrKind.IncorrectDimensions)
        b_cols = []
        for j in range(k):
            c = np.ascontiguousarray(b.get_col(j))
            if c.shape[0] < n:
                raise Panic(f"index out of bounds: the len is {c.shape[0]} but the index is {c.shape[0]}")
            b_cols.append(np.ascontiguousarray(c[:n]))
        dev = a._device()
        tol_used = refine_tol_in_use(a, dev, tol)
        lib = _lib.require_device()
        out = Dense.new_default_with_dims(k, n, dtype=a.dtype)
        iters = np.zeros(k, dtype=np.uint32)
        berr = np.zeros(k, dtype=np.float64)
        _raise_for(lib.bsm_nd_factor_solve_refined(h, dev.handle, k, n, _lib.ptr_array(b_cols),
                                                   _lib.ptr_array(out.data), max_iter, tol_used, _lib.ptr(iters),
                                                   _lib.ptr(berr)))
        return out, RefineInfo(iters, berr, berr <= tol_used, tol_used)

    def solve_pcg(self, a: Csr, b: Dense, *, max_iter: int = 50, tol: float | None = None):
        """Preconditioned conjugate gradients on this factor
        (``bsm_nd_factor_solve_pcg``): ``S x = b`` with the factor's solve as
        preconditioner, each column its own CG, everything but that solve in
        f64. ``a``, ``b`` and ``tol`` are ``solve_refined``'s, and so is the
        first iterate; where refinement needs ``a`` close to the factored
        matrix, this converges for any positive definite ``a`` (a stale
        factor, ``3 A``, a low-rank change) in at most ``max_iter`` steps.
        Returns ``(x, PcgInfo)``: ``berr`` is the backward error of ``x``'s
        true residual, ``breakdown`` marks a column on which ``a`` or the
        factor proved not positive definite (its ``x`` is that of its last
        completed step)."""
        h = self._h()
        dims = b.get_dims()
        n, k = dims.rows, dims.cols
        check_refine_args(a, b.dtype if k else a.dtype, max_iter, tol, "NdFactor.solve_pcg")
        if a.dims.rows != self.n or a.dims.cols != self.n or n != self.n:
            raise MatErr(MatErrKind.IncorrectDimensions)
        b_cols = []
        for j in range(k):
            c = np.ascontiguousarray(b.get_col(j))
            if c.shape[0] < n:
                raise Panic(f"index out of bounds: the len is {c.shape[0]} but the index is {c.shape[0]}")
            b_cols.append(np.ascontiguousarray(c[:n]))
        dev = a._device()
        tol_used = refine_tol_in_use(a, dev, tol)
        lib = _lib.require_device()
        out = Dense.new_default_with_dims(k, n, dtype=a.dtype)
        iters = np.zeros(k, dtype=np.uint32)
        berr = np.zeros(k, dtype=np.float64)
        flags = np.zeros(k, dtype=np.uint32)
        _raise_for(lib.bsm_nd_factor_solve_pcg(h, dev.handle, k, n, _lib.ptr_array(b_cols), _lib.ptr_array(out.data),
                                               max_iter, tol_used, _lib.ptr(iters), _lib.ptr(berr), _lib.ptr(flags)))
        return out, PcgInfo(iters, berr, berr <= tol_used, (flags & 1) != 0, tol_used)

    def eigsh(self, a: Csr, nev: int, block: int = 4, ncv: int | None = None, tol: float | None = None,
              v0: Dense | None = None, seed: int = 0, *, vectors: bool = True, m: Csr | None = None):
        """The ``nev`` smallest eigenvalues of ``S`` (``a``'s lower triangle
        mirrored, as ``solve_refined`` defines it) and their eigenvectors, by
        block shift-invert Lanczos on this factor (``bsm_nd_factor_eigsh``):
        the operator is ``A^-1`` by the refined solve, ``block`` columns at a
        time, with full reorthogonalisation, in a basis of at most ``ncv``
        columns (rounded down to a multiple of ``block``; ``None``:
        ``min(n, 128)``). ``tol`` bounds the residual estimate of a Ritz pair
        (``None``: ``2^-26`` for an f64 ``a``, ``2^-12`` for an f32 one);
        ``v0`` is a start block (a ``Dense`` of ``a``'s dtype, ``n x block``),
        else it is generated from ``seed``. Returns ``(lam, Dense, EigInfo)``:
        ``lam`` ascending (f64), the unit eigenvectors as the columns of a
        ``Dense`` of ``a``'s dtype (``None`` with ``vectors=False``). Pairs
        that the basis could not give (an ``exhausted`` run) have ``lam`` NaN.
        There is no restart: call again with ``v0`` made of the first
        ``block`` vectors and a larger ``ncv``. An eigenvalue of multiplicity
        above ``block`` is found ``block`` times at most (a long run may pick
        up a further copy from rounding; do not count on it).

        ``m`` (keyword only): a mass matrix, for the generalised problem ``S y
        = lam S_M y`` of finite elements and volumes (``bsm_nd_factor_eigsh_gen``;
        SciPy's ``eigsh(A, k, M=m, sigma=0)``). ``m`` is an ``n x n`` ``Csr`` of
        ``a``'s dtype with any pattern; ``S_M`` is its lower triangle mirrored
        and must be positive definite (else the call raises, "m is not
        positive definite"). The loop is the same in the ``S_M`` inner
        product; the vectors are normalised to ``y^T S_M y = 1`` and
        ``EigInfo.resid`` is ``||S y - lam S_M y||2 / ||y||2``. The loop stops
        on the estimates ``est <= tol``, which bound ``resid`` by ``tol
        ||S||inf sqrt(mu_max / mu_min)`` (``mu``: the extreme eigenvalues of
        ``S_M``), while ``EigInfo.converged`` is the normwise backward error
        test ``resid <= 2 tol (||S||inf + |lam| ||S_M||inf)``: for an
        ill-conditioned ``m`` a smaller ``tol`` may be needed for
        ``converged``. Without ``m`` the call is unchanged."""
        h = self._h()
        n = self.n
        ncv_use, tol_used = check_eig_args(a, n, nev, block, ncv, tol, seed, "NdFactor.eigsh")
        if m is not None:
            check_eig_mass(a, m, n, "NdFactor.eigsh")
        v0_cols = None
        if v0 is not None:
            dims = v0.get_dims()
            if v0.dtype != a.dtype:
                raise TypeError(f"NdFactor.eigsh: v0 must have a's dtype {a.dtype}, got {v0.dtype}")
            if dims.rows != n or dims.cols != block:
                raise MatErr(MatErrKind.IncorrectDimensions)
            v0_cols = []
            for j in range(block):
                c = np.ascontiguousarray(v0.get_col(j))
                if c.shape[0] < n:
                    raise Panic(f"index out of bounds: the len is {c.shape[0]} but the index is {c.shape[0]}")
                v0_cols.append(np.ascontiguousarray(c[:n]))
        if n == 0:
            nev = 0
        lam = np.zeros(nev, dtype=np.float64)
        resid = np.zeros(nev, dtype=np.float64)
        info = np.zeros(4, dtype=np.uint32)
        out = Dense.new_default_with_dims(nev, n, dtype=a.dtype) if vectors else None
        dev = a._device()
        mdev = m._device() if m is not None else None
        if n:
            lib = _lib.require_device()
            v0_p = _lib.ptr_array(v0_cols) if v0_cols is not None else None
            out_p = _lib.ptr_array(out.data) if vectors else None
            if m is None:
                _raise_for(lib.bsm_nd_factor_eigsh(h, dev.handle, nev, block, ncv_use, tol_used, seed, v0_p,
                                                   _lib.ptr(lam), out_p, _lib.ptr(resid), _lib.ptr(info)))
            else:
                _raise_for(lib.bsm_nd_factor_eigsh_gen(h, dev.handle, mdev.handle, nev, block, ncv_use, tol_used,
                                                       seed, v0_p, _lib.ptr(lam), out_p, _lib.ptr(resid),
                                                       _lib.ptr(info)))
        return lam, out, eig_info(a, dev, lam, resid, info, tol_used, m, mdev)

    def refactor(self, a: Csr) -> None:
        """New values on the same pattern (``bsm_nd_factor_refactor``): the
        numeric factor alone, into this handle's storage, on the plan fixed
        when the factor was made. Afterwards the factor has the bits of
        ``cholesky_nd(a)``. ``a`` must have the factored matrix's dtype, shape
        and pattern (else the error for ``BSM_ERR_INVALID``, the factor
        untouched). Values that are not positive definite raise as
        :func:`cholesky_nd` does and leave the handle WITHOUT a factor: until
        a later ``refactor`` succeeds, ``solve``, ``l()``, ``l_star()`` and
        ``logdet()`` raise; ``perm`` and ``nbytes`` still answer."""
        _check_factorable(a, "NdFactor.refactor")
        h = self._h()
        dev = a._device()
        self._bump_epoch()
        _raise_for(_lib.require_device().bsm_nd_factor_refactor(h, dev.handle))

    def refactor_partial(self, a: Csr, rows=None, cols=None, *, since: Csr | None = None) -> PartialInfo:
        """New values at a FEW places of the factored pattern
        (``bsm_nd_factor_refactor_partial``): only the fronts on the paths
        from the changed entries to the roots of the separator tree are
        factored again, and the factor has the bits ``refactor(a)`` gives.
        Give exactly one of

        * ``rows, cols``: the changed positions as two equally long 1-D
          integer sequences, any order, ``(j, i)`` as good as ``(i, j)``,
          repeats allowed; every pair must be a stored entry of ``a``;
        * ``since=a_old``: the matrix this is the factor of; the stored
          entries with ``col <= row`` whose bits differ are found on the
          device (``bsm_nd_factor_refactor_since``).

        ``a`` equals the factored matrix in every other stored entry with
        ``col <= row``; a changed entry that is not named gives an
        unspecified factor. After ``update`` / ``downdate`` the call raises
        the error for ``BSM_ERR_UNSUPPORTED`` until a ``refactor``. Pattern,
        shape and dtype are checked as ``refactor`` checks them; a pair that
        is not stored raises the error for ``BSM_ERR_INVALID``, an index
        ``>= n`` ``MatErr(OutOfBounds)``, all with the factor untouched.
        Values that are not positive definite leave the handle without a
        factor, as a failed ``refactor`` does. Returns
        :class:`PartialInfo`."""
        what = "NdFactor.refactor_partial"
        named = rows is not None or cols is not None
        if named == (since is not None):
            raise ValueError(f"{what}: give exactly one of (rows, cols) and since=")
        _check_factorable(a, what)
        h = self._h()
        info = np.zeros(3, dtype=np.uint64)
        lib = _lib.require_device
        if since is not None:
            if not isinstance(since, Csr):
                raise TypeError(f"{what}: since must be a Csr, got {type(since).__name__}")
            _check_factorable(since, what)
            if since.dtype != a.dtype:
                raise TypeError(f"{what}: since is Csr<{since.dtype}>, a is Csr<{a.dtype}>")
            self._bump_epoch()
            _raise_for(lib().bsm_nd_factor_refactor_since(h, since._device().handle, a._device().handle,
                                                          _lib.ptr(info)))
        else:
            if rows is None or cols is None:
                raise ValueError(f"{what}: rows and cols go together")
            r = self._rows_arg("refactor_partial", "rows", rows)
            c = self._rows_arg("refactor_partial", "cols", cols)
            if r.shape[0] != c.shape[0]:
                raise ValueError(f"{what}: rows has {r.shape[0]} entries, cols {c.shape[0]}")
            nc = r.shape[0]
            self._bump_epoch()
            _raise_for(lib().bsm_nd_factor_refactor_partial(h, a._device().handle, nc, _lib.ptr(r) if nc else None,
                                                            _lib.ptr(c) if nc else None, _lib.ptr(info)))
        return PartialInfo(int(info[0]), int(info[1]), int(info[2]))

    def _updown(self, w: Csr, sign: int, what: str) -> None:
        h = self._h()
        if w.dims.rows != self.n:
            raise MatErr(MatErrKind.IncorrectDimensions)
        want = self.src_dtype
        if w.dtype != want:
            raise TypeError(f"NdFactor.{what}: needs Csr<{want}> (the factored matrix's dtype), got {w.dtype}")
        k = w.dims.cols
        rp, ci, v = w._csr_arrays()
        rows = np.repeat(np.arange(self.n, dtype=np.uint64), np.diff(np.asarray(rp).astype(np.int64)))
        cols = np.asarray(ci).astype(np.int64)
        order = np.argsort(cols, kind="stable")  # column-compressed: rows stay ascending within a column
        col_ptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=k))]).astype(np.uint64)
        r = np.ascontiguousarray(rows[order])
        vals = np.ascontiguousarray(np.asarray(v, dtype=want)[order])
        self._bump_epoch()
        _raise_for(_lib.require_device().bsm_nd_factor_updown(h, sign, k, _lib.ptr(col_ptr), _lib.ptr(r),
                                                              _lib.ptr(vals)))

    def update(self, w: Csr) -> None:
        """The factor of ``P (S + W W^T) P^T`` in place
        (``bsm_nd_factor_updown``), ``S`` the matrix this was the factor of
        and ``w`` a ``Csr`` of shape ``n x k``, ``1 <= k <= 16``, of the
        FACTORED MATRIX's dtype (else ``TypeError``; another row count raises
        ``MatErr(IncorrectDimensions)``). Only the fronts on the paths from
        ``w``'s columns to the root of the separator tree are rewritten: a
        few launches instead of a ``refactor``. Afterwards ``solve``,
        ``logdet``, ``l()``, the selected inverse, ``solve_refined``,
        ``solve_pcg`` and ``eigsh`` see the new factor, and ``nnz_l`` is 0
        until the next ``l()``.

        Which columns are inside: take a column's entry whose vertex comes
        first in the new order (``perm``), in tree node ``N``; every other
        entry must be one of ``N``'s own columns or front rows. Always inside:
        a diagonal column ``alpha e_i``, and a vertex together with any of its
        neighbours in ``S``'s graph that come LATER in the new order (an edge
        ``sqrt(c) (e_i - e_j)`` of a stored ``(i, j)``; an element's clique
        seen from its first vertex). A column outside raises the error for
        ``BSM_ERR_INVALID`` naming how many columns and the first one, before
        anything is written; a row ``>= n`` raises ``MatErr(OutOfBounds)``,
        ``k > 16`` the error for ``BSM_ERR_UNSUPPORTED``. Stored zeros and
        empty columns are no-ops. The same call on the same factor gives the
        same bits."""
        self._updown(w, 1, "update")

    def downdate(self, w: Csr) -> None:
        """The factor of ``P (S - W W^T) P^T`` in place: :meth:`update`'s
        arguments and errors. A ``w`` that leaves the matrix not positive
        definite raises as :func:`cholesky_nd` does, found by a dry pass that
        writes only scratch: the factor keeps its bits and stays valid."""
        self._updown(w, -1, "downdate")

    @staticmethod
    def _rows_arg(what: str, name: str, x) -> np.ndarray:
        r = np.asarray(x)
        if r.ndim != 1:
            raise ValueError(f"NdFactor.{what}: {name} must be 1-D, got {r.shape}")
        if r.size and not np.issubdtype(r.dtype, np.integer):
            raise TypeError(f"NdFactor.{what}: {name} must be integers, got {r.dtype}")
        if r.size and int(r.min()) < 0:
            raise ValueError(f"NdFactor.{what}: {name} has a negative index")
        return np.ascontiguousarray(r, dtype=np.uint64)

    def _solve_sparse(self, k: int, col_ptr, b_rows, vals, rows):
        """``bsm_nd_factor_solve_sparse``: (the k result columns, info)."""
        h = self._h()
        nout = self.n if rows is None else rows.shape[0]
        cols = [np.zeros(nout, dtype=self.dtype) for _ in range(k)]
        info = np.zeros(4, dtype=np.uint32)
        if k and nout:  # an empty ``rows`` would read as NULL ("every row") on the other side
            lib = _lib.require_device()
            _raise_for(lib.bsm_nd_factor_solve_sparse(h, k, _lib.ptr(col_ptr), _lib.ptr(b_rows), _lib.ptr(vals),
                                                      0 if rows is None else nout,
                                                      None if rows is None else _lib.ptr(rows),
                                                      _lib.ptr_array(cols), _lib.ptr(info)))
        return cols, tuple(int(v) for v in info)

    def solve_sparse(self, b: Csr, rows=None, *, info: bool = False):
        """``x = A^-1 b`` for a SPARSE ``b`` (``bsm_nd_factor_solve_sparse``),
        with ``x`` wanted at ``rows`` only: a Green's function between two
        points, an effective resistance, a covariance ``(A^-1)[i, j]`` off the
        pattern of ``L + L^T``. ``b`` is a ``Csr`` of shape ``n x k`` of the
        FACTOR's dtype (else ``TypeError``; another row count raises
        ``MatErr(IncorrectDimensions)``); ``rows`` a 1-D integer array-like
        (A's order, unsorted and repeated as you like; not 1-D or negative:
        ``ValueError``, not integers: ``TypeError``, ``>= n``:
        ``MatErr(OutOfBounds)``), or ``None`` for every row. Returns a
        ``Dense`` of shape ``len(rows) x k`` (``n x k``): row ``e`` is
        ``x[rows[e]]``.

        Only the fronts on the paths from ``b``'s entries to the root of the
        separator tree run the forward pass and only those from the fronts
        owning ``rows`` the backward pass (15 and 14 of 15,397 at C5 for a point
        source and one row), with the dense solve's operations in its order:
        every value EQUALS ``solve``'s on the densified ``b`` (``np.array_equal``;
        a zero may differ in sign), whatever else is asked for in the same
        call. Stored zeros are ordinary entries, an empty column gives a zero
        column. ``info=True`` returns ``(x, (forward fronts, backward fronts,
        fronts in the plan, column chunks))``."""
        self._h()
        if b.dims.rows != self.n:
            raise MatErr(MatErrKind.IncorrectDimensions)
        if b.dtype != self.dtype:
            raise TypeError(f"NdFactor.solve_sparse: needs Csr<{self.dtype}> (the factor's dtype), got {b.dtype}")
        r = None if rows is None else self._rows_arg("solve_sparse", "rows", rows)
        k = b.dims.cols
        rp, ci, v = b._csr_arrays()
        b_rows = np.repeat(np.arange(self.n, dtype=np.uint64), np.diff(np.asarray(rp).astype(np.int64)))
        cols = np.asarray(ci).astype(np.int64)
        order = np.argsort(cols, kind="stable")  # column-compressed: rows stay ascending within a column
        col_ptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=k))]).astype(np.uint64)
        out, inf = self._solve_sparse(k, col_ptr, np.ascontiguousarray(b_rows[order]),
                                      np.ascontiguousarray(np.asarray(v, dtype=self.dtype)[order]), r)
        nout = self.n if r is None else r.shape[0]
        x = Dense(k, nout, out)
        return (x, inf) if info else x

    def inv_block(self, rows, cols) -> np.ndarray:
        """``A^-1[rows, cols]`` for ANY rows and columns (A's order), an array
        of shape ``len(rows) x len(cols)`` of the factor's dtype: the
        :meth:`solve_sparse` of the unit columns ``e_cols`` at ``rows``, so
        entry ``(i, j)`` has the bits of ``solve``'s row ``rows[i]`` for the
        right-hand side ``e_cols[j]``. Where :meth:`inv_entries` refuses a
        pair off the pattern of ``L + L^T``, this answers. ``rows`` / ``cols``
        as ``solve_sparse``'s ``rows``."""
        self._h()
        r = self._rows_arg("inv_block", "rows", rows)
        c = self._rows_arg("inv_block", "cols", cols)
        k = c.shape[0]
        col_ptr = np.arange(k + 1, dtype=np.uint64)
        out, _ = self._solve_sparse(k, col_ptr, c, np.ones(k, dtype=self.dtype), r)
        return np.stack(out, axis=1) if k else np.zeros((r.shape[0], 0), dtype=self.dtype)

    @property
    def schur_index(self) -> np.ndarray:
        """The Schur set as given to ``cholesky_nd(a, schur=idx)`` (uint64; empty
        for a factor made without one): the order of ``schur``'s rows and
        columns and of ``schur_condense``'s. ``perm`` ends in it, sorted."""
        lib = _lib.load()
        m = ctypes.c_uint64()
        _lib.check(lib.bsm_nd_factor_schur_info(self._h(), ctypes.byref(m), None))
        idx = np.zeros(m.value, dtype=np.uint64)
        _lib.check(lib.bsm_nd_factor_schur_info(self._h(), None, _lib.ptr(idx)))
        return idx

    def _schur_m(self, what: str) -> int:
        m = self.schur_index.shape[0]
        if m == 0:  # the library's own refusal, before the shapes are compared with an empty set's
            raise _lib.BsmError(_lib.BSM_ERR_INVALID, f"nd factor {what}: the factor was made without a Schur set "
                                                      "(cholesky_nd(a, schur=idx))")
        return m

    def _dense_cols(self, what: str, d: Dense, rows: int) -> tuple[int, list]:
        dims = d.get_dims()
        k = dims.cols
        if k and d.dtype != self.dtype:
            raise TypeError(f"NdFactor.{what}: needs Dense<{self.dtype}>, got {d.dtype}")
        if dims.rows != rows:
            raise MatErr(MatErrKind.IncorrectDimensions)
        return k, [np.ascontiguousarray(np.asarray(d.get_col(j))[:rows]) for j in range(k)]

    def schur(self, a: Csr) -> np.ndarray:
        """``S = A_GG - A_GI A_II^-1 A_IG`` on the set ``G`` the factor was made
        with (``bsm_nd_factor_schur``), an ``(m, m)`` array of the factor's
        dtype with rows and columns in ``schur_index``'s order. ``a`` is the
        matrix this is the factor of (its pattern is checked as ``refactor``
        checks it; its values are the caller's responsibility). ``S`` is read
        out of the factorisation: ``a``'s entries inside ``G`` plus the update
        block left under the separator tree's root, one addition per entry in
        a fixed order. ``S == S.T`` exactly and the bits repeat. Raises for a
        factor made without a set, and after ``update`` / ``downdate`` until a
        ``refactor``."""
        _check_factorable(a, "NdFactor.schur")
        h = self._h()
        m = self._schur_m("schur")
        out = np.zeros((m, m), dtype=self.dtype, order="F")
        _raise_for(_lib.require_device().bsm_nd_factor_schur(h, a._device().handle, _lib.ptr(out), max(m, 1)))
        return out

    def schur_condense(self, b: Dense) -> Dense:
        """``g = b_G - A_GI A_II^-1 b_I`` for the columns of ``b`` (``n x k``,
        the factor's dtype): a ``Dense`` ``m x k`` in ``schur_index``'s order
        (``bsm_nd_factor_schur_condense``). With ``S x_G = g`` solved by the
        caller, :meth:`schur_expand` gives ``x``."""
        h = self._h()
        m = self._schur_m("schur_condense")
        k, b_cols = self._dense_cols("schur_condense", b, self.n)
        out = Dense.new_default_with_dims(k, m, dtype=self.dtype)
        _raise_for(_lib.require_device().bsm_nd_factor_schur_condense(h, _lib.ptr_array(b_cols), k,
                                                                      _lib.ptr_array(out.data)))
        return out

    def schur_expand(self, b: Dense, xg) -> Dense:
        """``x`` (``n x k``) from ``b`` and a given ``x_G`` (``xg``: a ``Dense``
        or array ``m x k`` of the factor's dtype, ``schur_index``'s order):
        ``x_I = A_II^-1 (b_I - A_IG x_G)`` (``bsm_nd_factor_schur_expand``).
        Stateless: it repeats ``schur_condense``'s forward pass and keeps
        nothing between the two calls (about one forward pass of a solve).
        With ``xg`` the rows ``schur_index`` of ``solve(b)`` it returns
        ``solve(b)`` bit for bit."""
        h = self._h()
        m = self._schur_m("schur_expand")
        k, b_cols = self._dense_cols("schur_expand", b, self.n)
        if not isinstance(xg, Dense):
            arr = np.asarray(xg)
            arr = arr.reshape(arr.shape[0], -1) if arr.ndim <= 2 else arr
            if arr.ndim != 2:
                raise ValueError(f"NdFactor.schur_expand: xg must be (m,) or (m, k), got {arr.shape}")
            xg = Dense.from_columns([np.ascontiguousarray(arr[:, j]) for j in range(arr.shape[1])]) \
                if arr.shape[1] else Dense(0, arr.shape[0], [])
        kg, g_cols = self._dense_cols("schur_expand", xg, m)
        if kg != k:
            raise MatErr(MatErrKind.IncorrectDimensions)
        out = Dense.new_default_with_dims(k, self.n, dtype=self.dtype)
        _raise_for(_lib.require_device().bsm_nd_factor_schur_expand(h, _lib.ptr_array(b_cols), k,
                                                                    _lib.ptr_array(g_cols), _lib.ptr_array(out.data)))
        return out

    def logdet(self) -> float:
        """``log det A = 2 sum log L_ii`` (``bsm_nd_factor_logdet``), summed in
        f64 in a fixed order: the same bits on every call."""
        h = self._h()
        v = ctypes.c_double()
        _raise_for(_lib.require_device().bsm_nd_factor_logdet(h, ctypes.byref(v)))
        return v.value

    def _selinv(self, want_diag: bool, rows, cols):
        """``bsm_nd_factor_selinv``: (diag or None, vals or None)."""
        h = self._h()
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        c = np.ascontiguousarray(cols, dtype=np.uint64)
        diag = np.zeros(self.n, dtype=self.dtype) if want_diag else None
        nq = r.shape[0]
        vals = np.zeros(nq, dtype=self.dtype)
        if (want_diag and self.n) or nq:
            lib = _lib.require_device()
            _raise_for(lib.bsm_nd_factor_selinv(h, _lib.ptr(diag) if want_diag else None, nq, _lib.ptr(r),
                                                _lib.ptr(c), _lib.ptr(vals)))
        return diag, vals

    def inv_diag(self) -> np.ndarray:
        """``diag(A^-1)`` in A's order (the marginal variances of a Gaussian
        with precision ``A``), ``n`` values of the factor's dtype: the
        selected inverse by the Takahashi recursion over the fronts
        (``bsm_nd_factor_selinv``), a few times the factor's flops instead of
        ``n`` solves. Allocates a second set of fronts for the call. Every
        sum has a fixed order: the same bits on every call."""
        self._h()
        return self._selinv(True, (), ())[0]

    def inv_entries(self, rows, cols) -> np.ndarray:
        """``(A^-1)[rows[e], cols[e]]`` for pairs on the pattern of ``L + L^T``
        (A's order, either triangle: ``(i, j)`` and ``(j, i)`` give the same
        bits). ``rows`` and ``cols`` are 1-D integer array-likes of equal
        length. An index ``>= n`` raises ``MatErr(OutOfBounds)``; a pair
        outside the pattern raises the error for ``BSM_ERR_INVALID`` naming
        how many pairs and the first one."""
        self._h()
        r, c = np.asarray(rows), np.asarray(cols)
        if r.ndim != 1 or c.ndim != 1 or r.shape != c.shape:
            raise ValueError(f"NdFactor.inv_entries: rows and cols must be 1-D of equal length, got "
                             f"{r.shape} and {c.shape}")
        for name, x in (("rows", r), ("cols", c)):
            if x.size and not np.issubdtype(x.dtype, np.integer):
                raise TypeError(f"NdFactor.inv_entries: {name} must be integers, got {x.dtype}")
            if x.size and int(x.min()) < 0:
                raise ValueError(f"NdFactor.inv_entries: {name} has a negative index")
        return self._selinv(False, r, c)[1]

    def inv_on(self, a: Csr) -> Csr:
        """``A^-1`` on ``a``'s own stored pattern: a ``Csr`` with ``a``'s
        ``row_index`` / ``col_index`` and the values ``(A^-1)[i, j]``. Every
        stored entry of the factored matrix lies in the fronts, so this never
        raises for it. Zeros are KEPT: the pattern is ``a``'s, not
        ``Csr::insert``'s zero-dropping rule. ``a`` of another shape raises
        ``MatErr(IncorrectDimensions)``."""
        self._h()
        if a.dims.rows != self.n or a.dims.cols != self.n:
            raise MatErr(MatErrKind.IncorrectDimensions)
        rp, ci, _ = a._csr_arrays()
        rows = np.repeat(np.arange(self.n, dtype=np.uint64), np.diff(rp.astype(np.int64)))
        vals = self._selinv(False, rows, ci)[1]
        return Csr.from_csr_arrays((self.n, self.n), rp, ci, vals, dtype=self.dtype)

    @property
    def perm(self) -> np.ndarray:
        """``perm[new] = old``: ``(P A P^T)[i, j] = A[perm[i], perm[j]]``."""
        p = np.zeros(self.n, dtype=np.int64)
        _raise_for(_lib.require_device().bsm_nd_factor_perm(self._h(), _lib.ptr(p)))
        return p

    def _export(self, want_l: bool) -> Csr:
        lib = _lib.require_device()
        out = ctypes.c_void_p()
        args = (ctypes.byref(out), None) if want_l else (None, ctypes.byref(out))
        _raise_for(lib.bsm_nd_factor_export(self._h(), *args))
        return Csr._from_device(_lib.DeviceCsr(out.value))

    def l(self) -> Csr:
        """``L`` (new order): rows ascending, the diagonal last in each row,
        as ``cholesky_decomp`` returns it and ``forward_substitution`` reads it."""
        return self._export(True)

    def l_star(self) -> Csr:
        """``L^T`` (new order): the diagonal first in each row, as
        ``backward_substitution`` reads it."""
        return self._export(False)

    def _info(self, which: int) -> int:
        v = [ctypes.c_uint64(), ctypes.c_uint64()]
        _lib.check(_lib.load().bsm_nd_factor_info(self._h(), None, None, ctypes.byref(v[0]), ctypes.byref(v[1])))
        return v[which].value

    @property
    def nbytes(self) -> int:
        """Device memory the handle owns (fronts and inverse diagonal tiles)."""
        return self._info(0)

    @property
    def nnz_l(self) -> int:
        """Stored entries of ``L``, or 0 until ``l()`` / ``l_star()`` has counted them."""
        return self._info(1)

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h and _lib._lib is not None:
            _lib._lib.bsm_nd_factor_free(h)
        self.handle = None
        self._vals_key = self._vals_ref = self._grad_weights = None  # the device tensors kept for autograd

    def __enter__(self) -> "NdFactor":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        self.close()


def cholesky_nd(a: Csr, factor_dtype=None, schur=None) -> NdFactor:
    """Analysis (through the plan caches of ``solve(order="nd")``) and numeric
    factorisation of ``P A P^T`` (``bsm_nd_factor_create``), kept as an
    :class:`NdFactor`. The same type and shape checks as :func:`solve`; a
    matrix that is not positive definite is reported here.

    ``factor_dtype`` (``np.float32`` or ``np.float64``; ``None`` = ``a``'s)
    chooses the dtype the factor is computed and stored in
    (``bsm_nd_factor_create_as``): an f32 factor of an f64 matrix has half the
    bytes and the bits of ``cholesky_nd`` on the matrix rounded to f32;
    ``NdFactor.solve_refined`` brings its solves back to f64 accuracy.

    ``schur`` (a 1-D integer array-like of distinct vertices, any order;
    ``None`` = none): the Schur set ``G`` (``bsm_nd_factor_create_schur``). The
    analysis orders these vertices last, as the separator tree's root, over the
    ordinary tree of the others, and the factor then also answers
    ``schur(a)``, ``schur_condense(b)`` and ``schur_expand(b, xg)``. Every
    other method works as on any factor (of ``P A P^T`` with this ``P``), and
    ``refactor`` / ``refactor_partial`` keep the set. Such a plan is the
    factor's alone: the plan caches neither hold it nor hand it out. An index
    ``>= n`` or a repeated one raises the error for ``BSM_ERR_INVALID``, more
    than 16384 vertices the one for ``BSM_ERR_UNSUPPORTED`` (the root front is
    dense, ``(64 ceil(m / 64))^2`` values)."""
    _check_factorable(a, "cholesky_nd")
    if factor_dtype is not None and np.dtype(factor_dtype) not in _FLOATS:
        raise TypeError(f"cholesky_nd: factor_dtype must be float32 or float64, got {np.dtype(factor_dtype)}")
    idx = None if schur is None else NdFactor._rows_arg("cholesky_nd", "schur", schur)
    dev = a._device()
    lib = _lib.require_device()
    out = ctypes.c_void_p()
    if idx is not None:
        code = _lib.DTYPE_CODES[a.dtype if factor_dtype is None else np.dtype(factor_dtype)]
        _raise_for(lib.bsm_nd_factor_create_schur(dev.handle, code, _lib.ptr(idx), idx.shape[0], ctypes.byref(out)))
    elif factor_dtype is None:
        _raise_for(lib.bsm_nd_factor_create(dev.handle, ctypes.byref(out)))
    else:
        _raise_for(lib.bsm_nd_factor_create_as(dev.handle, _lib.DTYPE_CODES[np.dtype(factor_dtype)],
                                               ctypes.byref(out)))
    return NdFactor(out.value, a.dtype)


def nd_analyse(n: int, row_ptr, col_idx, leaf: int = 256, last=None) -> dict:
    """The host analysis of ``solve(order="nd")`` on a CSR pattern
    (``bsm_nd_analyse``; no device): ``perm`` (perm[new] = old) and the
    separator tree in post-order (``start``, ``end``, ``parent``, ``level``,
    ``slot``, front rows ``st``). ``last`` (distinct vertices, any order;
    ``bsm_nd_analyse_last``): the root node owns exactly these, over the tree
    of the others, as ``cholesky_nd(a, schur=last)`` orders them."""
    lib = _lib.load()
    rp = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    ci = np.ascontiguousarray(col_idx, dtype=np.uint64)
    perm = np.zeros(n, dtype=np.int64)
    nn = ctypes.c_uint64(0)
    sl = ctypes.c_uint64(0)
    if last is None:
        def run(*out):
            return lib.bsm_nd_analyse(n, _lib.ptr(rp), _lib.ptr(ci), leaf, *out)
    else:
        lv = np.ascontiguousarray(last, dtype=np.uint64)

        def run(*out):
            return lib.bsm_nd_analyse_last(n, _lib.ptr(rp), _lib.ptr(ci), leaf, _lib.ptr(lv), lv.shape[0], *out)
    _lib.check(run(_lib.ptr(perm), None, 0, ctypes.byref(nn), None, 0, ctypes.byref(sl)))
    nodes = np.zeros((max(nn.value, 1), 8), dtype=np.int64)
    st = np.zeros(max(sl.value, 1), dtype=np.int64)
    _lib.check(run(_lib.ptr(perm), _lib.ptr(nodes), nn.value, ctypes.byref(nn), _lib.ptr(st), sl.value,
                   ctypes.byref(sl)))
    nodes = nodes[: nn.value]
    return {"perm": perm, "start": nodes[:, 0], "end": nodes[:, 1], "parent": nodes[:, 2], "level": nodes[:, 3],
            "slot": nodes[:, 4],
            "st": [st[o: o + m] for m, o in zip(nodes[:, 5], nodes[:, 6])]}
