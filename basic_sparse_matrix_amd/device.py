"""Device-level (HBM-resident) entry points for benchmarks and multi-GPU runs.

Thin wrappers over the ``bsm_dev_*`` functions of include/bsm.h. PyTorch is
used only as plumbing: it allocates HBM buffers (``torch.empty(...,
device="cuda")``), supplies the HIP stream (``torch.cuda.current_stream()``)
and, in bench.py, ``torch.distributed`` (RCCL). All compute is the HIP
kernels of libbsm_hip.so.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

TORCH_DT = {
    np.dtype(np.float64): torch.float64,
    np.dtype(np.float32): torch.float32,
    np.dtype(np.int32): torch.int32,
    np.dtype(np.uint32): torch.uint32,
    np.dtype(np.int64): torch.int64,
    np.dtype(np.uint64): torch.uint64,
}


def _stream(stream=None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def _p(t: torch.Tensor) -> int:
    return t.data_ptr() if t.numel() else 0


@dataclass
class DeviceCsrBlock:
    """A CSR row block resident in HBM: rows [row0, row0+rows) of a matrix
    with n_cols columns. row_ptr is local (starts at 0)."""

    row0: int
    rows: int
    n_cols: int
    row_ptr: torch.Tensor  # int64 [rows+1]
    col: torch.Tensor  # int32 [nnz]
    vals: torch.Tensor  # T [nnz]
    dtype: np.dtype
    panel_cols: int = 0  # column-panel plan (bsm_dev_spmm_plan), 0 = none
    seg: torch.Tensor | None = None
    tiled: "TiledPlan | None" = None  # row-block x column-panel copy (bsm_dev_tiled_create)

    @property
    def nnz(self) -> int:
        return int(self.col.numel())

    @classmethod
    def generate(cls, seed, row0, rows, n_cols, rowlen_kind=_lib.ROWLEN_CONST, a=10, b=10,
                 value_kind=_lib.VAL_UNIFORM, dtype=np.float64, device="cuda") -> "DeviceCsrBlock":
        """Synthetic CSR rows (bsm_synth.h recipe) generated on the device."""
        lib = _lib.require_device()
        dt = np.dtype(dtype)
        rp = torch.empty(rows + 1, dtype=torch.int64, device=device)
        wsb = lib.bsm_dev_scan_workspace_bytes(rows)
        ws = torch.empty(max(16, wsb), dtype=torch.uint8, device=device)
        s = _stream()
        _lib.check(lib.bsm_dev_gen_row_ptr(seed, row0, rows, n_cols, rowlen_kind, a, b, _p(rp), _p(ws), wsb, s))
        nnz = int(rp[rows].item()) if rows else 0
        col = torch.empty(nnz, dtype=torch.int32, device=device)
        vals = torch.empty(nnz, dtype=TORCH_DT[dt], device=device)
        _lib.check(lib.bsm_dev_gen_entries(_lib.DTYPE_CODES[dt], seed, row0, rows, n_cols, value_kind, _p(rp),
                                           _p(col), _p(vals), s))
        return cls(row0, rows, n_cols, rp, col, vals, dt)

    def plan(self, k: int, panel_cols: int | None = None) -> int:
        """Build the column-panel plan for k right-hand columns (synchronous,
        once per matrix). Returns the panel width in use (0 = single pass)."""
        lib = _lib.require_device()
        w = lib.bsm_dev_spmm_panel_cols(_lib.DTYPE_CODES[self.dtype], self.n_cols, k) if panel_cols is None \
            else panel_cols
        self.panel_cols, self.seg = 0, None
        nbytes = lib.bsm_dev_spmm_plan_bytes(self.rows, self.n_cols, w)
        if w == 0 or nbytes == 0:
            return 0
        seg = torch.empty(nbytes // 4, dtype=torch.int32, device=self.col.device)
        usable = ctypes.c_int(0)
        _lib.check(lib.bsm_dev_spmm_plan(self.rows, self.n_cols, _p(self.row_ptr), _p(self.col), w, _p(seg),
                                         ctypes.byref(usable), _stream()))
        if usable.value:
            self.panel_cols, self.seg = w, seg
        return self.panel_cols

    def plan_tiled(self, k: int, force: bool = False) -> "TiledPlan | None":
        """Build the row-block x column-panel copy for k right-hand columns
        when the library wants it for this shape (f64; k = 32 and X > 1 GiB, or
        k = 1 and X > 4 MiB), or
        whenever possible with force (any chunk padding accepted). Synchronous, once per matrix. Returns
        the plan, or None (shape not served, or no memory for the copy)."""
        lib = _lib.require_device()
        self.tiled = None
        if self.dtype != np.float64 or k not in (1, 32) or self.nnz == 0:
            return None
        if not force:
            max_len = int((self.row_ptr[1:] - self.row_ptr[:-1]).max().item()) if self.rows else 0
            if not lib.bsm_dev_tiled_wanted(_lib.DTYPE_CODES[self.dtype], self.rows, self.n_cols, self.nnz, k,
                                            max_len):
                return None
        h = ctypes.c_void_p()
        rc = lib.bsm_dev_tiled_create(self.rows, self.n_cols, self.nnz, _p(self.row_ptr), _p(self.col),
                                      _p(self.vals), k, _lib.BSM_TILED_ANY_PADDING if force else 0,
                                      ctypes.byref(h), _stream())
        if rc in (_lib.BSM_ERR_UNSUPPORTED, _lib.BSM_ERR_OOM):
            return None
        _lib.check(rc)
        self.tiled = TiledPlan(h.value, k)
        return self.tiled

    def spmm(self, x: torch.Tensor, y: torch.Tensor, row_nnz: torch.Tensor | None = None, stream=None) -> None:
        """Y = A X (x: n_cols x k row-major, y: rows x k row-major), async.
        Uses the tiled copy or the column-panel plan when one was built (same
        bits)."""
        lib = _lib.load()
        k = x.shape[1] if x.dim() == 2 else 1
        if self.tiled is not None and k == self.tiled.k:
            _lib.check(lib.bsm_dev_spmm_tiled(self.tiled.handle, _p(x), _p(y),
                                              _p(row_nnz) if row_nnz is not None else 0, _stream(stream)))
            return
        if self.seg is not None:
            _lib.check(lib.bsm_dev_spmm_panelled(_lib.DTYPE_CODES[self.dtype], self.rows, self.n_cols, self.nnz,
                                                 _p(self.row_ptr), _p(self.col), _p(self.vals), k, _p(x), _p(y),
                                                 _p(row_nnz) if row_nnz is not None else 0, self.panel_cols,
                                                 _p(self.seg), _stream(stream)))
            return
        _lib.check(lib.bsm_dev_spmm(_lib.DTYPE_CODES[self.dtype], self.rows, self.n_cols, self.nnz, _p(self.row_ptr),
                                    _p(self.col), _p(self.vals), k, _p(x), _p(y),
                                    _p(row_nnz) if row_nnz is not None else 0, _stream(stream)))


class TiledPlan:
    """Owner of a bsm_tiled handle (the row-block x column-panel copy)."""

    def __init__(self, handle: int, k: int = 32):
        self.handle = handle
        self.k = k

    def info(self) -> dict:
        lib = _lib.load()
        b, sl, pc = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        ps, br = ctypes.c_uint32(), ctypes.c_uint32()
        _lib.check(lib.bsm_tiled_info(self.handle, ctypes.byref(b), ctypes.byref(sl), ctypes.byref(pc),
                                      ctypes.byref(ps), ctypes.byref(br)))
        return {"bytes": b.value, "slots": sl.value, "panel_cols": pc.value, "passes": ps.value,
                "batch_rows": br.value}

    def __del__(self):
        if getattr(self, "handle", None) and _lib._lib is not None:
            _lib._lib.bsm_tiled_destroy(self.handle)
            self.handle = None


def gen_dense(seed, row0, n, k, value_kind=_lib.VAL_UNIFORM, dtype=np.float64, device="cuda") -> torch.Tensor:
    """Row-major n x k dense operand X[r][j] = bsm_x_value(seed, row0+r, j)."""
    lib = _lib.require_device()
    dt = np.dtype(dtype)
    x = torch.empty((n, k), dtype=TORCH_DT[dt], device=device)
    _lib.check(lib.bsm_dev_gen_dense(_lib.DTYPE_CODES[dt], seed, row0, n, k, value_kind, _p(x), _stream()))
    return x


def nd_factor_solve(factor, b: torch.Tensor, out: torch.Tensor | None = None, *, system: str = "A",
                    stream=None) -> torch.Tensor:
    """A solve on a kept factor (``solver.NdFactor``) with ``b`` and ``x``
    resident in HBM (``bsm_dev_nd_factor_solve``): no host copy of either.
    ``b`` is ``(n,)`` or row-major ``(n, k)``, contiguous, of the factor's
    dtype, on its device; ``out`` defaults to a new tensor and may be ``b``
    (in place). ``system`` as ``NdFactor.solve``. Runs on ``stream`` and
    returns after the solve's status word is read back; the same kernels and
    bits as the host-buffer solve."""
    from .solver import nd_system_code
    from .sparse import _raise_for

    code = nd_system_code(system)
    want = TORCH_DT[np.dtype(factor.dtype)]
    out = torch.empty_like(b) if out is None else out
    for name, t in (("b", b), ("out", out)):
        if t.dtype != want:
            raise TypeError(f"nd_factor_solve: {name} is {t.dtype}, the factor is {factor.dtype}")
        if not t.is_cuda:
            raise ValueError(f"nd_factor_solve: {name} is not on the device")
        if t.dim() not in (1, 2) or t.shape[0] != factor.n or not t.is_contiguous():
            raise ValueError(f"nd_factor_solve: {name} must be contiguous, ({factor.n},) or ({factor.n}, k), "
                             f"got {tuple(t.shape)}")
    if out.shape != b.shape or out.device != b.device:
        raise ValueError(f"nd_factor_solve: out is {tuple(out.shape)} on {out.device}, b {tuple(b.shape)} on {b.device}")
    k = b.shape[1] if b.dim() == 2 else 1
    _raise_for(_lib.require_device().bsm_dev_nd_factor_solve(factor._h(), code, k, _p(b), _p(out), _stream(stream)))
    return out


def nd_factor_solve_sparse(factor, b, rows=None, out: torch.Tensor | None = None, *, stream=None) -> torch.Tensor:
    """``NdFactor.solve_sparse`` with ``x`` resident in HBM
    (``bsm_dev_nd_factor_solve_sparse``): ``b`` is a host ``Csr`` of shape
    ``n x k`` of the factor's dtype, ``rows`` a 1-D integer array-like or
    ``None`` (every row), both as ``NdFactor.solve_sparse`` takes them; ``out``
    is row-major ``(len(rows), k)`` (``(n, k)``), contiguous, of the factor's
    dtype, on its device, and defaults to a new tensor. Runs on ``stream`` and
    returns after it has drained; the same kernels and bits as the host call."""
    from .solver import MatErr, MatErrKind, NdFactor
    from .sparse import _raise_for

    h = factor._h()
    if b.dims.rows != factor.n:
        raise MatErr(MatErrKind.IncorrectDimensions)
    if b.dtype != factor.dtype:
        raise TypeError(f"nd_factor_solve_sparse: needs Csr<{factor.dtype}> (the factor's dtype), got {b.dtype}")
    r = None if rows is None else NdFactor._rows_arg("solve_sparse", "rows", rows)
    k = b.dims.cols
    nout = factor.n if r is None else r.shape[0]
    want = TORCH_DT[np.dtype(factor.dtype)]
    out = torch.empty((nout, k), dtype=want, device="cuda") if out is None else out
    if out.dtype != want:
        raise TypeError(f"nd_factor_solve_sparse: out is {out.dtype}, the factor is {factor.dtype}")
    if not out.is_cuda:
        raise ValueError("nd_factor_solve_sparse: out is not on the device")
    if tuple(out.shape) != (nout, k) or not out.is_contiguous():
        raise ValueError(f"nd_factor_solve_sparse: out must be contiguous, ({nout}, {k}), got {tuple(out.shape)}")
    rp, ci, v = b._csr_arrays()
    b_rows = np.repeat(np.arange(factor.n, dtype=np.uint64), np.diff(np.asarray(rp).astype(np.int64)))
    cols = np.asarray(ci).astype(np.int64)
    order = np.argsort(cols, kind="stable")  # column-compressed: rows stay ascending within a column
    col_ptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=k))]).astype(np.uint64)
    br = np.ascontiguousarray(b_rows[order])
    vals = np.ascontiguousarray(np.asarray(v, dtype=factor.dtype)[order])
    if k and nout:  # an empty ``rows`` would read as NULL ("every row") on the other side
        _raise_for(_lib.require_device().bsm_dev_nd_factor_solve_sparse(
            h, k, _lib.ptr(col_ptr), _lib.ptr(br), _lib.ptr(vals), 0 if r is None else nout,
            None if r is None else _lib.ptr(r), _p(out), None, _stream(stream)))
    return out


def _schur_operand(what: str, name: str, t: torch.Tensor, factor, rows: int) -> int:
    """The checks of a (rows,) or row-major (rows, k) device operand; returns k."""
    want = TORCH_DT[np.dtype(factor.dtype)]
    if t.dtype != want:
        raise TypeError(f"{what}: {name} is {t.dtype}, the factor is {factor.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} is not on the device")
    if t.dim() not in (1, 2) or t.shape[0] != rows or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous, ({rows},) or ({rows}, k), got {tuple(t.shape)}")
    return t.shape[1] if t.dim() == 2 else 1


def nd_factor_schur(factor, a, out: torch.Tensor | None = None, *, stream=None) -> torch.Tensor:
    """``NdFactor.schur`` with ``S`` resident in HBM (``bsm_dev_nd_factor_schur``):
    ``a`` is the host ``Csr`` the factor was made of, ``out`` an ``(m, m)``
    contiguous tensor of the factor's dtype on its device (``S`` is exactly
    symmetric, so row- and column-major agree) and defaults to a new one. Runs
    on ``stream`` and returns after it has drained; the same kernel and bits
    as the host call."""
    from .sparse import _raise_for

    h = factor._h()
    m = factor._schur_m("schur")
    want = TORCH_DT[np.dtype(factor.dtype)]
    out = torch.empty((m, m), dtype=want, device="cuda") if out is None else out
    if out.dtype != want:
        raise TypeError(f"nd_factor_schur: out is {out.dtype}, the factor is {factor.dtype}")
    if not out.is_cuda:
        raise ValueError("nd_factor_schur: out is not on the device")
    if tuple(out.shape) != (m, m) or not out.is_contiguous():
        raise ValueError(f"nd_factor_schur: out must be contiguous, ({m}, {m}), got {tuple(out.shape)}")
    _raise_for(_lib.require_device().bsm_dev_nd_factor_schur(h, a._device().handle, out.data_ptr(), max(m, 1),
                                                             _stream(stream)))
    return out


def nd_factor_schur_condense(factor, b: torch.Tensor, out: torch.Tensor | None = None, *, stream=None) -> torch.Tensor:
    """``NdFactor.schur_condense`` on device tensors
    (``bsm_dev_nd_factor_schur_condense``): ``b`` is ``(n,)`` or row-major
    ``(n, k)``, ``out`` ``(m,)`` / ``(m, k)`` in ``schur_index``'s order, both
    contiguous, of the factor's dtype, on its device."""
    from .sparse import _raise_for

    h = factor._h()
    m = factor._schur_m("schur_condense")
    k = _schur_operand("nd_factor_schur_condense", "b", b, factor, factor.n)
    out = torch.empty((m,) + tuple(b.shape[1:]), dtype=b.dtype, device=b.device) if out is None else out
    if _schur_operand("nd_factor_schur_condense", "out", out, factor, m) != k or out.dim() != b.dim():
        raise ValueError(f"nd_factor_schur_condense: out is {tuple(out.shape)}, b {tuple(b.shape)}")
    _raise_for(_lib.require_device().bsm_dev_nd_factor_schur_condense(h, _p(b), k, _p(out), _stream(stream)))
    return out


def nd_factor_schur_expand(factor, b: torch.Tensor, xg: torch.Tensor, out: torch.Tensor | None = None, *,
                           stream=None) -> torch.Tensor:
    """``NdFactor.schur_expand`` on device tensors
    (``bsm_dev_nd_factor_schur_expand``): ``b`` and ``out`` ``(n,)`` or
    row-major ``(n, k)``, ``xg`` ``(m,)`` / ``(m, k)`` in ``schur_index``'s
    order; ``out`` defaults to a new tensor and may be ``b``."""
    from .sparse import _raise_for

    h = factor._h()
    m = factor._schur_m("schur_expand")
    what = "nd_factor_schur_expand"
    k = _schur_operand(what, "b", b, factor, factor.n)
    out = torch.empty_like(b) if out is None else out
    if _schur_operand(what, "xg", xg, factor, m) != k or xg.dim() != b.dim():
        raise ValueError(f"{what}: xg is {tuple(xg.shape)}, b {tuple(b.shape)}")
    if _schur_operand(what, "out", out, factor, factor.n) != k or out.shape != b.shape:
        raise ValueError(f"{what}: out is {tuple(out.shape)}, b {tuple(b.shape)}")
    _raise_for(_lib.require_device().bsm_dev_nd_factor_schur_expand(h, _p(b), k, _p(xg), _p(out), _stream(stream)))
    return out


def nd_factor_solve_refined(factor, a, b: torch.Tensor, out: torch.Tensor | None = None, *, max_iter: int = 5,
                            tol: float | None = None, stream=None):
    """``NdFactor.solve_refined`` with ``b`` and ``x`` resident in HBM
    (``bsm_dev_nd_factor_solve_refined``). ``a`` is the system's ``Csr``;
    ``b`` is ``(n,)`` or row-major ``(n, k)``, contiguous, of ``a``'s dtype,
    on the factor's device; ``out`` defaults to a new tensor and may be ``b``.
    Returns ``(out, RefineInfo)``. Runs on ``stream`` and is synchronous for
    it; the same kernels and bits as the host-buffer call."""
    from .solver import RefineInfo, check_refine_args, refine_tol_in_use
    from .sparse import _raise_for
    from .util import MatErr, MatErrKind

    h = factor._h()
    if b.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"nd_factor_solve_refined: b is {b.dtype}, needs float32 or float64")
    b_np = np.dtype(np.float64) if b.dtype == torch.float64 else np.dtype(np.float32)
    check_refine_args(a, b_np, max_iter, tol, "nd_factor_solve_refined")
    out = torch.empty_like(b) if out is None else out
    for name, t in (("b", b), ("out", out)):
        if t.dtype != b.dtype:
            raise TypeError(f"nd_factor_solve_refined: {name} is {t.dtype}, a is {a.dtype}")
        if not t.is_cuda:
            raise ValueError(f"nd_factor_solve_refined: {name} is not on the device")
        if t.dim() not in (1, 2) or not t.is_contiguous():
            raise ValueError(f"nd_factor_solve_refined: {name} must be contiguous, (n,) or (n, k), "
                             f"got {tuple(t.shape)}")
    if out.shape != b.shape or out.device != b.device:
        raise ValueError(f"nd_factor_solve_refined: out is {tuple(out.shape)} on {out.device}, b {tuple(b.shape)} "
                         f"on {b.device}")
    if a.dims.rows != factor.n or a.dims.cols != factor.n or b.shape[0] != factor.n:
        raise MatErr(MatErrKind.IncorrectDimensions)
    k = b.shape[1] if b.dim() == 2 else 1
    iters = np.zeros(k, dtype=np.uint32)
    berr = np.zeros(k, dtype=np.float64)
    dev = a._device()
    tol_used = refine_tol_in_use(a, dev, tol)
    _raise_for(_lib.require_device().bsm_dev_nd_factor_solve_refined(
        h, dev.handle, k, _p(b), _p(out), max_iter, tol_used, _lib.ptr(iters), _lib.ptr(berr),
        _stream(stream)))
    return out, RefineInfo(iters, berr, berr <= tol_used, tol_used)


def nd_factor_solve_pcg(factor, a, b: torch.Tensor, out: torch.Tensor | None = None, *, max_iter: int = 50,
                        tol: float | None = None, stream=None):
    """``NdFactor.solve_pcg`` with ``b`` and ``x`` resident in HBM
    (``bsm_dev_nd_factor_solve_pcg``). The arguments are
    ``nd_factor_solve_refined``'s. Returns ``(out, PcgInfo)``. Runs on
    ``stream`` and is synchronous for it; the same kernels and bits as the
    host-buffer call."""
    from .solver import PcgInfo, check_refine_args, refine_tol_in_use
    from .sparse import _raise_for
    from .util import MatErr, MatErrKind

    h = factor._h()
    if b.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"nd_factor_solve_pcg: b is {b.dtype}, needs float32 or float64")
    b_np = np.dtype(np.float64) if b.dtype == torch.float64 else np.dtype(np.float32)
    check_refine_args(a, b_np, max_iter, tol, "nd_factor_solve_pcg")
    out = torch.empty_like(b) if out is None else out
    for name, t in (("b", b), ("out", out)):
        if t.dtype != b.dtype:
            raise TypeError(f"nd_factor_solve_pcg: {name} is {t.dtype}, a is {a.dtype}")
        if not t.is_cuda:
            raise ValueError(f"nd_factor_solve_pcg: {name} is not on the device")
        if t.dim() not in (1, 2) or not t.is_contiguous():
            raise ValueError(f"nd_factor_solve_pcg: {name} must be contiguous, (n,) or (n, k), got {tuple(t.shape)}")
    if out.shape != b.shape or out.device != b.device:
        raise ValueError(f"nd_factor_solve_pcg: out is {tuple(out.shape)} on {out.device}, b {tuple(b.shape)} "
                         f"on {b.device}")
    if a.dims.rows != factor.n or a.dims.cols != factor.n or b.shape[0] != factor.n:
        raise MatErr(MatErrKind.IncorrectDimensions)
    k = b.shape[1] if b.dim() == 2 else 1
    iters = np.zeros(k, dtype=np.uint32)
    berr = np.zeros(k, dtype=np.float64)
    flags = np.zeros(k, dtype=np.uint32)
    dev = a._device()
    tol_used = refine_tol_in_use(a, dev, tol)
    _raise_for(_lib.require_device().bsm_dev_nd_factor_solve_pcg(
        h, dev.handle, k, _p(b), _p(out), max_iter, tol_used, _lib.ptr(iters), _lib.ptr(berr), _lib.ptr(flags),
        _stream(stream)))
    return out, PcgInfo(iters, berr, berr <= tol_used, (flags & 1) != 0, tol_used)


def nd_factor_eigsh(factor, a, nev: int, block: int = 4, ncv: int | None = None, tol: float | None = None,
                    v0: torch.Tensor | None = None, seed: int = 0, out: torch.Tensor | None = None, *,
                    vectors: bool = True, stream=None, m=None):
    """``NdFactor.eigsh`` with the start block and the vectors resident in
    HBM (``bsm_dev_nd_factor_eigsh``). ``v0`` is row-major ``(n, block)`` and
    ``out`` row-major ``(n, nev)``, contiguous, of ``a``'s dtype, on the
    factor's device; ``out`` defaults to a new tensor (``None`` is returned
    with ``vectors=False``). Returns ``(lam, out, EigInfo)`` with ``lam`` a
    host array. Runs on ``stream`` and is synchronous for it; the same
    kernels and bits as the host-buffer call. ``m`` (keyword only) is the
    mass matrix of the generalised problem, as ``NdFactor.eigsh``'s
    (``bsm_dev_nd_factor_eigsh_gen``)."""
    from .solver import check_eig_args, check_eig_mass, eig_info
    from .sparse import _raise_for

    h = factor._h()
    n = factor.n
    ncv_use, tol_used = check_eig_args(a, n, nev, block, ncv, tol, seed, "nd_factor_eigsh")
    if m is not None:
        check_eig_mass(a, m, n, "nd_factor_eigsh")
    want = TORCH_DT[np.dtype(a.dtype)]
    if n == 0:
        nev = 0
    if vectors and out is None:
        out = torch.empty((n, nev), dtype=want, device="cuda")
    if not vectors:
        out = None
    for name, t, shape in (("v0", v0, (n, block)), ("out", out, (n, nev))):
        if t is None:
            continue
        if t.dtype != want:
            raise TypeError(f"nd_factor_eigsh: {name} is {t.dtype}, a is {a.dtype}")
        if not t.is_cuda:
            raise ValueError(f"nd_factor_eigsh: {name} is not on the device")
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"nd_factor_eigsh: {name} must be contiguous, {shape}, got {tuple(t.shape)}")
    lam = np.zeros(nev, dtype=np.float64)
    resid = np.zeros(nev, dtype=np.float64)
    info = np.zeros(4, dtype=np.uint32)
    dev = a._device()
    mdev = m._device() if m is not None else None
    if n:
        lib = _lib.require_device()
        v0_p = _p(v0) if v0 is not None else None
        out_p = _p(out) if out is not None else None
        if m is None:
            _raise_for(lib.bsm_dev_nd_factor_eigsh(h, dev.handle, nev, block, ncv_use, tol_used, seed, v0_p,
                                                   _lib.ptr(lam), out_p, _lib.ptr(resid), _lib.ptr(info),
                                                   _stream(stream)))
        else:
            _raise_for(lib.bsm_dev_nd_factor_eigsh_gen(h, dev.handle, mdev.handle, nev, block, ncv_use, tol_used,
                                                       seed, v0_p, _lib.ptr(lam), out_p, _lib.ptr(resid),
                                                       _lib.ptr(info), _stream(stream)))
    return lam, out, eig_info(a, dev, lam, resid, info, tol_used, m, mdev)


def nd_factor_inv_diag(factor, out: torch.Tensor | None = None, *, stream=None) -> torch.Tensor:
    """``diag(A^-1)`` of a kept factor (``solver.NdFactor.inv_diag``) into a
    device tensor (``bsm_dev_nd_factor_inv_diag``): ``(n,)``, contiguous, of
    the factor's dtype, on its device; ``out`` defaults to a new tensor. Runs
    on ``stream`` and returns after it has drained; the same kernels and bits
    as ``NdFactor.inv_diag()``."""
    from .sparse import _raise_for

    h = factor._h()
    want = TORCH_DT[np.dtype(factor.dtype)]
    out = torch.empty((factor.n,), dtype=want, device="cuda") if out is None else out
    if out.dtype != want:
        raise TypeError(f"nd_factor_inv_diag: out is {out.dtype}, the factor is {factor.dtype}")
    if not out.is_cuda:
        raise ValueError("nd_factor_inv_diag: out is not on the device")
    if out.dim() != 1 or out.shape[0] != factor.n or not out.is_contiguous():
        raise ValueError(f"nd_factor_inv_diag: out must be contiguous, ({factor.n},), got {tuple(out.shape)}")
    _raise_for(_lib.require_device().bsm_dev_nd_factor_inv_diag(h, _p(out), _stream(stream)))
    return out


SDDMM_MODES = {"all": _lib.BSM_SDDMM_ALL, "sym_lower": _lib.BSM_SDDMM_SYM_LOWER}
_NP_OF_TORCH = {torch.float64: np.dtype(np.float64), torch.float32: np.dtype(np.float32)}


def _sddmm_operands(what: str, u: torch.Tensor, v: torch.Tensor, out, nnz: int, rows: int, cols: int, want=None):
    """The SDDMM's host-side checks of U, V and out (dtype, shape, contiguity,
    device, in that order); ``(n,)`` counts as k = 1. Returns ``(k, out)``."""
    want = u.dtype if want is None else want
    if want not in _NP_OF_TORCH:
        raise TypeError(f"{what}: u is {u.dtype}, needs float32 or float64")
    out = torch.empty((nnz,), dtype=want, device=u.device) if out is None else out
    for name, t in (("u", u), ("v", v), ("out", out)):
        if t.dtype != want:
            raise TypeError(f"{what}: {name} is {t.dtype}, needs {want}")
    for name, t, n in (("u", u, rows), ("v", v, cols)):
        if t.dim() not in (1, 2) or t.shape[0] != n:
            raise ValueError(f"{what}: {name} must be ({n},) or ({n}, k), got {tuple(t.shape)}")
    ku, kv = (t.shape[1] if t.dim() == 2 else 1 for t in (u, v))
    if ku != kv:
        raise ValueError(f"{what}: u has {ku} columns, v {kv}")
    if ku == 0:
        raise ValueError(f"{what}: k == 0 (a dot product of no terms)")
    if out.dim() != 1 or out.shape[0] != nnz:
        raise ValueError(f"{what}: out must be ({nnz},), got {tuple(out.shape)}")
    for name, t in (("u", u), ("v", v), ("out", out)):
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
        if not t.is_cuda:
            raise ValueError(f"{what}: {name} is not on the device")
    if v.device != u.device or out.device != u.device:
        raise ValueError(f"{what}: u is on {u.device}, v on {v.device}, out on {out.device}")
    return ku, out


def sddmm(row_ptr: torch.Tensor, col: torch.Tensor, u: torch.Tensor, v: torch.Tensor, mode: str = "all",
          out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """The sampled dense-dense product on a CSR pattern (``bsm_dev_sddmm``):
    ``out[p] = dot(u[i, :], v[j, :])`` for every stored entry ``p = (i, j)``.
    ``row_ptr`` is int64 ``(rows + 1,)`` and ``col`` int32 ``(nnz,)`` as
    ``DeviceCsrBlock`` holds them; ``u`` is row-major ``(rows, k)``, ``v``
    ``(cols, k)`` (``(n,)`` counts as k = 1), float32 or float64, contiguous,
    on one device; ``out`` is ``(nnz,)`` of that dtype and defaults to a new
    tensor. ``mode="sym_lower"`` (square patterns) gives ``dot(u_i, v_j) +
    dot(u_j, v_i)`` below the diagonal, ``dot(u_i, v_i)`` on it and ``+0.0``
    above. The dot's order depends on k alone: the same bits on every launch.
    Asynchronous on ``stream``."""
    if mode not in SDDMM_MODES:
        raise ValueError(f"sddmm: mode must be one of {sorted(SDDMM_MODES)}, got {mode!r}")
    for name, t, dt in (("row_ptr", row_ptr, torch.int64), ("col", col, torch.int32)):
        if t.dtype != dt:
            raise TypeError(f"sddmm: {name} is {t.dtype}, needs {dt}")
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"sddmm: {name} must be contiguous and 1-D, got {tuple(t.shape)}")
    if row_ptr.shape[0] < 1:
        raise ValueError("sddmm: row_ptr needs rows + 1 entries")
    rows, nnz, cols = row_ptr.shape[0] - 1, col.shape[0], v.shape[0] if v.dim() else 0
    if mode == "sym_lower" and rows != cols:
        raise ValueError(f"sddmm: mode='sym_lower' needs a square pattern, got {rows} x {cols}")
    k, out = _sddmm_operands("sddmm", u, v, out, nnz, rows, cols)
    if row_ptr.device != u.device or col.device != u.device:
        raise ValueError(f"sddmm: the pattern is on {row_ptr.device} / {col.device}, u on {u.device}")
    _lib.check(_lib.require_device().bsm_dev_sddmm(_lib.DTYPE_CODES[_NP_OF_TORCH[u.dtype]], SDDMM_MODES[mode], rows,
                                                   cols, nnz, _p(row_ptr), _p(col), k, _p(u), _p(v), _p(out),
                                                   _stream(stream)))
    return out


def nd_factor_sddmm(factor, u: torch.Tensor, v: torch.Tensor, out: torch.Tensor | None = None, *,
                    stream=None) -> torch.Tensor:
    """:func:`sddmm` with ``mode="sym_lower"`` on the pattern a kept factor
    (``solver.NdFactor``) was made from (``bsm_dev_nd_factor_sddmm``): ``u``
    and ``v`` are ``(n,)`` or row-major ``(n, k)`` of one float dtype, ``out``
    is ``(pattern_nnz,)`` in the pattern's storage order. With ``u = Λ`` and
    ``v = x`` its negative is the gradient of a solve with respect to the
    matrix's stored values. Asynchronous on ``stream``."""
    from .sparse import _raise_for

    nnz = factor.pattern_nnz
    k, out = _sddmm_operands("nd_factor_sddmm", u, v, out, nnz, factor.n, factor.n)
    h = factor._h()
    _raise_for(_lib.require_device().bsm_dev_nd_factor_sddmm(h, _lib.DTYPE_CODES[_NP_OF_TORCH[u.dtype]], nnz, k,
                                                             _p(u), _p(v), _p(out), _stream(stream)))
    return out


def nd_factor_refactor_values(factor, vals: torch.Tensor, *, stream=None) -> None:
    """``NdFactor.refactor`` from values that are already in HBM
    (``bsm_dev_nd_factor_refactor_values``): ``vals`` is 1-D, contiguous, on
    the factor's device, of the FACTORED MATRIX's dtype (``src_dtype``), with
    ``pattern_nnz`` entries in the factored pattern's storage order. No
    upload, no pattern comparison; the factor has the bits ``refactor`` gives
    on a ``Csr`` with these values, and its errors. Runs on ``stream`` and
    returns after the factorisation's status word is read back. The factor
    records ``(vals.data_ptr(), vals._version, its rewrite count)`` for
    ``autograd``'s ``refactor=False`` and keeps a reference to ``vals`` until
    its next rewrite, so that the address cannot pass to another tensor."""
    from .sparse import _raise_for

    want = TORCH_DT[np.dtype(factor.src_dtype)]
    if vals.dtype != want:
        raise TypeError(f"nd_factor_refactor_values: vals is {vals.dtype}, the factored matrix is {factor.src_dtype}")
    nnz = factor.pattern_nnz
    if vals.dim() != 1 or vals.shape[0] != nnz or not vals.is_contiguous():
        raise ValueError(f"nd_factor_refactor_values: vals must be contiguous, ({nnz},), got {tuple(vals.shape)}")
    if not vals.is_cuda:
        raise ValueError("nd_factor_refactor_values: vals is not on the device")
    h = factor._h()
    factor._bump_epoch()  # the factor is rewritten, also when the call fails
    _raise_for(_lib.require_device().bsm_dev_nd_factor_refactor_values(
        h, _lib.DTYPE_CODES[np.dtype(factor.src_dtype)], nnz, _p(vals), _stream(stream)))
    factor._vals_key = (vals.data_ptr(), vals._version, factor._epoch)
    factor._vals_ref = vals  # keeps the storage, so no other tensor can take its address while the record stands


def nd_factor_inv_pattern(factor, out: torch.Tensor | None = None, *, stream=None) -> torch.Tensor:
    """``(S^-1)[i, j]`` at every stored entry of the factored pattern, both
    triangles, into a device tensor (``bsm_dev_nd_factor_inv_pattern``):
    ``(pattern_nnz,)``, contiguous, of the factor's dtype, in the pattern's
    storage order; ``out`` defaults to a new tensor. The bits of
    ``NdFactor.inv_on(a).v`` without the host round trip. Runs on ``stream``
    and returns after it has drained."""
    from .sparse import _raise_for

    want = TORCH_DT[np.dtype(factor.dtype)]
    nnz = factor.pattern_nnz
    if out is None:
        factor._h()
        out = torch.empty((nnz,), dtype=want, device="cuda")
    if out.dtype != want:
        raise TypeError(f"nd_factor_inv_pattern: out is {out.dtype}, the factor is {factor.dtype}")
    if out.dim() != 1 or out.shape[0] != nnz or not out.is_contiguous():
        raise ValueError(f"nd_factor_inv_pattern: out must be contiguous, ({nnz},), got {tuple(out.shape)}")
    if not out.is_cuda:
        raise ValueError("nd_factor_inv_pattern: out is not on the device")
    h = factor._h()
    _raise_for(_lib.require_device().bsm_dev_nd_factor_inv_pattern(h, nnz, _p(out), _stream(stream)))
    return out


class Compactor:
    """Dense Y -> output Csr (the zero-dropping insert of sparse.rs:229) with
    preallocated worst-case buffers, so a timed step allocates nothing."""

    def __init__(self, rows: int, k: int, dtype, device="cuda"):
        lib = _lib.load()
        self.rows, self.k, self.dtype = rows, k, np.dtype(dtype)
        self.row_ptr = torch.empty(rows + 1, dtype=torch.int64, device=device)
        self.col = torch.empty(max(1, rows * k), dtype=torch.int32, device=device)
        self.vals = torch.empty(max(1, rows * k), dtype=TORCH_DT[self.dtype], device=device)
        self.ws_bytes = lib.bsm_dev_scan_workspace_bytes(rows)
        self.ws = torch.empty(max(16, self.ws_bytes), dtype=torch.uint8, device=device)

    def __call__(self, y: torch.Tensor, row_nnz: torch.Tensor, stream=None) -> None:
        lib = _lib.load()
        _lib.check(lib.bsm_dev_compact(_lib.DTYPE_CODES[self.dtype], self.rows, self.k, _p(y), _p(row_nnz),
                                       _p(self.row_ptr), _p(self.col), _p(self.vals), _p(self.ws), self.ws_bytes,
                                       _stream(stream)))

    def nnz(self) -> int:
        return int(self.row_ptr[self.rows].item())


def gen_insert_stream(seed, n, rows=1000, cols=1000, vmod=255, dtype=np.uint32, device="cuda"):
    """Bench-shaped insert stream on the device (bsm_dev_gen_insert_stream;
    benches/sparse_dense_mul.rs:16-22): (row u64, col u64, v dtype) tensors."""
    lib = _lib.require_device()
    dt = np.dtype(dtype)
    r = torch.empty(max(1, n), dtype=torch.uint64, device=device)
    c = torch.empty(max(1, n), dtype=torch.uint64, device=device)
    v = torch.empty(max(1, n), dtype=TORCH_DT[dt], device=device)
    _lib.check(lib.bsm_dev_gen_insert_stream(_lib.DTYPE_CODES[dt], seed, 0, n, rows, cols, vmod, _p(r), _p(c), _p(v),
                                             _stream()))
    return r[:n], c[:n], v[:n]


def csr_from_device_inserts(dims, row: torch.Tensor, col: torch.Tensor, v: torch.Tensor, stream=None):
    """bsm_dev_csr_from_inserts on device tensors -> a finalised host Csr
    whose device copy stays cached (Csr::insert x n, then finalise)."""
    from .sparse import Csr, _raise_for
    from .util import MatDim

    lib = _lib.require_device()
    d = MatDim.of(dims)
    dt = np.dtype(str(v.dtype).replace("torch.", ""))
    h = ctypes.c_void_p()
    rc = lib.bsm_dev_csr_from_inserts(_lib.DTYPE_CODES[dt], d.rows, d.cols, v.numel(), _p(row), _p(col), _p(v),
                                      ctypes.byref(h), _stream(stream))
    _raise_for(rc)
    return Csr._from_device(_lib.DeviceCsr(h.value))
