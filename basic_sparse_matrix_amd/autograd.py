"""A kept nd factor as a torch building block: the solve and the
log-determinant with gradients (``torch.autograd``).

``vals`` are the stored values of the factored matrix in its CSR storage
order, a device tensor; S is its stored entries with ``col <= row``, mirrored
(what every nd call factors; entries with ``col > row`` are ignored, and their
gradient is exactly 0).

* ``nd_solve(f, vals, b)``: ``x = S^-1 b``. With the upstream gradient ``G``
  and ``Λ = S^-1 G``: ``grad_b = Λ`` and ``grad_vals = -sddmm(Λ, x)`` on the
  factor's pattern (``device.nd_factor_sddmm``), one more solve and one kernel.
* ``nd_logdet(f, vals)``: ``log det S`` as a 0-dim float64 tensor. Its
  gradient is ``S^-1`` on the pattern (``device.nd_factor_inv_pattern``), twice
  that below the diagonal.

Every value stays in HBM; the compute is the library's HIP kernels and torch
only carries the graph. Not imported by the package's ``__init__`` (it needs
torch). Double backward is not supported, and in this version the factor's
dtype must be the factored matrix's."""

from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import device

__all__ = ["nd_solve", "nd_logdet"]


def _check(what: str, f, vals: torch.Tensor) -> None:
    """The host-side checks both functions share."""
    if np.dtype(f.dtype) != np.dtype(f.src_dtype):
        raise TypeError(f"{what}: the factor is {f.dtype} of a {f.src_dtype} matrix; a factor in another dtype than "
                        f"its matrix is not differentiable in this version")
    want = device.TORCH_DT[np.dtype(f.src_dtype)]
    if vals.dtype != want:
        raise TypeError(f"{what}: vals is {vals.dtype}, the factored matrix is {f.src_dtype}")
    if vals.dim() != 1 or vals.shape[0] != f.pattern_nnz or not vals.is_contiguous():
        raise ValueError(f"{what}: vals must be contiguous, ({f.pattern_nnz},), got {tuple(vals.shape)}")
    if not vals.is_cuda:
        raise ValueError(f"{what}: vals is not on the device")


def _factor_of(what: str, f, vals: torch.Tensor, refactor: bool) -> None:
    """Make ``f`` the factor of ``vals``, or check the caller's word that it is:
    the same address, the same version (no in-place edit since) and no rewrite
    of the factor since ``refactor_values`` recorded them. The factor keeps a
    reference to the recorded tensor for as long as the record stands, so a
    tensor made later cannot be handed its address and pass for it."""
    if refactor:
        device.nd_factor_refactor_values(f, vals.detach())
        return
    key = (vals.data_ptr(), vals._version, f._epoch)
    if f._vals_key != key:
        raise ValueError(f"{what}: refactor=False, but the factor is not the one refactor_values made of this tensor "
                         f"(other values, an in-place edit of vals, or the factor was rewritten since)")


def _same_epoch(what: str, f, epoch: int) -> None:
    if f._epoch != epoch:
        raise RuntimeError(f"{what}: the factor was rewritten between forward and backward ({f._epoch - epoch} "
                           f"refactor / update calls since): its values are no longer the forward's")


class _NdSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, vals, b):
        x = device.nd_factor_solve(f, b.detach())
        ctx.f, ctx.epoch = f, f._epoch
        ctx.save_for_backward(x)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        f = ctx.f
        _same_epoch("nd_solve backward", f, ctx.epoch)
        (x,) = ctx.saved_tensors
        need_vals, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need_vals or need_b):
            return None, None, None
        lam = device.nd_factor_solve(f, g.contiguous())
        grad_vals = device.nd_factor_sddmm(f, lam, x).neg_() if need_vals else None
        return None, grad_vals, lam if need_b else None


def _weights(f, dev: torch.device) -> torch.Tensor:
    """Per stored entry: 2 below the diagonal, 1 on it, 0 above, in the
    factor's dtype; built once per factor on ``dev`` (the device of ``vals``,
    which is the factor's) and kept on the factor until ``close()``:
    ``pattern_nnz`` values. The SDDMM of two columns of ones is exactly that:
    1*1 + 1*1 below, 1*1 on the diagonal and the mode's +0.0 above."""
    if f._grad_weights is None:
        one = torch.ones((f.n, 1), dtype=device.TORCH_DT[np.dtype(f.dtype)], device=dev)
        f._grad_weights = device.nd_factor_sddmm(f, one, one)
    return f._grad_weights


class _NdLogdet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, vals):
        ctx.f, ctx.epoch, ctx.dtype, ctx.device = f, f._epoch, vals.dtype, vals.device
        return torch.tensor(f.logdet(), dtype=torch.float64, device=vals.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        f = ctx.f
        _same_epoch("nd_logdet backward", f, ctx.epoch)
        if not ctx.needs_input_grad[1]:
            return None, None
        z = torch.empty((f.pattern_nnz,), dtype=device.TORCH_DT[np.dtype(f.dtype)], device=ctx.device)
        device.nd_factor_inv_pattern(f, out=z)
        return None, (z * _weights(f, ctx.device) * g).to(ctx.dtype)


def nd_solve(f, vals: torch.Tensor, b: torch.Tensor, *, refactor: bool = True) -> torch.Tensor:
    """``x = S^-1 b`` on the kept factor ``f`` (``solver.NdFactor``),
    differentiable in ``vals`` and ``b``. ``vals``: 1-D, contiguous, on the
    factor's device, of ``f.src_dtype``, ``f.pattern_nnz`` entries; ``b``:
    ``(n,)`` or row-major ``(n, k)`` as ``device.nd_factor_solve`` takes it.
    The forward refactors ``f`` from ``vals`` (``refactor_values``) and
    solves; ``refactor=False`` states that ``f`` already is the factor of
    exactly this tensor, as an earlier call or ``f.refactor_values(vals)``
    left it (``ValueError`` otherwise). The backward is one more solve and
    one SDDMM, and raises ``RuntimeError`` when the factor was rewritten since
    the forward."""
    _check("nd_solve", f, vals)
    _factor_of("nd_solve", f, vals, refactor)
    return _NdSolve.apply(f, vals, b)


def nd_logdet(f, vals: torch.Tensor, *, refactor: bool = True) -> torch.Tensor:
    """``log det S`` as a 0-dim float64 tensor on the device, differentiable
    in ``vals``; the arguments are :func:`nd_solve`'s. The backward is the
    selected inverse on the pattern (``device.nd_factor_inv_pattern``)."""
    _check("nd_logdet", f, vals)
    _factor_of("nd_logdet", f, vals, refactor)
    return _NdLogdet.apply(f, vals)
