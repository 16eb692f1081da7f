"""Dressing of batched models on the device.

The reference dresses one model before every evaluation, `Model.update_dressed` (c3/model.py:453-534): an eigendecomposition of
the drift Hamiltonian, the reorder-and-sign rule of `reorder_frame`, and T^+ A T for every control and collapse operator.
`dress_batch` does that for P parameter sets in one launch (c3p_dress), `dress_batch_vjp` pulls cotangents of the dressed
operators back to the bare ones (c3p_dress_vjp), so that with a bare Hamiltonian linear in the model parameters,
H = sum_t theta_t G_t, `model_learning.model_param_grads(grad_H, ..., dh0=G)` gives exact parameter gradients.

numpy in, numpy out; torch device tensors in, tensors on that device out.  2 <= D <= 40, `ordered=True` only.
"""
from __future__ import annotations

import warnings
from typing import Dict, Optional

import numpy as np

from . import _lib
from ._lib import C3PropError
from .propagation import _Call, _hermitian_deviation, _is_torch, _ptr

MAX_D = 40
RECOVERED, DEGENERATE, NOT_CONVERGED = 1, 2, 4


def _empty(call, shape, kind):
    """An output buffer where the call's inputs live: kind "c" complex128, "d" float64, "i" int32."""
    if call.device:
        dt = {"c": call.torch.complex128, "d": call.torch.float64, "i": call.torch.int32}[kind]
        return call.torch.empty(shape, dtype=dt, device=call.dev)
    return np.empty(shape, dtype={"c": np.complex128, "d": np.float64, "i": np.int32}[kind])


def _host(x) -> np.ndarray:
    return x.cpu().numpy() if _is_torch(x) else np.asarray(x)


def _shapes(H, ops):
    """(P, D, M, ops_bstride, squeeze) of H [D,D] / [P,D,D] and ops None / [M,D,D] / [P,M,D,D]."""
    if H.ndim not in (2, 3) or H.shape[-1] != H.shape[-2]:
        raise C3PropError(f"C3:Error: H_bare has shape {tuple(H.shape)}; expected [D,D] or [P,D,D]")
    squeeze = H.ndim == 2
    P, D = (1 if squeeze else int(H.shape[0])), int(H.shape[-1])
    if D < 2 or D > MAX_D:
        raise C3PropError(f"C3:Error: the device dressing serves 2 <= D <= {MAX_D}, got D = {D}")
    M, bstride = 0, 0
    if ops is not None:
        if ops.ndim not in (3, 4) or tuple(ops.shape[-2:]) != (D, D):
            raise C3PropError(f"C3:Error: ops has shape {tuple(ops.shape)}; expected [M,{D},{D}] or [P,M,{D},{D}]")
        M = int(ops.shape[-3])
        if ops.ndim == 4:
            if int(ops.shape[0]) != P:
                raise C3PropError(f"C3:Error: ops holds {int(ops.shape[0])} operator lists, but there are {P} parameter sets")
            bstride = M * D * D
    return P, D, M, bstride, squeeze


def dress_batch(H_bare, ops=None, *, check_hermitian: bool = True) -> Dict:
    """`Model.update_dressed` for P parameter sets in one launch.

    `H_bare` [D,D] or [P,D,D]: the bare drift Hamiltonians; `ops` [M,D,D] (shared by the sets) or [P,M,D,D]: control Hamiltonians
    and collapse operators in one list.  Returns
      "eigenframe" [P,D]   the eigenvalues, reordered by overlap with the bare states;
      "transform" [P,D,D]  T, column i the eigenvector assigned to bare state i, T[i,i] real and positive (for a real drift the
                           reference's sign rule; for a complex Hermitian one the reference depends on LAPACK's phases, this defines it);
      "h0" [P,D,D]         diag(eigenframe), exactly;
      "ops" [P,M,D,D]      T^+ A_m T (None without `ops`);
      "status" int32 [P]   bit 1: the greedy recovery ordered the states (warned about, as the reference does).
    A set whose solve does not converge (NaN input) raises.  A leading axis is dropped from every result when H_bare is [D,D]."""
    call = _Call(H_bare, ops)
    H = call.c128(H_bare)
    A = call.c128(ops)
    P, D, M, bstride, squeeze = _shapes(H, A)
    if check_hermitian:
        dev = _hermitian_deviation(call, H)
        if dev > 1e-12:
            raise C3PropError(f"C3:Error: H_bare must be Hermitian to be dressed (|h - h^+| / |h| = {dev:.3e})")
    eig = _empty(call, (P, D), "d")
    T = _empty(call, (P, D, D), "c")
    h0 = _empty(call, (P, D, D), "c")
    out = _empty(call, (P, M, D, D), "c") if M else None
    status = _empty(call, (P,), "i")
    _lib.check(_lib.load().c3p_dress(_ptr(H), _ptr(A) if M else None, bstride, P, M, D, call.flags, _ptr(eig), _ptr(T), _ptr(h0), _ptr(out), _ptr(status),
                                     call.stream))
    st = _host(status)
    if (st & NOT_CONVERGED).any():
        raise C3PropError(f"C3:Error: the eigensolver did not converge for parameter set {int(np.argmax(st & NOT_CONVERGED))} (is H_bare finite?)")
    if (st & RECOVERED).any():
        warnings.warn(f"C3 Warning: Some states are overly dressed, trying to recover...{int(np.count_nonzero(st & RECOVERED))} parameter sets, "
                      f"{int(np.argmax(st & RECOVERED))} is lowest failed set")
    pick = (lambda x: None if x is None else x[0]) if squeeze else (lambda x: x)
    return {"h0": pick(h0), "ops": pick(out), "eigenframe": pick(eig), "transform": pick(T), "status": pick(status)}


def dress_batch_vjp(transform, eigenframe, ops=None, *, grad_h0=None, grad_ops=None, grad_eigenframe=None, grad_transform=None) -> Dict:
    """Vector-Jacobian product of `dress_batch` (d L = Re sum conj(Xbar) dX), from its "transform" and "eigenframe" -- nothing
    is solved again -- and the bare `ops` it was given.  Cotangents: `grad_h0` [P,D,D] (only Re diag enters: h0 = diag(eigenframe)),
    `grad_ops` [P,M,D,D], `grad_eigenframe` [P,D], `grad_transform` [P,D,D]; any may be None.  Returns
      "grad_H" [P,D,D]    the gradient on the Hermitian H_bare (Hermitian);
      "grad_ops"          cotangent of the bare operators: [P,M,D,D] for per-set `ops`, [M,D,D] summed over the sets for shared ones;
      "status" int32 [P]  bit 2: two eigenvalues closer than 2^-40 max|e|; the pair contributes zero (the reference: inf)."""
    call = _Call(transform, eigenframe, ops, grad_h0, grad_ops, grad_eigenframe, grad_transform)
    T = call.c128(transform)
    A = call.c128(ops)
    P, D, M, bstride, squeeze = _shapes(T, A)
    lead = (lambda x: None if x is None else x[None]) if squeeze else (lambda x: x)
    T = T.reshape((P, D, D))
    e = lead(call.f64(eigenframe))
    gh, go, ge, gt = lead(call.c128(grad_h0)), lead(call.c128(grad_ops)), lead(call.f64(grad_eigenframe)), lead(call.c128(grad_transform))
    for name, x, shape in (("eigenframe", e, (P, D)), ("grad_h0", gh, (P, D, D)), ("grad_ops", go, (P, M, D, D)), ("grad_eigenframe", ge, (P, D)),
                           ("grad_transform", gt, (P, D, D))):
        if x is not None and tuple(x.shape) != shape:
            raise C3PropError(f"C3:Error: {name} has shape {tuple(x.shape)}, expected {shape}")
    if go is not None and M == 0:
        raise C3PropError("C3:Error: grad_ops needs the bare ops dress_batch was given")
    want_ops = go is not None
    gH = _empty(call, (P, D, D), "c")
    gA = _empty(call, (P, M, D, D) if bstride else (M, D, D), "c") if want_ops else None
    status = _empty(call, (P,), "i")
    _lib.check(_lib.load().c3p_dress_vjp(_ptr(T), _ptr(e), _ptr(A) if want_ops else None, bstride, P, M if want_ops else 0, D, call.flags, _ptr(ge), _ptr(gh),
                                         _ptr(go), _ptr(gt), _ptr(gH), _ptr(gA), _ptr(status), call.stream))
    pick = (lambda x: None if x is None else x[0]) if squeeze else (lambda x: x)
    return {"grad_H": pick(gH), "grad_ops": pick(gA) if bstride else gA, "status": pick(status)}
