"""MI355X propagation library -- the drop-in counterpart of `c3/libraries/propagation.py`.

Same registries, same provider names, same argument meaning and return dicts as
the reference (propagation.py:18-68, 258-341, 687-752), so
`Experiment.set_prop_method("pwc")` / `set_prop_method(c3_amd.propagation.pwc)`
(experiment.py:76-91) finds the HIP path.  All arithmetic happens in libc3prop.so
(hand-written gfx950 kernels behind the C ABI of include/c3prop.h); this file is
host orchestration only: it gathers the dense arrays `Model`/`Generator` hand
over, calls the library once per gate (or once per *batch* of parameter samples
through `propagate_batch`), and returns numpy arrays (or torch device tensors
when given device tensors).

There is no CPU fallback: without the built library and a GPU every entry point
raises `C3PropError("C3:Error: ...")`.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._cache import TensorMemo
from ._lib import C3PropError

unitary_provider: Dict[str, Callable] = dict()  # propagation.py:18
state_provider: Dict[str, Callable] = dict()  # :19
solver_dict: Dict[str, int] = dict(_lib.SOLVERS)  # :20 (ids of the device tableaux)
step_dict: Dict[str, int] = dict(_lib.STEPS)  # :21

# (stride, window, interpolation code) per solver -- propagation.py:27-32.  The
# device kernel evaluates the interpolated Hamiltonian at the same stage times
# without materialising `Hs`.
solver_slicing = {"rk4": [2, 3, 2], "rk38": [3, 4, 3], "rk5": [6, 6, -1], "tsit5": [6, 6, -2]}


def unitary_deco(func):
    """Registry decorator (propagation.py:39-44)."""
    unitary_provider[str(func.__name__)] = func
    return func


def state_deco(func):
    """Registry decorator (propagation.py:47-52)."""
    state_provider[str(func.__name__)] = func
    return func


# --------------------------------------------------------------------------
# array plumbing
# --------------------------------------------------------------------------


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _c128(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x), dtype=np.complex128)


def _f64(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x), dtype=np.float64)


def _ptr(a) -> Optional[int]:
    if a is None:
        return None
    if _is_torch(a):
        return a.data_ptr()
    return a.ctypes.data


class _Call:
    """Decides host-vs-device pointer mode for one library call and keeps arrays alive."""

    def __init__(self, *arrays):
        self.device = any(_is_torch(a) and a.is_cuda for a in arrays if a is not None)
        self.torch = None
        self.stream = None
        if self.device:
            import torch

            self.torch = torch
            dev = next(a.device for a in arrays if a is not None and _is_torch(a) and a.is_cuda)
            self.dev = dev
            torch.cuda.set_device(dev)
            self.stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.require_gpu()

    def c128(self, x):
        if x is None:
            return None
        if self.device:
            t = self.torch.as_tensor(x, device=self.dev) if not _is_torch(x) else x.to(self.dev)
            return t.to(self.torch.complex128).contiguous()
        return _c128(x.cpu().numpy() if _is_torch(x) else x)

    def f64(self, x):
        if x is None:
            return None
        if self.device:
            t = self.torch.as_tensor(x, device=self.dev) if not _is_torch(x) else x.to(self.dev)
            return t.to(self.torch.float64).contiguous()
        return _f64(x.cpu().numpy() if _is_torch(x) else x)

    def empty(self, shape):
        if self.device:
            return self.torch.empty(shape, dtype=self.torch.complex128, device=self.dev)
        return np.empty(shape, dtype=np.complex128)

    @property
    def flags(self) -> int:
        return 0 if self.device else _lib.HOST_PTRS


def _bstride(arr, base_ndim: int, B: int, what: str) -> int:
    """0 if `arr` is shared by all samples, else elements between consecutive samples."""
    if arr.ndim == base_ndim:
        return 0
    if arr.ndim == base_ndim + 1 and arr.shape[0] == B:
        n = 1
        for s in arr.shape[1:]:
            n *= int(s)
        return n
    raise C3PropError(f"C3:Error: {what} has shape {tuple(arr.shape)}; expected {base_ndim} dims or a leading batch of {B}")


def _col_per_sample(col, B: int):
    """(C, flag) of collapse operators [C,D,D] (one set for the batch) or [B,C,D,D] (one per sample: C3P_COL_PER_SAMPLE)."""
    return int(col.shape[-3]), (_lib.COL_PER_SAMPLE if _bstride(col, 3, B, "col_ops") else 0)


def _shared_col_only(col_ops, what: str) -> None:
    if col_ops is not None and not isinstance(col_ops, (list, tuple)) and getattr(col_ops, "ndim", 3) == 4:
        raise C3PropError(f"C3:Error: {what} takes one col_ops [C,D,D] for the batch; per-sample col_ops [B,C,D,D] are served by "
                          "propagate_batch(..., lindbladian=True) and propagate_batch_lindblad_vjp")


# --------------------------------------------------------------------------
# Batched entry point (the build's batch axis B; the reference loops in Python,
# optimalcontrol_robust.py:54-63, modellearning.py:305-318)
# --------------------------------------------------------------------------


def propagate_batch(
    h0,
    hks,
    signals,
    dt: float,
    *,
    col_ops=None,
    lindbladian: bool = False,
    fr_phase=None,
    want_dUs: bool = False,
    force_generic: bool = False,
    recheck_operators: bool = False,
) -> Dict:
    """U[b] for B independent parameter samples in one library call.

    h0       [D,D] | [B,D,D]             (branch A)   or, with hks=None/signals=None,
             [N,D,D] | [B,N,D,D]         per-slice Hamiltonians (branch B, propagation.py:295-308)
    hks      [K,D,D] | [B,K,D,D] | None
    signals  [B,K,N] real | None
    col_ops  [C,D,D] | [B,C,D,D] (lindbladian): one set of collapse operators for the batch, or one per sample
    fr_phase [B,Dm] real or None; U <- diag(exp(i phase)) U   (experiment.py:482-509)
    Returns {"U": [B,Dm,Dm], "dUs": [B,N,Dm,Dm] or None}, Dm = D (unitary) or D*D (Lindblad).

    `recheck_operators`: measure the hermiticity of device operator tensors again instead of trusting the per-tensor verdict
    (`forget_operators`; needed after a write through a raw pointer / DLPack view, which does not bump `_version`).
    """
    if recheck_operators:
        forget_operators(h0, hks)
    call = _Call(h0, hks, signals, col_ops, fr_phase)
    lib = _lib.load()
    flags = call.flags | (_lib.FORCE_GENERIC if force_generic else 0)
    h0 = call.c128(h0)
    D = int(h0.shape[-1])
    if signals is not None and hks is not None:
        signals = call.f64(signals)
        if signals.ndim != 3:
            raise C3PropError(f"C3:Error: signals must be [B,K,N], got {tuple(signals.shape)}")
        B, K, N = (int(s) for s in signals.shape)
        hks = call.c128(hks)
        h0_bs = _bstride(h0, 2, B, "h0")
        hk_bs = _bstride(hks, 3, B, "hks")
        if int(hks.shape[-3]) != K:
            raise C3PropError(f"C3:Error: {K} signal channels but {int(hks.shape[-3])} control Hamiltonians")
    else:
        flags |= _lib.PER_SLICE_H
        hks, signals, K, hk_bs = None, None, 0, 0
        if h0.ndim == 3:
            B, N, h0_bs = 1, int(h0.shape[0]), 0
        elif h0.ndim == 4:
            B, N = int(h0.shape[0]), int(h0.shape[1])
            h0_bs = N * D * D
        else:
            raise C3PropError(f"C3:Error: per-slice Hamiltonian must be [N,D,D] or [B,N,D,D], got {tuple(h0.shape)}")
    Dm = D * D if lindbladian else D
    if fr_phase is not None:
        fr_phase = call.f64(fr_phase)
        if tuple(fr_phase.shape) != (B, Dm):
            raise C3PropError(f"C3:Error: fr_phase must be [{B},{Dm}], got {tuple(fr_phase.shape)}")
    U = call.empty((B, Dm, Dm))
    dUs = call.empty((B, N, Dm, Dm)) if want_dUs else None
    if lindbladian:
        if col_ops is None:
            raise C3PropError("C3:Error: lindbladian propagation needs collapse operators")
        col = call.c128(col_ops if _is_torch(col_ops) else np.asarray(col_ops))
        C, col_flag = _col_per_sample(col, B)
        flags |= col_flag
        if D in (2, 3, 4) and not (flags & _lib.PER_SLICE_H) and not want_dUs and _is_hermitian(call, h0) and (K == 0 or _is_hermitian(call, hks)):
            # one qubit / qutrit with Hermitian Hamiltonians: the generator is real in the Hermitian basis (c3p_smallr.hip)
            flags |= _lib.HERMITIAN_H
        rc = lib.c3p_pwc_lindblad(
            _ptr(h0), h0_bs, _ptr(hks), hk_bs, _ptr(signals), _ptr(col), C, float(dt),
            B, K, N, D, flags, _ptr(fr_phase), _ptr(U), _ptr(dUs), call.stream,
        )
    else:
        _shared_col_only(col_ops, "the unitary propagation (lindbladian=False)")
        rc = lib.c3p_pwc_unitary(
            _ptr(h0), h0_bs, _ptr(hks), hk_bs, _ptr(signals), float(dt), B, K, N, D, flags,
            _ptr(fr_phase), _ptr(U), _ptr(dUs), call.stream,
        )
    _lib.check(rc)
    return {"U": U, "dUs": dUs}


_hermitian_memo = TensorMemo()  # per operator tensor OBJECT: the measured relative deviation |h - h^+| / |h| (both verdicts)


def forget_operators(*tensors) -> None:
    """Drop the cached hermiticity verdict of these operator tensors.  The verdict is kept per tensor object and
    `_version`; in-place writes that torch does not see -- a libc3prop output pointer, a DLPack / cupy view, another library's
    kernel -- leave `_version` unchanged, and a stale 'Hermitian' verdict would send a non-Hermitian operator down the real
    Hermitian-basis Lindblad kernels (D = 2..4) or past the gradient's hermiticity guard.  Call this (or pass
    `recheck_operators=True`) after such a write."""
    for t in tensors:
        if t is not None:
            _hermitian_memo.forget(t)


def _hermitian_deviation(call, h) -> float:
    """|h - h^+|_max / |h|_max.  Device tensors: measured ONCE per tensor object and `_version` (an optimiser calls with the same
    operator tensors every iteration; the measurement is two host synchronisations, which also break stream capture) -- the
    number is kept, so a tensor that FAILS a tolerance is not reduced again either.  Keyed on the object through a
    weak reference (c3_amd/_cache.py), not on its address."""
    if call.device:
        dev = _hermitian_memo.get(h, "dev")
        if dev is None:
            if h.numel() == 0:
                dev = 0.0
            else:
                d = float((h - h.conj().transpose(-1, -2)).abs().max().item())
                dev = d / max(float(h.abs().max().item()), 1e-300)
            _hermitian_memo.put(h, "dev", dev)
        return dev
    h = np.asarray(h)
    if h.size == 0:
        return 0.0
    return float(np.abs(h - np.conj(np.swapaxes(h, -1, -2))).max()) / max(float(np.abs(h).max()), 1e-300)


def _is_hermitian(call, h) -> bool:
    """|h - h^+| <= 1e-14 |h| (an empty operator set -- K = 0 -- is Hermitian)."""
    return _hermitian_deviation(call, h) <= 1e-14


def _require_hermitian(call, name, h, tol=1e-12):
    """The adjoint sweep assumes unitary slices, i.e. Hermitian Hamiltonians; the library only checks host-pointer
    inputs, so device tensors are checked here (once per operator tensor, see _hermitian_deviation)."""
    dev = _hermitian_deviation(call, h)
    if dev > tol:
        raise C3PropError(f"C3:Error: {name} must be Hermitian for the gradient (|h - h^+| / |h| = {dev:.3e})")


def propagate_batch_vjp(h0, hks, signals, dt: float, U_bar, *, fr_phase=None, force_generic: bool = False, want_model_grads: bool = False, check_hermitian: bool = True, recheck_operators: bool = False):
    """Vector-Jacobian product of `propagate_batch` (unitary, branch A) w.r.t. the control samples.

    The reference tapes the goal function (optimizers/optimizer.py:206-216) and lets TensorFlow
    differentiate propagation.py:426-440 + tf_utils.py:144-193; here the adjoint sweep runs on the
    device.  With d loss = Re sum conj(U_bar) dU, returns d loss / d signals as f64 [B,K,N].
    `U_bar` [B,D,D] for unitary_infid / average_infid comes from `fidelities.*_cotangent`.

    With `want_model_grads` returns `(grad_signals, grad_h0 [B,D,D], grad_hks [B,K,D,D])`: the cotangents of the
    Hamiltonians themselves (d loss = Re sum conj(grad_h) dh), contracted from the per-slice generator
    cotangents Z[b,n] -- what a model-parameter fit differentiates (optimizers/modellearning.py:300-341).
    """
    if recheck_operators:
        forget_operators(h0, hks)
    call = _Call(h0, hks, signals, U_bar, fr_phase)
    h0 = call.c128(h0)
    hks = call.c128(hks)
    signals = call.f64(signals)
    if signals.ndim != 3:
        raise C3PropError(f"C3:Error: signals must be [B,K,N], got {tuple(signals.shape)}")
    B, K, N = (int(s) for s in signals.shape)
    D = int(h0.shape[-1])
    h0_bs = _bstride(h0, 2, B, "h0")
    hk_bs = _bstride(hks, 3, B, "hks")
    if int(hks.shape[-3]) != K:
        raise C3PropError(f"C3:Error: {K} signal channels but {int(hks.shape[-3])} control Hamiltonians")
    if check_hermitian:
        _require_hermitian(call, "h0", h0)
        _require_hermitian(call, "hks", hks)
    U_bar = call.c128(U_bar)
    if tuple(U_bar.shape) != (B, D, D):
        raise C3PropError(f"C3:Error: U_bar must be [{B},{D},{D}], got {tuple(U_bar.shape)}")
    if fr_phase is not None:
        fr_phase = call.f64(fr_phase)
        if tuple(fr_phase.shape) != (B, D):
            raise C3PropError(f"C3:Error: fr_phase must be [{B},{D}], got {tuple(fr_phase.shape)}")
    if call.device:
        grad = call.torch.empty((B, K, N), dtype=call.torch.float64, device=call.dev)
    else:
        grad = np.empty((B, K, N), dtype=np.float64)
    Z = call.empty((B, N, D, D)) if want_model_grads else None
    _lib.check(
        _lib.load().c3p_pwc_unitary_vjp(
            _ptr(h0), h0_bs, _ptr(hks), hk_bs, _ptr(signals), float(dt), B, K, N, D, call.flags | (_lib.FORCE_GENERIC if force_generic else 0), _ptr(fr_phase), _ptr(U_bar), _ptr(grad), _ptr(Z), call.stream
        )
    )
    if not want_model_grads:
        return grad
    # G_n = -i dt (h0 + sum_k c_k(n) hk)  =>  h0_bar = conj(-i dt) sum_n Z_n,  hk_bar = conj(-i dt) sum_n c_k(n) Z_n
    if call.device:
        t = call.torch
        g0 = (1j * dt) * Z.sum(dim=1)
        gk = (1j * dt) * t.einsum("bkn,bnij->bkij", signals.to(t.complex128), Z)
    else:
        g0 = (1j * dt) * Z.sum(axis=1)
        gk = (1j * dt) * np.einsum("bkn,bnij->bkij", signals, Z)
    return grad, g0, gk


_goal_rows_cache: Dict[tuple, object] = {}


def goal_vjp_is_fused(B: int, D: int) -> bool:
    """Shapes `propagate_batch_goal_vjp` serves (the on-chip and VALU backward sweeps, include/c3prop.h)."""
    return D <= 40 or (D <= 64 and B < 384 and _lib.get_option("tiled_grad") <= 0)


def propagate_batch_goal_vjp(h0, hks, signals, dt: float, ideal, index, dims, *, kind: str = "unitary", fr_phase=None, want_U: bool = True, check_hermitian: bool = True, recheck_operators: bool = False):
    """Goal and gradient of one optimiser evaluation from ONE pass over the chains (c3p_pwc_unitary_goal_vjp).

    The reference evaluates `goal_run = fid_func(compute_propagators())` (optimizers/optimalcontrol.py:200-228) under a
    GradientTape (optimizers/optimizer.py:206-216).  Returns `{"goal": f64 [B], "grad_signals": f64 [B,K,N],
    "grad_fr_phase": f64 [B,D] or None, "U": c128 [B,D,D] or None}` with goal = unitary_infid (kind "unitary",
    fidelities.py:154-184) or average_infid ("average", :290-313) of every sample and grad = d goal[b] / d signals[b]."""
    from .fidelities import computational_rows

    if recheck_operators:
        forget_operators(h0, hks)
    call = _Call(h0, hks, signals, fr_phase, ideal)
    h0 = call.c128(h0)
    hks = call.c128(hks)
    signals = call.f64(signals)
    if signals.ndim != 3:
        raise C3PropError(f"C3:Error: signals must be [B,K,N], got {tuple(signals.shape)}")
    B, K, N = (int(s) for s in signals.shape)
    D = int(h0.shape[-1])
    h0_bs = _bstride(h0, 2, B, "h0")
    hk_bs = _bstride(hks, 3, B, "hks")
    if int(hks.shape[-3]) != K:
        raise C3PropError(f"C3:Error: {K} signal channels but {int(hks.shape[-3])} control Hamiltonians")
    if kind not in ("unitary", "average"):
        raise C3PropError(f"C3:Error: unknown infidelity kind '{kind}'")
    if dims is None or int(np.prod(dims)) != D:
        raise C3PropError(f"C3:Error: dims {dims} do not match the propagator dimension {D}")
    if check_hermitian:
        _require_hermitian(call, "h0", h0)
        _require_hermitian(call, "hks", hks)
    rows = computational_rows(dims, index)
    L = int(rows.shape[0])
    G = call.c128(ideal)
    if tuple(G.shape) != (L, L):
        raise C3PropError(f"C3:Error: ideal gate must be [{L},{L}] for index {index}, got {tuple(G.shape)}")
    if fr_phase is not None:
        fr_phase = call.f64(fr_phase)
        if tuple(fr_phase.shape) != (B, D):
            raise C3PropError(f"C3:Error: fr_phase must be [{B},{D}], got {tuple(fr_phase.shape)}")
    if call.device:
        t = call.torch
        key = (tuple(int(d) for d in dims), tuple(index) if index else None, str(call.dev))
        rows_d = _goal_rows_cache.get(key)
        if rows_d is None:
            rows_d = _goal_rows_cache[key] = t.as_tensor(rows, device=call.dev)
        goal = t.empty((B,), dtype=t.float64, device=call.dev)
        grad = t.empty((B, K, N), dtype=t.float64, device=call.dev)
        gph = t.empty((B, D), dtype=t.float64, device=call.dev) if fr_phase is not None else None
    else:
        rows_d = rows
        goal = np.empty((B,), dtype=np.float64)
        grad = np.empty((B, K, N), dtype=np.float64)
        gph = np.empty((B, D), dtype=np.float64) if fr_phase is not None else None
    U = call.empty((B, D, D)) if want_U else None
    _lib.check(
        _lib.load().c3p_pwc_unitary_goal_vjp(
            _ptr(h0), h0_bs, _ptr(hks), hk_bs, _ptr(signals), float(dt), B, K, N, D, call.flags, _ptr(fr_phase), _ptr(rows_d), L, _ptr(G),
            0 if kind == "unitary" else 1, _ptr(goal), _ptr(grad), _ptr(gph), _ptr(U), call.stream
        )
    )
    return {"goal": goal, "grad_signals": grad, "grad_fr_phase": gph, "U": U}


class LindbladTape:
    """The forward intermediates of one `propagate_batch_lindblad_taped` call (device memory owned by this object), as the
    reference's GradientTape keeps those of `tf_propagation_lind` (propagation.py:551-585 under optimizers/optimizer.py:206-216):
    `tape.vjp(U_bar)` returns d loss / d signals [B,K,N] without a second forward pass."""

    def __init__(self, buf, nbytes, segments, per_sample, signals, B, K, N, D, fr_phase, flags=0):
        self.buf, self.nbytes, self.segments, self.per_sample = buf, nbytes, segments, per_sample
        self.signals, self.B, self.K, self.N, self.D, self.fr_phase = signals, B, K, N, D, fr_phase
        self.flags = flags  # C3P_HERMITIAN_H as given to the forward call: it selects the layout of the tape

    def vjp(self, U_bar):
        import torch

        Dm = self.D * self.D
        U_bar = U_bar.to(torch.complex128).contiguous()
        if tuple(U_bar.shape) != (self.B, Dm, Dm):
            raise C3PropError(f"C3:Error: U_bar must be [{self.B},{Dm},{Dm}], got {tuple(U_bar.shape)}")
        dev = self.buf.device
        grad = torch.empty((self.B, self.K, self.N), dtype=torch.float64, device=dev)
        _lib.check(
            _lib.load().c3p_pwc_lindblad_vjp_taped(
                self.buf.data_ptr(), self.nbytes, self.segments, 1 if self.per_sample else 0, self.signals.data_ptr(), self.B, self.K, self.N, self.D, self.flags,
                _ptr(self.fr_phase), U_bar.data_ptr(), grad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream
            )
        )
        return grad


def lindblad_tape_supported(B: int, K: int, N: int, D: int) -> bool:
    import ctypes

    seg = ctypes.c_int(0)
    return int(_lib.load().c3p_pwc_lindblad_tape_bytes(B, K, N, D, ctypes.byref(seg))) > 0


def propagate_batch_lindblad_taped(h0, hks, signals, dt: float, col_ops, *, fr_phase=None, recheck_operators: bool = False):
    """`propagate_batch(..., lindbladian=True)` for device tensors that also records a `LindbladTape` (D = 2, 3; D = 7, 8, 9 with Hermitian
    Hamiltonians; c3p_pwc_lindblad_taped): returns {"U": [B,D^2,D^2], "tape": LindbladTape}.  One forward pass serves the
    superoperators AND their vector-Jacobian product (`tape.vjp`), where `propagate_batch` + `propagate_batch_lindblad_vjp`
    compute the chain twice."""
    import ctypes

    import torch

    if recheck_operators:
        forget_operators(h0, hks)
    _shared_col_only(col_ops, "the taped Lindblad evaluation")
    call = _Call(h0, hks, signals, col_ops, fr_phase)
    if not call.device:
        raise C3PropError("C3:Error: the taped Lindblad evaluation takes device tensors")
    h0 = call.c128(h0)
    hks = call.c128(hks)
    signals = call.f64(signals)
    col = call.c128(col_ops)
    if signals.ndim != 3:
        raise C3PropError(f"C3:Error: signals must be [B,K,N], got {tuple(signals.shape)}")
    B, K, N = (int(x) for x in signals.shape)
    D = int(h0.shape[-1])
    h0_bs = _bstride(h0, 2, B, "h0")
    hk_bs = _bstride(hks, 3, B, "hks")
    Dm = D * D
    if fr_phase is not None:
        fr_phase = call.f64(fr_phase)
        if tuple(fr_phase.shape) != (B, Dm):
            raise C3PropError(f"C3:Error: fr_phase must be [{B},{Dm}], got {tuple(fr_phase.shape)}")
    lib = _lib.load()
    seg = ctypes.c_int(0)
    nbytes = int(lib.c3p_pwc_lindblad_tape_bytes(B, K, N, D, ctypes.byref(seg)))
    if nbytes <= 0:
        raise C3PropError(f"C3:Error: the taped Lindblad evaluation serves D = 2, 3, 4 (up to 8 control lines, at least four slices) and D = 7, 8, 9 (up to 16), got D={D} K={K} N={N}")
    buf = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=call.dev)
    U = call.empty((B, Dm, Dm))
    tflags = _lib.HERMITIAN_H if D in (2, 3, 4) and _is_hermitian(call, h0) and _is_hermitian(call, hks) else 0
    _lib.check(
        lib.c3p_pwc_lindblad_taped(
            _ptr(h0), h0_bs, _ptr(hks), hk_bs, _ptr(signals), _ptr(col), int(col.shape[0]), float(dt), B, K, N, D,
            tflags, _ptr(fr_phase), _ptr(U),
            buf.data_ptr(), nbytes, int(seg.value), call.stream
        )
    )
    return {"U": U, "tape": LindbladTape(buf, nbytes, int(seg.value), bool(h0_bs or hk_bs), signals, B, K, N, D, fr_phase, tflags)}


def propagate_per_slice_vjp(hs, dt: float, U_bar, *, fr_phase=None):
    """Branch B of `pwc` (propagation.py:295-308: the model hands over one Hamiltonian per slice): vector-Jacobian
    product of `propagate_batch(hs, None, None, dt)` w.r.t. the Hamiltonians.  hs [N,D,D] or [B,N,D,D]; returns the
    cotangents of the Hamiltonians, [B,N,D,D] with d loss = Re sum conj(H_bar) dH (the slice generator is G_n = -i dt H_n, so
    H_bar = i dt Z with Z the generator cotangent the library returns) -- what the reference's tape propagates on into
    `model.get_Hamiltonian(signal)`."""
    call = _Call(hs, U_bar, fr_phase)
    hs = call.c128(hs)
    D = int(hs.shape[-1])
    if hs.ndim == 3:
        B, N, bs = 1, int(hs.shape[0]), 0
    elif hs.ndim == 4:
        B, N = int(hs.shape[0]), int(hs.shape[1])
        bs = N * D * D
    else:
        raise C3PropError(f"C3:Error: per-slice Hamiltonian must be [N,D,D] or [B,N,D,D], got {tuple(hs.shape)}")
    U_bar = call.c128(U_bar)
    if U_bar.ndim == 2:
        U_bar = U_bar[None]
    if hs.ndim == 3 and int(U_bar.shape[0]) != 1:
        B = int(U_bar.shape[0])  # one Hamiltonian stack shared by B cotangents
    if tuple(U_bar.shape) != (B, D, D):
        raise C3PropError(f"C3:Error: U_bar must be [{B},{D},{D}], got {tuple(U_bar.shape)}")
    if fr_phase is not None:
        fr_phase = call.f64(fr_phase)
        if tuple(fr_phase.shape) != (B, D):
            raise C3PropError(f"C3:Error: fr_phase must be [{B},{D}], got {tuple(fr_phase.shape)}")
    Z = call.empty((B, N, D, D))
    _lib.check(
        _lib.load().c3p_pwc_unitary_vjp(
            _ptr(hs), bs, None, 0, None, float(dt), B, 0, N, D, call.flags | _lib.PER_SLICE_H, _ptr(fr_phase), _ptr(U_bar), None, _ptr(Z), call.stream
        )
    )
    return (1j * dt) * Z


def propagate_batch_lindblad_vjp(h0, hks, signals, dt: float, col_ops, U_bar, *, fr_phase=None, recheck_operators: bool = False, want_model_grads: bool = False, hermitian_basis: bool = False):
    """Vector-Jacobian product of `propagate_batch(..., lindbladian=True)` w.r.t. the control samples: the reference
    tapes tf_propagation_lind (propagation.py:551-585) under the same GradientTape (optimizers/optimizer.py:206-216).
    `U_bar` [B,D^2,D^2] is the cotangent of the superoperators (d loss = Re sum conj(U_bar) dU); returns f64 [B,K,N].

    `col_ops` is [C,D,D] or, one set per sample, [B,C,D,D] (grad_col_ops[b] is then the cotangent of col_ops[b]).

    `want_model_grads`: (grad_signals, grad_h0 [B,D,D], grad_hks [B,K,D,D], grad_col_ops [B,C,D,D]) through
    c3p_pwc_lindblad_model_vjp -- per sample (sum over B for operators the batch shares), d loss = Re sum conj(grad) d(operator),
    every operator entry an independent complex number (nothing assumed Hermitian).  D <= 6.

    `hermitian_basis` (with `want_model_grads`): the same four results for D = 7, 8, 9 through c3p_pwc_lindblad_model_vjp_hb, the
    real Hermitian-basis sweep.  h0 / hks must be Hermitian (an error otherwise, never a fallback).  grad_col_ops is the full
    cotangent; grad_h0 / grad_hks are HERMITIAN matrices, the Hermitian part (g + g^+) / 2 of the general cotangent: a real
    generator only sees Hermitian perturbations of H, and Re sum conj(grad) dH is exact for every Hermitian dH."""
    if hermitian_basis and not want_model_grads:
        raise C3PropError("C3:Error: hermitian_basis selects the model-cotangent entry of the Hermitian-basis sweep: it needs want_model_grads=True")
    if recheck_operators:
        forget_operators(h0, hks)
    call = _Call(h0, hks, signals, U_bar, fr_phase, col_ops)
    h0 = call.c128(h0)
    hks = call.c128(hks)
    signals = call.f64(signals)
    if signals.ndim != 3:
        raise C3PropError(f"C3:Error: signals must be [B,K,N], got {tuple(signals.shape)}")
    B, K, N = (int(s) for s in signals.shape)
    D = int(h0.shape[-1])
    Dm = D * D
    h0_bs = _bstride(h0, 2, B, "h0")
    hk_bs = _bstride(hks, 3, B, "hks")
    if int(hks.shape[-3]) != K:
        raise C3PropError(f"C3:Error: {K} signal channels but {int(hks.shape[-3])} control Hamiltonians")
    if col_ops is None:
        raise C3PropError("C3:Error: lindbladian propagation needs collapse operators")
    col = call.c128(col_ops if _is_torch(col_ops) else np.asarray(col_ops))
    C, col_flag = _col_per_sample(col, B)
    U_bar = call.c128(U_bar)
    if tuple(U_bar.shape) != (B, Dm, Dm):
        raise C3PropError(f"C3:Error: U_bar must be [{B},{Dm},{Dm}], got {tuple(U_bar.shape)}")
    if fr_phase is not None:
        fr_phase = call.f64(fr_phase)
        if tuple(fr_phase.shape) != (B, Dm):
            raise C3PropError(f"C3:Error: fr_phase must be [{B},{Dm}], got {tuple(fr_phase.shape)}")
    if call.device:
        grad = call.torch.empty((B, K, N), dtype=call.torch.float64, device=call.dev)
    else:
        grad = np.empty((B, K, N), dtype=np.float64)
    if want_model_grads:
        g0, gk, gc = call.empty((B, D, D)), call.empty((B, K, D, D)), call.empty((B, C, D, D))
        entry = _lib.load().c3p_pwc_lindblad_model_vjp_hb if hermitian_basis else _lib.load().c3p_pwc_lindblad_model_vjp
        _lib.check(
            entry(
                _ptr(h0), h0_bs, _ptr(hks), hk_bs, _ptr(signals), _ptr(col), C, float(dt), B, K, N, D, call.flags | col_flag,
                _ptr(fr_phase), _ptr(U_bar), _ptr(grad), _ptr(g0), _ptr(gk), _ptr(gc), call.stream
            )
        )
        return grad, g0, gk, gc
    _lib.check(
        _lib.load().c3p_pwc_lindblad_vjp(
            _ptr(h0), h0_bs, _ptr(hks), hk_bs, _ptr(signals), _ptr(col), C, float(dt), B, K, N, D,
            call.flags | col_flag | (_lib.HERMITIAN_H if D in (2, 3, 4) and _is_hermitian(call, h0) and _is_hermitian(call, hks) else 0),
            _ptr(fr_phase), _ptr(U_bar), _ptr(grad), call.stream
        )
    )
    return grad


# --------------------------------------------------------------------------
# tf_utils counterparts on the device (tf_utils.py:120-193, 240-289)
# --------------------------------------------------------------------------


def tf_matmul_n(tensor_list, folding_stack: Optional[Sequence] = None):
    """Ordered product dU[N-1]...dU[0] (tf_utils.py:144-163).  The device kernel multiplies
    time-segments in parallel and combines them in order; `folding_stack` is accepted for
    signature parity (it only encodes N)."""
    return _chain(tensor_list, 0)


def tf_matmul_left(dUs):
    """tf.foldr(matmul): dU[N-1] @ ... @ dU[0]  (tf_utils.py:120-129)."""
    return _chain(dUs, 0)


def tf_matmul_right(dUs):
    """tf.foldl(matmul): dU[0] @ ... @ dU[N-1]  (tf_utils.py:132-141)."""
    return _chain(dUs, _lib.ORDER_RIGHT)


def _chain(dUs, order_flag):
    call = _Call(dUs)
    M = call.c128(dUs)
    squeeze = M.ndim == 3
    if squeeze:
        M = M[None]
    B, N, D = int(M.shape[0]), int(M.shape[1]), int(M.shape[-1])
    out = call.empty((B, D, D))
    _lib.check(_lib.load().c3p_matmul_chain(_ptr(M), B, N, D, call.flags | order_flag, _ptr(out), call.stream))
    return out[0] if squeeze else out


def expm(A, force_generic: bool = False):
    """Batched matrix exponential on the device: the tf.linalg.expm call sites
    (propagation.py:378,422,440,456,584)."""
    call = _Call(A)
    M = call.c128(A)
    shp = tuple(M.shape)
    D = shp[-1]
    n = 1
    for s in shp[:-2]:
        n *= int(s)
    Mf = M.reshape((n, D, D))
    out = call.empty((n, D, D))
    _lib.check(_lib.load().c3p_expm(_ptr(Mf), n, D, call.flags | (_lib.FORCE_GENERIC if force_generic else 0), _ptr(out), call.stream))
    return out.reshape(shp)


def _superop(A, which):
    call = _Call(A)
    M = call.c128(A)
    shp = tuple(M.shape)
    D = shp[-1]
    n = 1
    for s in shp[:-2]:
        n *= int(s)
    out = call.empty((n, D * D, D * D))
    _lib.check(_lib.load().c3p_superop(_ptr(M.reshape((n, D, D))), n, D, which, call.flags, _ptr(out), call.stream))
    return out.reshape(shp[:-2] + (D * D, D * D))


def tf_spre(A):
    """A (x) I (tf_utils.py:271-274)."""
    return _superop(A, 0)


def tf_spost(A):
    """I (x) A^T (tf_utils.py:277-280)."""
    return _superop(A, 1)


def tf_super(A):
    """spre(A) spost(A^dagger) = A (x) conj(A) (tf_utils.py:284-289)."""
    return _superop(A, 2)


def tf_kron(A, B):
    """Batched Kronecker product (tf_utils.py:257-267)."""
    call = _Call(A, B)
    a, b = call.c128(A), call.c128(B)
    if tuple(a.shape[:-2]) != tuple(b.shape[:-2]):
        raise C3PropError("C3:Error: tf_kron operands need equal batch shapes")
    Da, Db = int(a.shape[-1]), int(b.shape[-1])
    n = 1
    for s in a.shape[:-2]:
        n *= int(s)
    out = call.empty((n, Da * Db, Da * Db))
    _lib.check(
        _lib.load().c3p_kron(_ptr(a.reshape((n, Da, Da))), _ptr(b.reshape((n, Db, Db))), n, Da, Db, call.flags, _ptr(out), call.stream)
    )
    return out.reshape(tuple(a.shape[:-2]) + (Da * Db, Da * Db))


def Id_like(A):
    """Identity with A's batch shape (tf_utils.py:240-245)."""
    A = np.asarray(A)
    return np.broadcast_to(np.eye(A.shape[-1], dtype=A.dtype), A.shape).copy()


# --------------------------------------------------------------------------
# tf_batch_propagate / per-slice providers (propagation.py:349-585)
# --------------------------------------------------------------------------


def tf_batch_propagate(hamiltonian, hks, signals, dt, batch_size, col_ops=None, lindbladian=False):
    """dUs[N,Dm,Dm] for one gate (propagation.py:460-515).  `batch_size` bounded the
    reference's memory by chunking the time axis; the device kernel segments the time
    axis itself, so the value is accepted and ignored."""
    del batch_size
    if signals is not None:
        sig = np.asarray(signals)
        if np.iscomplexobj(sig):
            sig = sig.real  # the reference casts real signals to c128 (propagation.py:293)
        r = propagate_batch(hamiltonian, hks, sig[None], dt, col_ops=col_ops, lindbladian=lindbladian, want_dUs=True)
    else:
        r = propagate_batch(hamiltonian, None, None, dt, col_ops=col_ops, lindbladian=lindbladian, want_dUs=True)
    return r["dUs"][0]


def tf_propagation_vectorized(h0, hks, cflds_t, dt):
    """dU[n] = expm(-i H[n] dt) (propagation.py:426-440)."""
    return tf_batch_propagate(h0, hks, cflds_t, dt, None)


def tf_propagation_lind(h0, hks, col_ops, cflds_t, dt, history=False):
    """dU[n] = expm(L[n] dt) (propagation.py:551-585)."""
    return tf_batch_propagate(h0, hks, cflds_t, dt, None, col_ops=col_ops, lindbladian=True)


def tf_dU_of_t(h0, hks, cflds_t, dt):
    """Single slice (propagation.py:349-379)."""
    sig = np.real(np.asarray(cflds_t, dtype=np.complex128)).reshape(-1, 1)
    return tf_batch_propagate(h0, np.asarray(hks), sig, dt, None)[0]


def tf_dU_of_t_lind(h0, hks, col_ops, cflds_t, dt):
    """Single Lindblad slice (propagation.py:382-423)."""
    sig = np.real(np.asarray(cflds_t, dtype=np.complex128)).reshape(-1, 1)
    return tf_batch_propagate(h0, np.asarray(hks), sig, dt, None, col_ops=col_ops, lindbladian=True)[0]


@unitary_deco
def tf_propagation(h0, hks, cflds, dt):
    """Legacy list-of-dU provider (propagation.py:518-548)."""
    sig = np.real(np.asarray(cflds, dtype=np.complex128))
    dUs = tf_batch_propagate(h0, np.asarray(hks), sig, dt, None)
    return [dUs[i] for i in range(dUs.shape[0])]


def tf_expm(A, terms: int):
    """Fixed-length Taylor series (propagation.py:630-655), evaluated with device matmuls:
    the k-th term is the ordered product of k copies of A divided by k!."""
    A = _c128(A)
    r = np.broadcast_to(np.eye(A.shape[-1], dtype=np.complex128), A.shape) + A
    P = A
    for k in range(2, terms):
        P = _pairwise(P, A) / complex(k)
        r = r + P
    return r


def tf_expm_dynamic(A, acc: float = 1e-5):
    """Taylor series to accuracy (propagation.py:658-684)."""
    A = _c128(A)
    r = np.eye(A.shape[0], dtype=np.complex128) + A
    P = A
    k = 2.0
    while np.max(np.abs(P)) > acc:
        P = _pairwise(P, A) / k
        k += 1.0
        r = r + P
    return r


def _pairwise(X, Y):
    """X @ Y on the device through the ordered-chain entry ([.., 2, D, D] -> Y is slice 0)."""
    stack = np.stack([Y, X], axis=-3)  # chain computes M[1] @ M[0]
    shp = stack.shape
    flat = stack.reshape((-1, 2) + shp[-2:])
    return np.asarray(_chain(flat, 0)).reshape(shp[:-3] + shp[-2:])


def pwc_trott_drift(h0, hks, cflds_t, dt):
    """Trotterised-drift variant (propagation.py:443-457); eigh stays on the host
    (tf.linalg.eigh is out of scope), expm and products run on the device."""
    h0 = _c128(h0)
    hks = _c128(hks)
    c = np.asarray(cflds_t).astype(np.complex128)
    e, v = np.linalg.eigh(h0)
    dU0 = v @ np.diag(np.exp(-1.0j * e.real * complex(dt))) @ v.T
    ht = np.sum(c * hks, axis=0)
    comm = h0 @ ht - ht @ h0
    E = np.asarray(expm(-1.0j * ht * complex(dt)))
    right = dU0 + comm * complex(dt) ** 2 / 2.0
    return np.asarray(_chain(np.stack([right, E, dU0]), 0))


def evaluate_sequences(propagators: Dict, sequences: list):
    """Total propagator of gate sequences, multiplied from the left (propagation.py:588-627)."""
    gates = propagators
    first = np.asarray(list(gates.values())[0])
    dim = first.shape[0]
    out = []
    for seq in sequences:
        if len(seq) == 0:
            out.append(np.eye(dim, dtype=first.dtype))
        else:
            out.append(np.asarray(tf_matmul_left(np.asarray([np.asarray(gates[g]) for g in seq], dtype=np.complex128))))
    return out


# --------------------------------------------------------------------------
# pwc -- the north-star provider (propagation.py:258-341)
# --------------------------------------------------------------------------


def _uniform_ts(ts_list):
    ts_list = np.asarray(ts_list, dtype=np.float64)
    ts = ts_list.mean(axis=0)
    step = ts[1] - ts[0]
    if not np.all(ts_list.var(axis=0) < 1e-5 * step):
        raise Exception("C3Error:Something with the times happend.")
    if not np.all(np.var(ts[1:] - ts[:-1]) < 1e-5 * step):
        raise Exception("C3Error:Something with the times happend.")
    return ts


def gather_pwc_inputs(model, gen, instr):
    """The host half of `pwc` (propagation.py:282-321): dense arrays for one gate."""
    signal = gen.generate_signals(instr)
    if model.controllability:
        h0, hctrls = model.get_Hamiltonians()
        signals, hks, ts = [], [], None
        for key in signal:
            signals.append(np.asarray(signal[key]["values"], dtype=np.float64))
            ts = np.asarray(signal[key]["ts"])
            hks.append(np.asarray(hctrls[key]))
        signals = np.asarray(signals)
        hks = np.asarray(hks, dtype=np.complex128)
    else:
        h0 = np.asarray(model.get_Hamiltonian(signal))
        ts = _uniform_ts([np.asarray(sig["ts"])[1:] for sig in signal.values()])
        hks, signals = None, None
    dt = float(np.real(ts[1] - ts[0]))
    col_ops = None
    if model.lindbladian:
        col_ops = [np.asarray(c) for c in model.get_Lindbladians()]
        if model.max_excitations:
            cutter = np.asarray(model.ex_cutter)
            col_ops = [cutter @ c @ cutter.T for c in col_ops]
    return np.asarray(h0), hks, signals, ts, dt, col_ops


@unitary_deco
def pwc(model, gen, instr, folding_stack: list, batch_size=None) -> Dict:
    """Piecewise-constant propagator of one gate on the GPU.

    Same contract as the reference `pwc` (propagation.py:258-341): returns
    {"U": [Dm,Dm], "dUs": [N,Dm,Dm], "ts": ts}.  `folding_stack` and `batch_size`
    are accepted for call compatibility (experiment.py:472-478); the kernel does its
    own time segmentation and ordered reduction.
    """
    del folding_stack, batch_size
    h0, hks, signals, ts, dt, col_ops = gather_pwc_inputs(model, gen, instr)
    lind = bool(model.lindbladian)
    if signals is not None:
        r = propagate_batch(h0, hks, signals[None], dt, col_ops=col_ops, lindbladian=lind, want_dUs=True)
    else:
        r = propagate_batch(h0, None, None, dt, col_ops=col_ops, lindbladian=lind, want_dUs=True)
    U, dUs = np.asarray(r["U"][0]), np.asarray(r["dUs"][0])
    if model.max_excitations:
        # propagation.py:337-339: with the cut active U comes from tf_matmul_left (same
        # ordered product) and everything is embedded back into the full space
        U = model.blowup_excitations(U)
        C = np.asarray(model.ex_cutter)
        if lind:
            raise C3PropError("C3:Error: blow-up of a cut Lindblad superoperator is undefined in the reference")
        dUs = np.einsum("ia,nij,jb->nab", C, dUs, C)
    return {"U": U, "dUs": dUs, "ts": ts}


# --------------------------------------------------------------------------
# ODE state solver (propagation.py:687-752)
# --------------------------------------------------------------------------


def _ode_operands(h0, hks, signals, init_state, solver, step_function, col_ops, states_bar=None, target=None, vjp=False):
    """What c3p_ode_solve and c3p_ode_solve_vjp take in common, checked and converted: one flat tuple
    (call, lib, h0, hks, sig, col, Cn, init, init_bs, B, K, N, D, M, solver id, step id)."""
    _shared_col_only(col_ops, "the ODE solver")
    call = _Call(h0, hks, signals, init_state, col_ops, states_bar, target)
    lib = _lib.load()
    if solver not in solver_dict:
        raise C3PropError(f"C3:Error: unknown solver '{solver}'")
    if col_ops is not None:
        step_function = "lindblad"
    if step_function not in step_dict:
        raise C3PropError(f"C3:Error: unknown step function '{step_function}'")
    if vjp and (states_bar is None) == (target is None):
        raise C3PropError("C3:Error: exactly one of states_bar and target must be given")
    h0 = call.c128(h0)
    hks = call.c128(hks)
    sig = call.f64(signals)
    if sig.ndim != 3:
        raise C3PropError(f"C3:Error: signals must be [B,K,N], got {tuple(sig.shape)}")
    B, K, N = (int(s) for s in sig.shape)
    D = int(h0.shape[-1])
    # both entries take ONE set of operators for the whole batch (no per-sample strides in the ABI)
    if h0.ndim != 2 or tuple(h0.shape) != (D, D):
        raise C3PropError(f"C3:Error: ode solvers take one drift Hamiltonian [D,D], got {tuple(h0.shape)}")
    if hks.ndim != 3 or tuple(hks.shape) != (K, D, D):
        raise C3PropError(f"C3:Error: {K} signal channels need control Hamiltonians [{K},{D},{D}], got {tuple(hks.shape)}")
    M = 1 if step_function == "schrodinger" else D
    init = call.c128(init_state)
    if tuple(init.shape[-2:]) != (D, M):
        raise C3PropError(f"C3:Error: initial state must be [..,{D},{M}] for step '{step_function}', got {tuple(init.shape)}")
    init_bs = _bstride(init, 2, B, "init_state")
    col = None
    Cn = 0
    if step_function == "lindblad":
        if col_ops is None:
            raise C3PropError("C3:Error: the lindblad step needs collapse operators")
        col = call.c128(col_ops if _is_torch(col_ops) else np.asarray(col_ops))
        Cn = int(col.shape[0])
    return call, lib, h0, hks, sig, col, Cn, init, init_bs, B, K, N, D, M, solver_dict[solver], step_dict[step_function]


def ode_solve_batch(h0, hks, signals, dt, init_state, solver="rk4", step_function="schrodinger", col_ops=None, final_only=False):
    """RK integration of B independent samples: signals [B,K,N]; init [D,M] or [B,D,M]."""
    call, lib, h0, hks, sig, col, Cn, init, init_bs, B, K, N, D, M, solver_id, step_id = _ode_operands(
        h0, hks, signals, init_state, solver, step_function, col_ops)
    out = call.empty((B, D, M) if final_only else (B, N, D, M))
    rc = lib.c3p_ode_solve(
        _ptr(h0), _ptr(hks), _ptr(sig), _ptr(col), Cn, float(dt), B, K, N, D, solver_id, step_id, _ptr(init), init_bs,
        0 if final_only else 1, call.flags, _ptr(out), call.stream,
    )
    _lib.check(rc)
    return out


def _ode_vjp_call(h0, hks, signals, dt, init_state, solver, step_function, col_ops, states_bar, target, want_states):
    call, lib, h0, hks, sig, col, Cn, init, init_bs, B, K, N, D, M, solver_id, step_id = _ode_operands(
        h0, hks, signals, init_state, solver, step_function, col_ops, states_bar, target, True)
    bar = tgt = None
    bar_all = 0
    tgt_bs = 0
    if states_bar is not None:
        bar = call.c128(states_bar)
        if tuple(bar.shape) == (B, N, D, M):
            bar_all = 1
        elif tuple(bar.shape) != (B, D, M):
            raise C3PropError(f"C3:Error: states_bar must be [{B},{D},{M}] or [{B},{N},{D},{M}], got {tuple(bar.shape)}")
    else:
        tgt = call.c128(target)
        if tuple(tgt.shape) == (D, 1):
            tgt_bs = 0
        elif tuple(tgt.shape) == (B, D, 1):
            tgt_bs = D
        else:
            raise C3PropError(f"C3:Error: target must be a ket [{D},1] or [{B},{D},1], got {tuple(tgt.shape)}")
    if call.device:
        t = call.torch
        grad = t.empty((B, K, N), dtype=t.float64, device=call.dev)
        goal = t.empty((B,), dtype=t.float64, device=call.dev) if tgt is not None else None
    else:
        grad = np.empty((B, K, N), dtype=np.float64)
        goal = np.empty((B,), dtype=np.float64) if tgt is not None else None
    init_bar = call.empty((B, D, M))
    final = call.empty((B, D, M)) if want_states else None
    rc = lib.c3p_ode_solve_vjp(
        _ptr(h0), _ptr(hks), _ptr(sig), _ptr(col), Cn, float(dt), B, K, N, D, solver_id, step_id,
        _ptr(init), init_bs, _ptr(bar), bar_all, _ptr(tgt), tgt_bs, call.flags, _ptr(grad), _ptr(init_bar), _ptr(goal),
        _ptr(final), call.stream,
    )
    _lib.check(rc)
    return {"grad_signals": grad, "init_bar": init_bar, "goal": goal, "states": final}


def ode_solve_batch_vjp(h0, hks, signals, dt, init_state, states_bar, solver="rk4", step_function="schrodinger", col_ops=None, want_states=True):
    """Discrete adjoint of `ode_solve_batch` (c3p_ode_solve_vjp): `states_bar` is the cotangent of the final state [B,D,M]
    or of every trajectory state [B,N,D,M] (d loss = Re sum conj(states_bar) d states).  Returns {"grad_signals" [B,K,N],
    "init_bar" [B,D,M] (the cotangent of the initial state: consecutive gates chain through it), "goal": None,
    "states" [B,D,M] (the final state of the call's own forward pass)}.  Torch CUDA tensors in give torch CUDA tensors out."""
    return _ode_vjp_call(h0, hks, signals, dt, init_state, solver, step_function, col_ops, states_bar, None, want_states)


def ode_goal_vjp(h0, hks, signals, dt, init_state, target, solver="rk4", step_function="schrodinger", col_ops=None, want_states=True):
    """State-transfer goal and its gradient in one call: goal[b] = 1 - |<target|psi_N>| for state vectors (tf_ketket_fid),
    1 - sqrt(Re <target|rho_N|target>) for density matrices (tf_dmket_fid) -- state_transfer_from_states
    (fidelities.py:793-816) on the final state of the call's own forward pass; `target` is a ket [D,1] or [B,D,1].
    Returns the dict of `ode_solve_batch_vjp` with "goal" [B]."""
    return _ode_vjp_call(h0, hks, signals, dt, init_state, solver, step_function, col_ops, None, target, want_states)


def _ode_gate(model, gen, instr, init_state, solver, step_function, final_only):
    signal = gen.generate_signals(instr)
    col = [np.asarray(c) for c in model.get_Lindbladians()] if model.lindbladian else None
    if model.lindbladian:
        step_function = "lindblad"
    h0, hctrls = model.get_Hamiltonians()
    ts_list, signals, hks = [], [], []
    for key in signal:
        ts_list.append(np.asarray(signal[key]["ts"], dtype=np.float64))
        signals.append(np.asarray(signal[key]["values"], dtype=np.float64))
        hks.append(np.asarray(hctrls[key]))
    ts = _uniform_ts(ts_list)
    dt = float(ts[1] - ts[0])
    states = ode_solve_batch(
        np.asarray(h0), np.asarray(hks), np.asarray(signals)[None], dt, np.asarray(init_state), solver, step_function,
        col_ops=col, final_only=final_only,
    )
    return {"states": np.asarray(states[0]), "ts": ts.astype(np.complex128)}


@state_deco
def ode_solver(model, gen, instr, init_state, solver, step_function) -> Dict:
    """Trajectory of the state under explicit RK (propagation.py:687-721)."""
    return _ode_gate(model, gen, instr, init_state, solver, step_function, False)


@state_deco
def ode_solver_final_state(model, gen, instr, init_state, solver, step_function) -> Dict:
    """Final state only (propagation.py:724-752)."""
    return _ode_gate(model, gen, instr, init_state, solver, step_function, True)


# --------------------------------------------------------------------------
# Pre-bound batched call (no per-call argument massaging): used by bench.py and by
# optimiser loops that evaluate the same shapes repeatedly.
# --------------------------------------------------------------------------


class BatchPropagator:
    """Holds device-resident inputs/outputs for repeated `propagate_batch` calls of one shape.

    All tensors are torch CUDA tensors (complex128 / float64, contiguous).  `run()` issues
    exactly one C-ABI call on torch's current stream and returns the output tensor `U`
    (valid once that stream is synchronised).

    Closed systems at 2 <= D <= 12 with operators shared by the batch: the generator tables of the model (h0, hks, dt) are
    built once, here, into a model record the object owns (c3p_pwc_record_build), and `run()` hands it to the chain kernel
    (c3p_pwc_unitary_rec), whose workgroups then copy the tables instead of rebuilding them in every launch -- same kernel,
    same bits.  `run()` TRUSTS the record: after overwriting `self.h0` or `self.hks` in place call `rebuild_record()`.
    """

    def __init__(self, h0, hks, signals, dt, *, col_ops=None, fr_phase=None, want_dUs=False, force_generic=False, hermitian=None):
        import torch

        self.torch = torch
        _shared_col_only(col_ops, "BatchPropagator")
        _lib.require_gpu()
        self.lib = _lib.load()
        dev = signals.device
        self.dev = dev
        c128, f64 = torch.complex128, torch.float64
        self.h0 = h0.to(dev, c128).contiguous()
        self.hks = hks.to(dev, c128).contiguous()
        self.signals = signals.to(dev, f64).contiguous()
        self.B, self.K, self.N = (int(s) for s in self.signals.shape)
        self.D = int(self.h0.shape[-1])
        self.lind = col_ops is not None
        self.col = col_ops.to(dev, c128).contiguous() if self.lind else None
        self.Dm = self.D * self.D if self.lind else self.D
        self.fr = fr_phase.to(dev, f64).contiguous() if fr_phase is not None else None
        self.h0_bs = _bstride(self.h0, 2, self.B, "h0")
        self.hk_bs = _bstride(self.hks, 3, self.B, "hks")
        self.dt = float(dt)
        self.U = torch.empty((self.B, self.Dm, self.Dm), dtype=c128, device=dev)
        self.dUs = torch.empty((self.B, self.N, self.Dm, self.Dm), dtype=c128, device=dev) if want_dUs else None
        self.flags = _lib.FORCE_GENERIC if force_generic else 0
        # open systems of one qubit / qutrit / two qubits: Hermitian Hamiltonians run in real arithmetic (C3P_HERMITIAN_H).
        # hermitian = None: checked here, once (the tensors are held by this object); True / False: the caller's word
        if self.lind and self.D in (2, 3, 4) and not want_dUs:
            if hermitian is None:
                herm = lambda h: float((h - h.conj().transpose(-1, -2)).abs().max().item()) <= 1e-14 * max(float(h.abs().max().item()), 1e-300)
                hermitian = herm(self.h0) and (self.K == 0 or herm(self.hks))
            if hermitian:
                self.flags |= _lib.HERMITIAN_H
        # the model record (None where the library serves none for this call: open systems, per-sample operators, want_dUs,
        # force_generic, D outside 2 .. 12)
        self.record = None
        if not self.lind and self.h0_bs == 0 and self.hk_bs == 0 and not want_dUs and not force_generic:
            nbytes = int(self.lib.c3p_pwc_record_bytes(self.D, self.K))
            if nbytes:
                self.record = torch.empty(nbytes // 8, dtype=f64, device=dev)
                self.rebuild_record()

    def rebuild_record(self):
        """Build the model record again from `self.h0`, `self.hks` and `self.dt` as they are now: one small launch on torch's
        current stream.  For callers that overwrite the operators in place; a no-op where no record is held."""
        if self.record is None:
            return
        st = self.torch.cuda.current_stream(self.dev).cuda_stream
        _lib.check(self.lib.c3p_pwc_record_build(self.h0.data_ptr(), self.hks.data_ptr() if self.K else None, self.dt, self.K, self.D, 0,
                                                 self.record.data_ptr(), st))

    def run(self, out=None):
        """One C-ABI call on torch's current stream; `out` overrides the result tensor
        (lets callers double-buffer results, e.g. to overlap a gather with the next batch)."""
        U = self.U if out is None else out
        st = self.torch.cuda.current_stream(self.dev).cuda_stream
        if self.lind:
            rc = self.lib.c3p_pwc_lindblad(
                self.h0.data_ptr(), self.h0_bs, self.hks.data_ptr(), self.hk_bs, self.signals.data_ptr(),
                self.col.data_ptr(), int(self.col.shape[0]), self.dt, self.B, self.K, self.N, self.D, self.flags,
                None if self.fr is None else self.fr.data_ptr(), U.data_ptr(),
                None if self.dUs is None else self.dUs.data_ptr(), st,
            )
        else:
            rc = self.lib.c3p_pwc_unitary_rec(
                self.h0.data_ptr(), self.h0_bs, self.hks.data_ptr(), self.hk_bs, self.signals.data_ptr(), self.dt,
                self.B, self.K, self.N, self.D, self.flags, None if self.fr is None else self.fr.data_ptr(),
                U.data_ptr(), None if self.dUs is None else self.dUs.data_ptr(),
                None if self.record is None else self.record.data_ptr(), st,
            )
        _lib.check(rc)
        return U


# --------------------------------------------------------------------------
# rk4_unitary family (propagation.py:71-101, 104-218, 221-255)
# --------------------------------------------------------------------------


def sum_h0_hks(h0, hks, cf_t):
    """H(t) = H_0 + sum_k c_k H_k for one time (propagation.py:207-218); host helper."""
    h = np.array(h0, dtype=np.complex128)
    for k in range(len(hks)):
        h = h + complex(cf_t[k]) * np.asarray(hks[k], dtype=np.complex128)
    return h


def get_hs_of_t_ts(model, gen, instr, prop_res=1) -> Dict:
    """Hamiltonian samples for the RK "unitary" provider (propagation.py:104-204).

    Returns {"Hs", "ts", "dt"} like the reference plus the raw pieces the device kernel
    consumes ("h0", "hks", "signals" in branch A).  The generator resolution is multiplied
    by `prop_res` for the signal generation as in the reference (:143,193) and restored
    afterwards (the reference leaves it multiplied, which compounds on repeated calls).
    """
    old_res = gen.resolution
    gen.resolution = prop_res * gen.resolution
    try:
        signal = gen.generate_signals(instr)
    finally:
        gen.resolution = old_res
    out: Dict = {}
    if model.controllability:
        h0, hctrls = model.get_Hamiltonians()
        signals, hks, ts = [], [], None
        for key in signal:
            signals.append(np.asarray(signal[key]["values"], dtype=np.float64))
            ts = np.asarray(signal[key]["ts"])
            hks.append(np.asarray(hctrls[key]))
        signals = np.asarray(signals)
        hks = np.asarray(hks, dtype=np.complex128)
        out.update(h0=np.asarray(h0), hks=hks, signals=signals)
        out["Hs"] = np.asarray(h0)[None] + np.einsum("kn,kij->nij", signals.astype(np.complex128), hks)
    else:
        out["Hs"] = np.asarray(model.get_Hamiltonian(signal))
        ts = _uniform_ts([np.asarray(sig["ts"])[1:] for sig in signal.values()])
    out["dt"] = complex(ts[1 * prop_res] - ts[0])
    out["ts"] = ts[::prop_res]
    return out


def _rk4_unitary_device(Hs=None, h0=None, hks=None, signals=None, dt=0.0, want_dUs=True):
    """One gate (B=1) through c3p_rk4_unitary.  Either Hs [Ns,D,D] or (h0, hks, signals[K,Ns])."""
    lib = _lib.load()
    call = _Call(Hs, h0, hks, signals)
    if Hs is not None and signals is None:
        hs = call.c128(Hs)
        Ns, D = int(hs.shape[0]), int(hs.shape[-1])
        h0p = hkp = sgp = None
        K = 0
    else:
        hs = None
        h0p = call.c128(h0)
        hkp = call.c128(hks)
        sgp = call.f64(np.asarray(signals)[None])
        K, Ns, D = int(sgp.shape[1]), int(sgp.shape[2]), int(h0p.shape[-1])
    nst = (Ns - 1) // 2
    U = call.empty((1, D, D))
    dUs = call.empty((1, nst, D, D)) if want_dUs else None
    rc = lib.c3p_rk4_unitary(_ptr(h0p), _ptr(hkp), _ptr(sgp), _ptr(hs), 0, float(np.real(dt)), 1, K, Ns, D, call.flags,
                             _ptr(U), _ptr(dUs), call.stream)
    _lib.check(rc)
    return U[0], (dUs[0] if want_dUs else None)


def rk4_step(h, psi, dt):
    """One RK4 step of psi under h[0], h[1], h[2] (propagation.py:95-101) on the device."""
    h = _c128(h)
    D = h.shape[-1]
    U, _ = _rk4_unitary_device(Hs=h[:3], dt=dt, want_dUs=False)
    return np.asarray(U) @ np.asarray(psi, dtype=np.complex128).reshape(D)


def gen_du_rk4(h, dt, dim):
    """Per-step map with propagated basis vectors as rows (propagation.py:85-92)."""
    _, dUs = _rk4_unitary_device(Hs=_c128(h)[:3], dt=dt)
    return np.asarray(dUs[0])


@unitary_deco
def gen_dus_rk4(h, dt, dim=None):
    """List of per-step maps (propagation.py:71-82)."""
    _, dUs = _rk4_unitary_device(Hs=_c128(h), dt=dt)
    dUs = np.asarray(dUs)
    return [dUs[i] for i in range(dUs.shape[0])]


def gen_u_rk4(h, dt, dim):
    """Total RK4 propagator, columns = propagated basis vectors (propagation.py:246-255)."""
    U, _ = _rk4_unitary_device(Hs=_c128(h), dt=dt, want_dUs=False)
    return np.asarray(U)


@unitary_deco
def rk4_unitary(model, gen, instr, init_state=None) -> Dict:
    """RK4 "unitary" provider (propagation.py:221-243): prop_res = 2."""
    prop_res = 2
    d = get_hs_of_t_ts(model, gen, instr, prop_res)
    if "signals" in d:
        U, dUs = _rk4_unitary_device(h0=d["h0"], hks=d["hks"], signals=d["signals"], dt=d["dt"])
    else:
        U, dUs = _rk4_unitary_device(Hs=d["Hs"], dt=d["dt"])
    U, dUs = np.asarray(U), np.asarray(dUs)
    if model.max_excitations:
        C = np.asarray(model.ex_cutter)
        U = model.blowup_excitations(U)
        dUs = np.einsum("ia,nij,jb->nab", C, dUs, C)
    return {"U": U, "dUs": dUs, "ts": d["ts"]}
