"""Read-out model of model learning on the device: confusion matrix, rescale, estimators.

The reference turns populations into simulated measurement values in `Experiment.process` (c3/experiment.py:355-407): the
confusion matrix of `ConfusionMatrix.confuse` (c3/libraries/tasks.py:107-129), the selection of state labels, the linear
`MeasurementRescale.rescale` (:161-178); an estimator of c3/libraries/estimators.py then scores them against the measured values.
`readout_goal` does all of that for P parameter sets in one call (c3p_readout_goal) from the sequence states, `readout_goal_vjp`
returns the cotangent of the states and of the read-out parameters as well (c3p_readout_goal_vjp).

numpy in, numpy out (host pointers); torch device tensors in, tensors on that device out (current stream).
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import C3PropError
from .propagation import _Call, _is_torch, _ptr

# the split of the kernels over the sequences of a set (csrc/c3p_readout.h): a workgroup of the element-wise kernels serves
# SEQ_BLOCK sequences; the per-set sums stride over the S V values with REDUCE_THREADS
SEQ_BLOCK = 32
REDUCE_THREADS = 256

# include/c3prop.h: C3P_EST_*
ESTIMATORS = {"g_LL_prime": 0, "neg_loglkh_gauss": 1, "neg_loglkh_gauss_norm": 2, "neg_loglkh_gauss_norm_sum": 3, "rms_dist": 4,
              "rms_exp_stds_dist": 5, "rms_sim_stds_dist": 6}
_NOT_SERVED = ("mean_dist", "median_dist", "mean_sim_stds_dist", "mean_exp_stds_dist", "std_of_diffs", "neg_loglkh_binom",
               "neg_loglkh_binom_norm", "neg_loglkh_multinom", "neg_loglkh_multinom_norm")


@dataclass
class Readout:
    """The SPAM parameters of a model.  `conf_rows[q]` [d_q] or [P,d_q]: the confusion row of subsystem q (None: no confusion
    matrix); `meas_scale` / `meas_offset`: scalars or [P] (None: no rescale; one of them alone leaves the other at 1 / 0);
    `dims`: the subsystem dimensions (needed for state labels given as tuples; else optional)."""

    conf_rows: Optional[Sequence] = None
    meas_scale: Optional[object] = None
    meas_offset: Optional[object] = None
    dims: Optional[Sequence[int]] = None


def estimator_id(name: str) -> int:
    if name in ESTIMATORS:
        return ESTIMATORS[name]
    if name in _NOT_SERVED:
        raise C3PropError(f"C3:Error: estimator {name!r} is not served on the device (not differentiable at 0, not a mean, or needs lgamma); "
                          f"served are {sorted(ESTIMATORS)}")
    raise C3PropError(f"C3:Error: unknown estimator {name!r}; served are {sorted(ESTIMATORS)}")


def _kron_last2(a, b):
    """Kronecker product over the last two axes, leading axes broadcast."""
    out = a[..., :, None, :, None] * b[..., None, :, None, :]
    return out.reshape(tuple(out.shape[:-4]) + (int(a.shape[-2]) * int(b.shape[-2]), int(a.shape[-1]) * int(b.shape[-1])))


def _stack2(a, b):
    if _is_torch(a):
        import torch

        return torch.stack([a, b], -2)
    return np.stack([a, b], -2)


def confusion_matrix(rows):
    """`ConfusionMatrix.confuse`'s matrix (tasks.py:122-127): the Kronecker product, first subsystem slowest, of [[row],[1-row]].
    `rows[q]` is [d_q] or [P,d_q] (numpy arrays or tensors of one device); the result [2^Q, D] or [P,2^Q,D]."""
    rows = [r if _is_torch(r) else np.asarray(r, dtype=np.float64) for r in rows]
    if not rows:
        raise C3PropError("C3:Error: a confusion matrix needs at least one row")
    for r in rows:
        if r.ndim not in (1, 2):
            raise C3PropError(f"C3:Error: a confusion row has shape {tuple(r.shape)}; expected [d_q] or [P,d_q]")
    mat = None
    for r in rows:
        m = _stack2(r, 1.0 - r)  # [...,2,d_q]
        if mat is None:
            mat = m
        else:
            if mat.ndim != m.ndim:  # one of them per set: the other gets the leading axis
                mat, m = (mat[None], m) if mat.ndim < m.ndim else (mat, m[None])
            mat = _kron_last2(mat, m)
    return mat


def confusion_matrix_vjp(rows, conf_bar) -> List:
    """Cotangents of every row from `conf_bar` [P,2^Q,D] (or [2^Q,D]): d loss = sum conf_bar dCm.  Every result is per set,
    [P,d_q] ([d_q] for a [2^Q,D] cotangent), also for a shared row: sum over p then.  Stays where its inputs are."""
    is_t = _is_torch(conf_bar)
    if is_t:
        import torch

        rows = [torch.as_tensor(r, dtype=torch.float64, device=conf_bar.device) for r in rows]
        einsum = torch.einsum
    else:
        conf_bar = np.asarray(conf_bar, dtype=np.float64)
        rows = [np.asarray(r, dtype=np.float64) for r in rows]
        einsum = np.einsum
    Q = len(rows)
    if Q > 8:
        raise C3PropError("C3:Error: confusion_matrix_vjp serves up to 8 subsystems")
    squeeze = conf_bar.ndim == 2
    cb = conf_bar[None] if squeeze else conf_bar
    P = int(cb.shape[0])
    dims = [int(r.shape[-1]) for r in rows]
    if tuple(cb.shape[1:]) != (2**Q, int(np.prod(dims))):
        raise C3PropError(f"C3:Error: conf_bar has shape {tuple(conf_bar.shape)}, expected [P,{2 ** Q},{int(np.prod(dims))}]")
    cb = cb.reshape((P,) + (2,) * Q + tuple(dims))
    ms = []
    for r in rows:
        m = _stack2(r, 1.0 - r)
        ms.append(m[None].expand(P, -1, -1) if (is_t and m.ndim == 2) else (np.broadcast_to(m[None], (P,) + m.shape) if m.ndim == 2 else m))
    up, lo = "ABCDEFGH", "abcdefgh"
    out = []
    for q in range(Q):
        others = [k for k in range(Q) if k != q]
        spec = "z" + up[:Q] + lo[:Q] + "".join(",z" + up[k] + lo[k] for k in others) + "->z" + up[q] + lo[q]
        mbar = einsum(spec, cb, *[ms[k] for k in others])  # [P,2,d_q]
        g = mbar[:, 0] - mbar[:, 1]
        out.append(g[0] if squeeze else g)
    return out


def label_weights(dims: Sequence[int], labels: Sequence[Sequence[int]], computational: bool):
    """The weight vector of a label selection (experiment.py:380-400): w[r] = how often label r is listed, over
    `comp_state_labels` (levels {0,1} per subsystem, model.py:147-159; what the rows of a confusion matrix mean) when
    `computational`, else over `state_labels`."""
    space = [[0, 1] if computational else list(range(int(d))) for d in dims]
    state_labels = list(itertools.product(*space))
    w = np.zeros(len(state_labels))
    for label in labels:
        try:
            w[state_labels.index(tuple(label))] += 1.0
        except ValueError:
            raise C3PropError(f"C3:ERROR:State {label} not defined. Available are:\n{state_labels}")
    return w


def stack_data(data_sets: Sequence[Dict], device=None) -> Dict:
    """{"results", "results_std", "shots"} [P,S] or [P,S,V] from the data sets of `goal_run_batched`; tensors on `device` if given."""
    res = np.stack([np.asarray(d["results"], dtype=np.float64) for d in data_sets])
    if any(np.shape(d["results"]) != res.shape[1:] for d in data_sets):
        raise C3PropError("C3:Error: the results of the data sets differ in shape")
    std = np.stack([np.broadcast_to(np.asarray(d["results_std"], dtype=np.float64), res.shape[1:]) for d in data_sets])
    sh = np.stack([np.broadcast_to(np.asarray(d["shots"], dtype=np.float64), res.shape[1:]) for d in data_sets])
    out = {"results": res, "results_std": std, "shots": sh}
    if device is not None:
        import torch

        out = {k: torch.as_tensor(np.ascontiguousarray(v), device=device) for k, v in out.items()}
    return out


def _weights_of(readout: Readout, labels, R: int, D: int):
    """`labels` None, a list of row indices, or a list of label tuples -> the weight vector [R] or None."""
    if labels is None:
        return None
    labels = list(labels)
    if labels and np.ndim(labels[0]) > 0:
        if readout.dims is None:
            raise C3PropError("C3:Error: state labels given as tuples need Readout.dims")
        return label_weights(readout.dims, labels, readout.conf_rows is not None)
    w = np.zeros(R)
    for i in labels:
        if not 0 <= int(i) < R:
            raise C3PropError(f"C3:Error: label index {int(i)} outside the {R} read-out rows")
        w[int(i)] += 1.0  # a label listed twice counts twice, as in process_batch
    return w


def _run(vjp: bool, x, readout: Optional[Readout], data, labels, estimator: str, weights, dim: Optional[int], want_pop_bar: bool = False) -> Dict:
    readout = Readout() if readout is None else readout
    est = estimator_id(estimator)
    if isinstance(data, (list, tuple)):
        data = stack_data(data)
    call = _Call(x, data["results"])
    xs = call.c128(x)
    if xs.ndim != 3:
        raise C3PropError(f"C3:Error: x has shape {tuple(xs.shape)}; expected the sequence states [P,S,M]")
    P, S, M = (int(n) for n in xs.shape)
    conf = None
    if readout.conf_rows is not None:
        conf = confusion_matrix([call.f64(r if _is_torch(r) else np.asarray(r, dtype=np.float64)) for r in readout.conf_rows])
        conf = conf.contiguous() if call.device else np.ascontiguousarray(conf)
    if dim is not None:
        D = int(dim)
    elif readout.dims is not None:
        D = int(np.prod(readout.dims))
    elif conf is not None:
        D = int(conf.shape[-1])
    else:
        D = M  # kets
    R = D if conf is None else int(conf.shape[-2])
    if conf is not None and int(conf.shape[-1]) != D:
        raise C3PropError(f"C3:Error: the confusion rows span {int(conf.shape[-1])} states, the model has {D}")
    if conf is not None and conf.ndim == 3 and int(conf.shape[0]) != P:
        raise C3PropError(f"C3:Error: the confusion rows hold {int(conf.shape[0])} parameter sets, x holds {P}")
    conf_bstride = R * D if (conf is not None and conf.ndim == 3) else 0
    w = _weights_of(readout, labels, R, D)
    V = 1 if w is not None else R
    if w is not None and len(w) != R:
        raise C3PropError(f"C3:Error: {len(w)} label weights for {R} read-out rows")
    lw = call.f64(w)
    rescale, rescale_bstride = None, 0
    if readout.meas_scale is not None or readout.meas_offset is not None:
        # (through numpy: a Python float handed to torch directly would pass through float32)
        as64 = lambda v: call.f64(v if _is_torch(v) else np.asarray(v, dtype=np.float64)).reshape(-1)
        sc = as64(1.0 if readout.meas_scale is None else readout.meas_scale)
        of = as64(0.0 if readout.meas_offset is None else readout.meas_offset)
        n = max(int(sc.shape[0]), int(of.shape[0]))
        if n not in (1, P) or int(sc.shape[0]) not in (1, n) or int(of.shape[0]) not in (1, n):
            raise C3PropError(f"C3:Error: meas_scale / meas_offset hold {int(sc.shape[0])} / {int(of.shape[0])} values, expected 1 or {P}")
        if call.device:
            rescale = call.torch.stack([sc.expand(n), of.expand(n)], -1).contiguous()
        else:
            rescale = np.ascontiguousarray(np.stack([np.broadcast_to(sc, (n,)), np.broadcast_to(of, (n,))], -1))
        rescale_bstride = 2 if (n == P and P > 1) else 0
    shape = (P, S) if w is not None else (P, S, R)
    meas, stds, shots = call.f64(data["results"]), call.f64(data.get("results_std")), call.f64(data["shots"])
    for name, a in (("results", meas), ("results_std", stds), ("shots", shots)):
        if a is not None and tuple(a.shape) != shape:
            raise C3PropError(f"C3:Error: the {name} of the data sets have shape {tuple(a.shape)}, the simulated values {shape}")
    if call.device:
        new = lambda sh, c=False: call.torch.empty(sh, dtype=call.torch.complex128 if c else call.torch.float64, device=call.dev)
    else:
        new = lambda sh, c=False: np.empty(sh, dtype=np.complex128 if c else np.float64)
    sim, goals = new(shape), new((P,))
    raw = new(shape) if rescale is not None else None
    lib = _lib.load()
    if not vjp:
        _lib.check(lib.c3p_readout_goal(_ptr(xs), P, S, M, D, _ptr(conf), conf_bstride, R, _ptr(lw), _ptr(rescale), rescale_bstride, _ptr(meas), _ptr(stds),
                                        _ptr(shots), est, call.flags, _ptr(sim), _ptr(raw), _ptr(goals), call.stream))
        return {"sim": sim, "sim_raw": raw, "goals": goals}
    gw = call.f64(weights if _is_torch(weights) else np.asarray(weights, dtype=np.float64)).reshape(-1)
    if int(gw.shape[0]) != P:
        raise C3PropError(f"C3:Error: {int(gw.shape[0])} goal weights for {P} parameter sets")
    x_bar = new((P, S, M), True)
    conf_bar = new((P, R, D)) if conf is not None else None
    rs_bar = new((P, 2)) if rescale is not None else None
    pop_bar = new((P, S, D)) if want_pop_bar else None
    _lib.check(lib.c3p_readout_goal_vjp(_ptr(xs), P, S, M, D, _ptr(conf), conf_bstride, R, _ptr(lw), _ptr(rescale), rescale_bstride, _ptr(meas), _ptr(stds),
                                        _ptr(shots), est, _ptr(gw), call.flags, _ptr(sim), _ptr(raw), _ptr(goals), _ptr(x_bar), _ptr(conf_bar), _ptr(rs_bar),
                                        _ptr(pop_bar), call.stream))
    rows_bar = None if conf is None else confusion_matrix_vjp([call.f64(r if _is_torch(r) else np.asarray(r, dtype=np.float64)) for r in readout.conf_rows], conf_bar)
    return {"sim": sim, "sim_raw": raw, "goals": goals, "x_bar": x_bar, "conf_bar": conf_bar, "rescale_bar": rs_bar, "pop_bar": pop_bar,
            "grad_conf_rows": rows_bar, "grad_meas_scale": None if rs_bar is None else rs_bar[:, 0], "grad_meas_offset": None if rs_bar is None else rs_bar[:, 1]}


def readout_goal(x, readout: Optional[Readout], data, labels=None, estimator: str = "g_LL_prime", *, dim: Optional[int] = None) -> Dict:
    """Simulated values and goals of P parameter sets from the sequence states `x` [P,S,M] (M = D: kets, M = D^2: density vectors;
    D from `dim`, `readout.dims` or the confusion rows, else M).  `data`: {"results", "results_std", "shots"} [P,S] (with `labels`) or
    [P,S,R], or the list of data sets of `goal_run_batched`.  `labels`: None (every read-out row is a value), row indices, or label
    tuples (`label_weights`).  Returns {"sim" [P,S(,R)], "sim_raw" (before the rescale; None without one), "goals" [P]}."""
    return _run(False, x, readout, data, labels, estimator, None, dim)


def readout_goal_vjp(x, readout: Optional[Readout], data, labels=None, estimator: str = "g_LL_prime", weights=None, *, dim: Optional[int] = None,
                     want_pop_bar: bool = False) -> Dict:
    """`readout_goal` and the cotangents of sum_p weights[p] goals[p]: "x_bar" [P,S,M] as `evaluate_sequences_indexed_vjp` reads it,
    "grad_conf_rows" (list of [P,d_q]), "grad_meas_scale" / "grad_meas_offset" [P] -- always per set, a shared read-out sums over p --
    "conf_bar" [P,R,D], "rescale_bar" [P,2], "pop_bar" [P,S,D] with `want_pop_bar`; None where the read-out has no such part."""
    if weights is None:
        raise C3PropError("C3:Error: readout_goal_vjp needs the goal weights [P]")
    return _run(True, x, readout, data, labels, estimator, weights, dim, want_pop_bar)
