"""Batched callers of the propagator path for model learning and sensitivity sweeps.

The reference evaluates one control-parameter set at a time: `ModelLearning.goal_run` loops over `ipar`
(optimizers/modellearning.py:300-341), each pass setting the gate-set parameters, calling
`exp.compute_propagators()`, `exp.evaluate(sequences)` and `exp.process(...)` (:218-242), then scoring the
simulated populations against the measured ones with `g_LL_prime` (libraries/estimators.py:155-170);
`Sensitivity` drives the same function along a one-dimensional sweep of a model parameter
(optimizers/sensitivity.py:100-124).  Here all P parameter sets (or sweep points) are ONE batch per gate:

  signals[gate] [P,K,N] (+ per-set model operators)  --propagate_batch-->  U[gate] [P,D,D]
  sequences  --c3p_matmul_chain over P x sequences-->  U_seq [P,S,D,D]  -->  |U_seq psi0|^2  -->  sim_vals [P,S]

Everything up to the populations stays in HBM.  By default the likelihood (`g_LL_prime`, a perfect read-out) is evaluated on the host;
with `readout=` (a `readout.Readout`: confusion rows, meas_scale, meas_offset -- an empty one too) or another `estimator=` the read-out
model, the estimator and their reverse mode run on the device (c3p_readout_goal, c3p_readout_goal_vjp) and the result
also holds "sim_vals_no_rescale" and, with the gradient, "grad_conf_rows", "grad_meas_scale", "grad_meas_offset".

Open systems (`col_ops` given): the propagators are Lindblad superoperators [P,D^2,D^2], the sequence states density vectors
and the populations their diagonal; `thermal_initial_state` mirrors InitialiseGround (libraries/tasks.py:46-88).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from . import propagation
from ._lib import C3PropError


KB = 1.380649e-23  # libraries/constants.py
HBAR = 1.054571817e-34


def thermal_initial_state(h0_diag_or_h0, init_temp, lindbladian: bool = True):
    """`InitialiseGround.initialise` (libraries/tasks.py:46-88): the initial state at temperature `init_temp` from the drift
    Hamiltonian (a matrix, of which the diagonal is read, or that diagonal).  A finite temperature gives the Boltzmann weights
    exp(-hbar (E_i - E_0) / (kb T)), normalised, on the diagonal of a density matrix, returned as the density vector [D^2]
    (tf_dm_to_vec) -- this needs the Lindblad path, as in the reference; T = 0 gives the ground state, as vec(|0><0|) with
    `lindbladian`, else as the ket [D].  `thermal_initial_state_vjp` is its derivative: with "grad_psi_init" of
    `goal_run_batched_with_grad` it gives the gradient of a goal with respect to the temperature through rho0."""
    a = np.asarray(h0_diag_or_h0, dtype=np.complex128)
    diag = np.diagonal(a) if a.ndim == 2 else a.reshape(-1)
    dim = len(diag)
    if abs(init_temp) > np.finfo(float).eps:
        freq_diff = diag - diag[0]
        beta = 1 / (init_temp * KB)
        det_bal = np.exp(-HBAR * freq_diff * beta)
        dm = np.diag(det_bal / np.sum(det_bal))
        if not lindbladian:
            raise C3PropError("C3:Error: a thermal initial state needs the Lindblad path (lindbladian=True)")
        return dm.T.reshape(-1)
    state = np.zeros(dim, dtype=np.complex128)
    state[0] = 1.0
    if lindbladian:
        return np.outer(state, state).T.reshape(-1)
    return state


def thermal_initial_state_vjp(h0_diag_or_h0, init_temp, rho0_bar):
    """The exact derivative of `thermal_initial_state` at a finite temperature, in host numpy: from the cotangent `rho0_bar` [D^2] of
    the density vector (d goal = Re sum conj(rho0_bar) d vec(rho0), "grad_psi_init"[p] of `goal_run_batched_with_grad`) returns
    (grad_temp, grad_diag): d goal / d T and d goal / d E_k [D] for the diagonal energies E_k of the drift Hamiltonian (taken real).

    With a_i = hbar (E_i - E_0) / (kb T), w_i = exp(-a_i) / Z and g_i = Re rho0_bar[i (D + 1)] (only the diagonal of rho0 moves):
      d w_i / d T   = w_i (a_i - <a>) / T            grad_temp    = sum_i g_i w_i (a_i - <a>) / T
      d w_i / d E_k = hbar / (kb T) w_i (w_k - d_ik)   grad_diag[k] = hbar / (kb T) w_k (<g> - g_k)
    (<.> the mean under w; the shift by E_0 cancels).  At T = 0 the state is the ground state whatever the energies: both are zero."""
    a = np.asarray(h0_diag_or_h0, dtype=np.complex128)
    diag = (np.diagonal(a) if a.ndim == 2 else a.reshape(-1)).real
    dim = len(diag)
    bar = np.asarray(rho0_bar, dtype=np.complex128).reshape(-1)
    if bar.size != dim * dim:
        raise C3PropError(f"C3:Error: rho0_bar has {bar.size} entries, expected the cotangent of a density vector [{dim * dim}]")
    if not abs(init_temp) > np.finfo(float).eps:
        return 0.0, np.zeros(dim)
    g = bar[:: dim + 1].real
    c = HBAR / (KB * init_temp)
    act = c * (diag - diag[0])
    w = np.exp(-act)
    w = w / np.sum(w)
    grad_temp = float(np.sum(g * w * (act - np.sum(w * act))) / init_temp)
    grad_diag = c * w * (np.sum(g * w) - g)
    return grad_temp, grad_diag


def _per_set_states(psi_init, D: int, P: int, sizes) -> Optional[np.ndarray]:
    """psi_init as [P,n] with n in `sizes` when it holds one state per parameter set, else None (one state for every set: any shape
    with n entries, or what the single-state code refuses -- so P kets [P,D] with P == D are read as ONE density vector [D^2]; pass density vectors [P,D^2] there)."""
    psi = np.asarray(psi_init, dtype=np.complex128)
    if psi.size in sizes:
        return None
    if psi.ndim == 2 and psi.shape[0] == P and psi.shape[1] in sizes:
        return psi
    return None  # (anything else is refused where a single state of that size is)


def _density_vector(psi_init, D: int) -> np.ndarray:
    """vec(rho0) [D^2] from a ket [D] (vec(|psi><psi|), tf_state_to_dm / tf_dm_to_vec) or a density vector [D^2]."""
    psi = np.asarray(psi_init, dtype=np.complex128).reshape(-1)
    if psi.size == D * D:
        return psi
    if psi.size == D:
        return np.outer(psi, psi.conj()).T.reshape(-1)
    raise C3PropError(f"C3:Error: psi_init has {psi.size} entries, expected a ket [{D}] or a density vector [{D * D}]")


def _check_data_sets(data_sets):
    seqs = data_sets[0]["seqs"]
    for d in data_sets:
        if d["seqs"] != seqs:
            raise C3PropError("C3:Error: batched model learning needs the same sequences for every parameter set")
    return seqs


def _open_system_states(h0, hks, gate_signals: Dict, dt: float, col_ops, P: int, seqs, psi_init, fr_phase, device):
    """Superoperators S[gate] [P,D^2,D^2] by `propagate_batch(..., lindbladian=True)`, the sequence states
    x = S_seq vec(rho0) [P,S,D^2] on the indexed path and their populations Re diag(vec_to_dm(x)) [P,S,D]
    (experiment.py:619-622).  Returns (per-gate call arguments, S, vec(rho0), x, pops)."""
    from . import sequences as sq

    D = int(np.shape(h0)[-1])
    sets = _per_set_states(psi_init.detach().cpu().numpy() if propagation._is_torch(psi_init) else psi_init, D, P, (D, D * D))
    rho0 = _density_vector(psi_init, D) if sets is None else np.stack([_density_vector(s, D) for s in sets])  # [D^2] or [P,D^2]
    for gate, sig in gate_signals.items():
        if int(sig.shape[0]) != P:
            raise C3PropError(f"C3:Error: gate {gate!r} has {int(sig.shape[0])} parameter sets, but there are {P} data sets")
    args, Us = {}, {}
    if device is not None:
        import torch

        to = lambda v, dt_: v.to(device) if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=dt_), device=device)
        rho0 = torch.as_tensor(rho0, device=device)
    else:
        to = lambda v, dt_: v
    col = to(col_ops, np.complex128)
    for gate, sig in gate_signals.items():
        ph = None if fr_phase is None else fr_phase.get(gate)
        args[gate] = (to(h0, np.complex128), to(hks, np.complex128), to(sig, np.float64), None if ph is None else to(ph, np.float64))
        a = args[gate]
        Us[gate] = propagation.propagate_batch(a[0], a[1], a[2], dt, col_ops=col, lindbladian=True, fr_phase=a[3])["U"]
    x = sq.evaluate_sequences_indexed(Us, seqs, "state", rho0, superop=True)  # [P,S,D^2]
    pops = x[..., :: D + 1].real  # the diagonal of vec_to_dm(x): entries n D + n
    return args, col, Us, rho0, x, pops


def g_LL_prime(exp_values, sim_values, exp_stds, shots):
    """estimators.py:155-157: mean of ((m - s)^2 / (s (1 - s) / shots) - 1) / 2."""
    m = np.asarray(exp_values, dtype=np.float64)
    s = np.asarray(sim_values, dtype=np.float64)
    var = s * (1.0 - s) / np.asarray(shots, dtype=np.float64)
    return np.mean(((m - s) ** 2 / var - 1.0) / 2.0)


def g_LL_prime_combined(gs, weights):
    """estimators.py:168-170."""
    K = np.sum(weights)
    return np.sum(np.array(weights) * np.asarray(gs)) / K


def g_LL_prime_grad(exp_values, sim_values, exp_stds, shots):
    """d g_LL_prime / d sim_values, analytically: with r = m - s and v = s (1 - s),
    d/ds [r^2 shots / v] = -shots (2 r / v + r^2 (1 - 2 s) / v^2), halved and divided by the number of values."""
    m = np.asarray(exp_values, dtype=np.float64)
    s = np.asarray(sim_values, dtype=np.float64)
    sh = np.asarray(shots, dtype=np.float64)
    r, v = m - s, s * (1.0 - s)
    return -sh * (2.0 * r / v + r**2 * (1.0 - 2.0 * s) / v**2) / (2.0 * s.size)


def dv_g_LL_prime(gs, dv_gs, weights):
    """estimators.py:160-165: the gradient of `g_LL_prime_combined`, sum_i w_i dv_gs[i] / sum_i w_i."""
    K = np.sum(weights)
    g = 0
    for ii in range(len(weights)):
        g = g + weights[ii] * dv_gs[ii]
    return g / K


def propagate_parameter_sets(h0, hks, gate_signals: Dict[str, np.ndarray], dt: float, *, fr_phase: Optional[Dict] = None, device=None) -> Dict:
    """U[gate] [P,D,D] for P parameter sets: one `propagate_batch` call per gate (the reference recomputes every
    gate inside the `ipar` loop, modellearning.py:236-237).  `h0` / `hks` may carry a leading P axis (a model
    parameter differs between the sets, as in a sensitivity sweep); `gate_signals[gate]` is [P,K,N]."""
    out = {}
    P = None
    for gate, sig in gate_signals.items():
        if P is None:
            P = int(sig.shape[0])
        if int(sig.shape[0]) != P:
            raise C3PropError(f"C3:Error: gate {gate!r} has {int(sig.shape[0])} parameter sets, expected {P}")
        ph = None if fr_phase is None else fr_phase.get(gate)
        if device is not None:
            import torch

            to = lambda x, dt_: x.to(device) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=dt_), device=device)
            out[gate] = propagation.propagate_batch(to(h0, np.complex128), to(hks, np.complex128), to(sig, np.float64), dt, fr_phase=None if ph is None else to(ph, np.float64))["U"]
        else:
            out[gate] = propagation.propagate_batch(h0, hks, sig, dt, fr_phase=ph)["U"]
    return out


def evaluate_sequences_batch(gate_Us: Dict, sequences: Sequence[Sequence[str]]):
    """U_seq [P,S,D,D]: total propagator of every sequence for every parameter set, `... U2 U1 U0`
    (propagation.py:588-627).  Sequences of equal length are multiplied in one `c3p_matmul_chain` launch over
    P x (sequences of that length) chains; an empty sequence is the identity."""
    first = next(iter(gate_Us.values()))
    is_t = propagation._is_torch(first)
    P, D = int(first.shape[0]), int(first.shape[-1])
    S = len(sequences)
    if is_t:
        import torch

        out = torch.empty((P, S, D, D), dtype=first.dtype, device=first.device)
        eye = torch.eye(D, dtype=first.dtype, device=first.device)
        stack = torch.stack
    else:
        out = np.empty((P, S, D, D), dtype=np.complex128)
        eye = np.eye(D, dtype=np.complex128)
        stack = np.stack
    by_len: Dict[int, List[int]] = {}
    for si, seq in enumerate(sequences):
        for g in seq:
            if g not in gate_Us:
                raise C3PropError(f"C3:Error: sequence uses gate {g!r} without a propagator")
        by_len.setdefault(len(seq), []).append(si)
    for L, idx in by_len.items():
        if L == 0:
            for si in idx:
                out[:, si] = eye
            continue
        if L == 1:
            for si in idx:
                out[:, si] = gate_Us[sequences[si][0]]
            continue
        # [P, n, L, D, D] -> P n chains of L factors, first gate applied first
        M = stack([stack([gate_Us[g] for g in sequences[si]], 1) for si in idx], 1)
        prod = propagation.tf_matmul_left(M.reshape((P * len(idx), L, D, D)))
        prod = prod.reshape((P, len(idx), D, D))
        for j, si in enumerate(idx):
            out[:, si] = prod[:, j]
    return out


def populations_batch(U_seq, psi_init):
    """|U_seq psi0|^2 [P,S,D]  (experiment.py:291-301,603-624, unitary case); psi_init one ket, or one per set [P,D]."""
    P, D = int(U_seq.shape[0]), int(U_seq.shape[-1])
    sets = _per_set_states(psi_init, D, P, (D,))
    if propagation._is_torch(U_seq):
        import torch

        if sets is not None:
            amp = torch.einsum("psij,pj->psi", U_seq, torch.as_tensor(sets, dtype=U_seq.dtype, device=U_seq.device))
            return amp.real**2 + amp.imag**2
        psi = torch.as_tensor(np.asarray(psi_init).reshape(-1), dtype=U_seq.dtype, device=U_seq.device)
        amp = U_seq @ psi
        return amp.real**2 + amp.imag**2
    if sets is not None:
        return np.abs(np.einsum("psij,pj->psi", U_seq, sets)) ** 2
    amp = U_seq @ np.asarray(psi_init, dtype=np.complex128).reshape(-1)
    return np.abs(amp) ** 2


def process_batch(pops, label_indices: Optional[Sequence[int]] = None):
    """`Experiment.process` without a confusion matrix or rescaling (experiment.py:355-400): the summed
    population of the selected state labels, [P,S]; all populations [P,S,D] when no labels are given."""
    if label_indices is None:
        return pops
    idx = list(label_indices)
    return pops[..., idx].sum(-1)


def _legacy_epilogue(readout, estimator) -> bool:
    """True for the host epilogue (perfect read-out, g_LL_prime in numpy); a `Readout` -- an empty one too -- or another estimator
    takes the device epilogue of `readout.readout_goal` / `readout_goal_vjp`."""
    return readout is None and estimator == "g_LL_prime"


def _host_or_none(a):
    if a is None:
        return None
    return a.cpu().numpy() if propagation._is_torch(a) else np.asarray(a)


def _readout_forward(x, D: int, data, readout, estimator, label_indices, P: int, n_seqs: int) -> Dict:
    """Goals of the device epilogue from the sequence states x [P,S,M]; only the results leave the device."""
    from . import readout as ro

    r = ro.readout_goal(x, readout, data, label_indices, estimator, dim=D)
    goals = _host_or_none(r["goals"])
    return {"goal": g_LL_prime_combined(goals, [n_seqs] * P), "goals": goals, "sim_vals": _host_or_none(r["sim"]),
            "sim_vals_no_rescale": _host_or_none(r["sim_raw"])}


def _readout_backward(x, D: int, data, readout, estimator, label_indices, P: int, n_seqs: int):
    """(result entries, x_bar) of the device epilogue: c3p_readout_goal_vjp with the weights w_p / sum w of `dv_g_LL_prime`.
    The goals and simulated values stay where x is; `_readout_results` copies them out once the reverse sweep is enqueued."""
    from . import readout as ro

    weights = np.full(P, float(n_seqs)) / (float(n_seqs) * P)
    if propagation._is_torch(x):
        import torch

        weights = torch.as_tensor(weights, device=x.device)
    r = ro.readout_goal_vjp(x, readout, data, label_indices, estimator, weights, dim=D)
    return r, r["x_bar"]


def _readout_results(r, P: int, n_seqs: int) -> Dict:
    goals = _host_or_none(r["goals"])
    return {"goal": g_LL_prime_combined(goals, [n_seqs] * P), "goals": goals, "sim_vals": _host_or_none(r["sim"]),
            "sim_vals_no_rescale": _host_or_none(r["sim_raw"]), "grad_conf_rows": r["grad_conf_rows"], "grad_meas_scale": r["grad_meas_scale"],
            "grad_meas_offset": r["grad_meas_offset"]}


def goal_run_batched(h0, hks, gate_signals: Dict, dt: float, data_sets: Sequence[Dict], psi_init, label_indices, *, fr_phase: Optional[Dict] = None, device=None, col_ops=None,
                     readout=None, estimator: str = "g_LL_prime") -> Dict:
    """`ModelLearning.goal_run` (modellearning.py:285-360) with the `ipar` loop as one batch.

    `data_sets[p]` = {"seqs": [...], "results": [...], "results_std": [...], "shots": [...]} for parameter set
    p, whose pulses are row p of every `gate_signals[gate]`.  All sets must use the same sequence list (the
    reference's `seqs_per_point`).  Returns {"goal", "goals" [P], "sim_vals" [P,S]}; the per-set goal is
    `g_LL_prime`, combined with the sequence counts as weights.

    With `col_ops` [C,D,D] the system is open: Lindblad superoperators, `psi_init` a ket [D] (taken as |psi><psi|) or a density
    vector [D^2] (`thermal_initial_state`), `fr_phase[gate]` [P,D^2], populations Re diag(vec_to_dm(S_seq vec(rho0))).

    Per parameter set: `col_ops` [P,C,D,D] gives set p its own collapse operators (T1, T2*, bath temperature differ between the
    sets), `psi_init` [P,D] or [P,D^2] (closed systems: [P,D]) its own initial state.  One state is recognised by its size, so P kets
    with P == D are read as one density vector: pass [P,D^2] there.

    `readout` (a `readout.Readout`): the confusion matrix and the rescale of `Experiment.process` between the populations and the
    estimator, shared or per set; `label_indices` then index the rows of the confusion matrix (`comp_state_labels`) when it has one.
    `estimator`: a name of `readout.ESTIMATORS`.  With either, the sequence states go through c3p_readout_goal on the device and the
    result also holds "sim_vals_no_rescale" (None without a rescale); with both at their defaults nothing changes.
    """
    P = len(data_sets)
    if not _legacy_epilogue(readout, estimator):
        return _goal_run_readout(h0, hks, gate_signals, dt, data_sets, psi_init, label_indices, fr_phase, device, col_ops, readout, estimator)
    if col_ops is not None:
        seqs = _check_data_sets(data_sets)
        sim = process_batch(_open_system_states(h0, hks, gate_signals, dt, col_ops, P, seqs, psi_init, fr_phase, device)[-1], label_indices)
        sim = sim.cpu().numpy() if propagation._is_torch(sim) else np.asarray(sim)
        goals = np.array([g_LL_prime(d["results"], sim[p], d["results_std"], d["shots"]) for p, d in enumerate(data_sets)])
        return {"goal": g_LL_prime_combined(goals, [len(seqs)] * P), "goals": goals, "sim_vals": sim}
    seqs = data_sets[0]["seqs"]
    for d in data_sets:
        if d["seqs"] != seqs:
            raise C3PropError("C3:Error: batched model learning needs the same sequences for every parameter set")
    Us = propagate_parameter_sets(h0, hks, gate_signals, dt, fr_phase=fr_phase, device=device)
    if int(next(iter(Us.values())).shape[0]) != P:
        raise C3PropError("C3:Error: number of data sets and parameter sets differ")
    sim = process_batch(populations_batch(evaluate_sequences_batch(Us, seqs), psi_init), label_indices)
    sim = sim.cpu().numpy() if propagation._is_torch(sim) else np.asarray(sim)
    goals = np.array([g_LL_prime(d["results"], sim[p], d["results_std"], d["shots"]) for p, d in enumerate(data_sets)])
    weights = [len(seqs)] * P
    return {"goal": g_LL_prime_combined(goals, weights), "goals": goals, "sim_vals": sim}


def _closed_system_states(h0, hks, gate_signals, dt, P: int, seqs, psi_init, fr_phase, device):
    """(U[gate], psi0, x [P,S,D]): the sequence states of a closed system on the indexed path."""
    from . import sequences as sq

    Us = propagate_parameter_sets(h0, hks, gate_signals, dt, fr_phase=fr_phase, device=device)
    first = next(iter(Us.values()))
    if int(first.shape[0]) != P:
        raise C3PropError("C3:Error: number of data sets and parameter sets differ")
    D = int(first.shape[-1])
    sets = _per_set_states(psi_init, D, P, (D,))
    psi = np.asarray(psi_init, dtype=np.complex128).reshape(-1) if sets is None else sets
    if device is not None:
        import torch

        psi = torch.as_tensor(psi, device=device)
    return Us, psi, sq.evaluate_sequences_indexed(Us, seqs, "state", psi)


def _goal_run_readout(h0, hks, gate_signals, dt, data_sets, psi_init, label_indices, fr_phase, device, col_ops, readout, estimator) -> Dict:
    """`goal_run_batched` with the read-out model: sequence states on the indexed path, then c3p_readout_goal.  `label_indices`
    index the rows of the confusion matrix (`comp_state_labels`) when `readout.conf_rows` is given, the states otherwise."""
    from . import readout as ro

    P = len(data_sets)
    seqs = _check_data_sets(data_sets)
    data = ro.stack_data(data_sets, device)  # (on its way before the first launch)
    if col_ops is not None:
        x = _open_system_states(h0, hks, gate_signals, dt, col_ops, P, seqs, psi_init, fr_phase, device)[4]
        D = int(np.shape(h0)[-1])
    else:
        x = _closed_system_states(h0, hks, gate_signals, dt, P, seqs, psi_init, fr_phase, device)[2]
        D = int(x.shape[-1])
    return _readout_forward(x, D, data, readout, estimator, label_indices, P, len(seqs))


def goal_run_batched_with_grad(h0, hks, gate_signals: Dict, dt: float, data_sets: Sequence[Dict], psi_init, label_indices, *, fr_phase: Optional[Dict] = None, device=None, col_ops=None,
                               readout=None, estimator: str = "g_LL_prime") -> Dict:
    """`goal_run_batched` and the gradient of its combined goal -- what `ModelLearning.goal_run_with_grad` tapes
    (modellearning.py:362-440): model operators -> propagators -> sequence states -> label populations -> g_LL_prime,
    the per-set gradients combined by `dv_g_LL_prime`.

    1. U[gate] [P,D,D] by `propagate_parameter_sets`;
    2. the sequence states U_seq psi0 [P,S,D] on the indexed path (c3p_seq_chain, state mode), and from the cotangent
       xbar = 2 simbar x on the label rows the propagator cotangents by ONE c3p_seq_chain_vjp call (with
       `label_indices` None every population is a simulated value, sim_vals [P,S,D] and results [S,D] per set);
    3. per gate, `propagate_batch_vjp(..., want_model_grads=True)`;
    4. the operator cotangents summed over the gates.

    Returns {"goal", "goals" [P], "sim_vals" [P,S]} as `goal_run_batched` and
      "grad_h0" [P,D,D], "grad_hks" [P,K,D,D]: row p is d goal / d h0[p] (d goal = Re sum conj(grad) dh) of the COMBINED
          goal, the weights w_p / sum w folded in (a model shared by every set: sum over p, or `model_param_grads`);
      "grad_signals" {gate: [P,K,N]}; "grad_fr_phase" {gate: [P,D]} or None.
    With `device` everything up to the populations stays there (gradients are tensors on it).

    With `col_ops` [C,D,D] the system is open (D <= 9), as in `goal_run_batched`: the populations are LINEAR in the sequence
    state x = S_seq vec(rho0), so x_bar is pop_bar on its diagonal entries n D + n; step 3 is
    `propagate_batch_lindblad_vjp(..., want_model_grads=True)`, and the result also holds "grad_col_ops" [P,C,D,D], the cotangent
    of the collapse operators (through which T1, T2* and the temperature of the bath act), `grad_fr_phase[gate]` is [P,D^2].
    `col_ops` [P,C,D,D]: one set of collapse operators per parameter set; grad_col_ops[p] is then the cotangent of col_ops[p].
    "grad_psi_init" is the cotangent of the initial state per set (also for a shared one: sum over p then): [P,D^2], that of
    vec(rho0), for open systems (through `thermal_initial_state_vjp` the gradient of the temperature through rho0), [P,D], that of
    the ket, for closed ones; `psi_init` may be one state or one per set, as in `goal_run_batched`.
    D = 7, 8, 9 (two coupled qutrits) take the Hermitian-basis sweep (`hermitian_basis=True`): h0 / hks must be Hermitian, and
    "grad_h0" / "grad_hks" are then Hermitian matrices, the Hermitian part of the general cotangent -- exact in
    `model_param_grads` for every Hermitian dh0 / dhks, which is what a model parameter moves.

    `readout` / `estimator` as in `goal_run_batched`: the epilogue is then ONE c3p_readout_goal_vjp call between the two sequence
    calls, nothing touches the host in between, and the result also holds "grad_conf_rows" (a list of [P,d_q]), "grad_meas_scale" and
    "grad_meas_offset" ([P]; None where the read-out has no such parameter; a shared read-out: sum over p) and "sim_vals_no_rescale".
    """
    P = len(data_sets)
    if col_ops is not None:
        return _goal_run_open_with_grad(h0, hks, gate_signals, dt, data_sets, psi_init, label_indices, fr_phase, device, col_ops, readout, estimator)
    seqs = data_sets[0]["seqs"]
    for d in data_sets:
        if d["seqs"] != seqs:
            raise C3PropError("C3:Error: batched model learning needs the same sequences for every parameter set")
    from . import sequences as sq

    legacy = _legacy_epilogue(readout, estimator)
    if not legacy:
        from . import readout as ro

        ro_data = ro.stack_data(data_sets, device)  # (on its way before the first launch)
    if device is not None:
        import torch
    Us, psi, x = _closed_system_states(h0, hks, gate_signals, dt, P, seqs, psi_init, fr_phase, device)  # x [P,S,D]
    D = int(x.shape[-1])
    ro_res = None
    if legacy:
        pops = x.real**2 + x.imag**2
        sim = process_batch(pops, label_indices)
        sim_h = sim.cpu().numpy() if propagation._is_torch(sim) else np.asarray(sim)
        goals = np.array([g_LL_prime(d["results"], sim_h[p], d["results_std"], d["shots"]) for p, d in enumerate(data_sets)])
        weights = [len(seqs)] * P
        dgs = [g_LL_prime_grad(d["results"], sim_h[p], d["results_std"], d["shots"]) for p, d in enumerate(data_sets)]
        if any(np.shape(g) != sim_h.shape[1:] for g in dgs):
            raise C3PropError(f"C3:Error: the results of a data set do not have the shape of its simulated values {sim_h.shape[1:]}")
        # combined goal: d goal / d sim[p] = w_p / sum w * d g_p / d sim[p]
        sim_bar = np.stack([w / np.sum(weights) * g for w, g in zip(weights, dgs)])
        # sim = sum over the label rows of |x|^2 ([P,S]), or every population |x|^2 itself ([P,S,D], no labels):
        # x_bar = 2 sim_bar x on the rows that enter
        if label_indices is None:
            pop_bar = sim_bar
        else:
            rows = np.zeros(D)
            np.add.at(rows, list(label_indices), 1.0)  # a label listed twice counts twice, as in process_batch
            pop_bar = sim_bar[..., None] * rows
        x_bar = 2.0 * (torch.as_tensor(pop_bar, device=device) if device is not None else pop_bar) * x
    else:  # confusion, selection, rescale, estimator and their reverse mode in one call on the device
        ro_res, x_bar = _readout_backward(x, D, ro_data, readout, estimator, label_indices, P, len(seqs))
    U_bar, psi_bar = sq.evaluate_sequences_indexed_vjp(Us, seqs, "state", x_bar, psi, want_psi0_bar=True)
    grad_h0 = grad_hks = None
    grad_signals, grad_ph = {}, ({} if fr_phase is not None else None)
    for gate, sig in gate_signals.items():
        ph = None if fr_phase is None else fr_phase.get(gate)
        if device is not None:
            to = lambda v, dt_: v.to(device) if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=dt_), device=device)
            args = (to(h0, np.complex128), to(hks, np.complex128), to(sig, np.float64))
            ph = None if ph is None else to(ph, np.float64)
        else:
            args = (h0, hks, sig)
        g_sig, g0, gk = propagation.propagate_batch_vjp(*args, dt, U_bar[gate], fr_phase=ph, want_model_grads=True)
        grad_signals[gate] = g_sig
        grad_h0 = g0 if grad_h0 is None else grad_h0 + g0
        grad_hks = gk if grad_hks is None else grad_hks + gk
        if grad_ph is not None:
            Ug, Ub = Us[gate], U_bar[gate]
            # U = diag(e^{i phi}) P  =>  d loss / d phi_i = -Im sum_j conj(Ubar_ij) U_ij (optimal_control.goal_run_with_grad)
            grad_ph[gate] = None if ph is None else (-(Ub.conj() * Ug).sum(-1).imag)
    head = {"goal": g_LL_prime_combined(goals, weights), "goals": goals, "sim_vals": sim_h} if legacy else _readout_results(ro_res, P, len(seqs))
    return {**head, "grad_h0": grad_h0, "grad_hks": grad_hks, "grad_signals": grad_signals, "grad_fr_phase": grad_ph, "grad_psi_init": psi_bar}


def _goal_run_open_with_grad(h0, hks, gate_signals, dt, data_sets, psi_init, label_indices, fr_phase, device, col_ops, readout=None,
                             estimator: str = "g_LL_prime") -> Dict:
    """The open-system branch of `goal_run_batched_with_grad`."""
    from . import sequences as sq

    P = len(data_sets)
    seqs = _check_data_sets(data_sets)
    legacy = _legacy_epilogue(readout, estimator)
    if not legacy:
        from . import readout as ro

        ro_data = ro.stack_data(data_sets, device)  # (on its way before the first launch)
    args, col, Us, rho0, x, pops = _open_system_states(h0, hks, gate_signals, dt, col_ops, P, seqs, psi_init, fr_phase, device)
    D = int(pops.shape[-1])
    ro_res = None
    if legacy:
        sim = process_batch(pops, label_indices)
        sim_h = sim.cpu().numpy() if propagation._is_torch(sim) else np.asarray(sim)
        goals = np.array([g_LL_prime(d["results"], sim_h[p], d["results_std"], d["shots"]) for p, d in enumerate(data_sets)])
        weights = [len(seqs)] * P
        dgs = [g_LL_prime_grad(d["results"], sim_h[p], d["results_std"], d["shots"]) for p, d in enumerate(data_sets)]
        if any(np.shape(g) != sim_h.shape[1:] for g in dgs):
            raise C3PropError(f"C3:Error: the results of a data set do not have the shape of its simulated values {sim_h.shape[1:]}")
        sim_bar = np.stack([w / np.sum(weights) * g for w, g in zip(weights, dgs)])
        if label_indices is None:
            pop_bar = sim_bar
        else:
            rows = np.zeros(D)
            np.add.at(rows, list(label_indices), 1.0)  # a label listed twice counts twice, as in process_batch
            pop_bar = sim_bar[..., None] * rows
        # pops = Re x[n D + n]: x_bar is pop_bar on those entries (d loss = Re sum conj(x_bar) dx), zero elsewhere
        x_bar = np.zeros(pop_bar.shape[:-1] + (D * D,), dtype=np.complex128)
        x_bar[..., :: D + 1] = pop_bar
        if device is not None:
            import torch

            x_bar = torch.as_tensor(x_bar, device=device)
    else:
        ro_res, x_bar = _readout_backward(x, D, ro_data, readout, estimator, label_indices, P, len(seqs))
    U_bar, rho0_bar = sq.evaluate_sequences_indexed_vjp(Us, seqs, "state", x_bar, rho0, superop=True, want_psi0_bar=True)
    grad_h0 = grad_hks = grad_col = None
    grad_signals, grad_ph = {}, ({} if fr_phase is not None else None)
    for gate in gate_signals:
        a = args[gate]
        g_sig, g0, gk, gc = propagation.propagate_batch_lindblad_vjp(a[0], a[1], a[2], dt, col, U_bar[gate], fr_phase=a[3], want_model_grads=True,
                                                                     hermitian_basis=D >= 7)
        grad_signals[gate] = g_sig
        grad_h0 = g0 if grad_h0 is None else grad_h0 + g0
        grad_hks = gk if grad_hks is None else grad_hks + gk
        grad_col = gc if grad_col is None else grad_col + gc
        if grad_ph is not None:
            grad_ph[gate] = None if a[3] is None else (-(U_bar[gate].conj() * Us[gate]).sum(-1).imag)
    head = {"goal": g_LL_prime_combined(goals, weights), "goals": goals, "sim_vals": sim_h} if legacy else _readout_results(ro_res, P, len(seqs))
    return {**head, "grad_h0": grad_h0, "grad_hks": grad_hks, "grad_col_ops": grad_col, "grad_signals": grad_signals, "grad_fr_phase": grad_ph,
            "grad_psi_init": rho0_bar}


def model_param_grads(grad_h0, grad_hks, dh0, dhks=None, grad_col_ops=None, dcol_ops=None):
    """Gradient w.r.t. T model parameters theta from the operator cotangents of `goal_run_batched_with_grad`:
    Re sum conj(grad_h0) dh0/dtheta (+ Re sum conj(grad_hks) dhks/dtheta).  `dh0` [T,D,D] (a model shared by the P sets:
    result [T], summed over the sets) or [P,T,D,D] (per set: result [P,T]); `dhks` [T,K,D,D] or [P,T,K,D,D], or None.
    Open systems: `grad_col_ops` [P,C,D,D] with `dcol_ops` [T,C,D,D] or [P,T,C,D,D] adds Re sum conj(grad_col_ops) dcol_ops/dtheta.
    Open systems at D = 7, 8, 9 return Hermitian grad_h0 / grad_hks (the Hermitian part of the general cotangent): the result is exact
    for Hermitian `dh0` / `dhks`; the anti-Hermitian part of a direction does not enter."""
    tonp = lambda a: a.detach().cpu().numpy() if propagation._is_torch(a) else np.asarray(a)
    g0, gk = tonp(grad_h0), tonp(grad_hks)
    dh0 = np.asarray(tonp(dh0), dtype=np.complex128)
    per_set = dh0.ndim == 4
    out = np.einsum("pij,ptij->pt" if per_set else "pij,tij->pt", g0.conj(), dh0).real
    if dhks is not None:
        dk = np.asarray(tonp(dhks), dtype=np.complex128)
        out = out + np.einsum("pkij,ptkij->pt" if dk.ndim == 5 else "pkij,tkij->pt", gk.conj(), dk).real
    if (grad_col_ops is None) != (dcol_ops is None):
        raise C3PropError("C3:Error: grad_col_ops and dcol_ops go together")
    if dcol_ops is not None:
        dc = np.asarray(tonp(dcol_ops), dtype=np.complex128)
        out = out + np.einsum("pcij,ptcij->pt" if dc.ndim == 5 else "pcij,tcij->pt", tonp(grad_col_ops).conj(), dc).real
    return out if per_set else out.sum(axis=0)


def sensitivity_sweep(h0_of, hks_of, sweep_values: Sequence[float], gate_signals_one: Dict, dt: float, data_set: Dict, psi_init, label_indices, *, device=None, col_ops_of=None,
                      psi_init_of=None, readout=None, estimator: str = "g_LL_prime") -> Dict:
    """`Sensitivity.sensitivity` for one swept model parameter (sensitivity.py:100-124): the goal at every sweep
    point, all points in one batch.  `h0_of(v)` / `hks_of(v)` build the (dressed) operators at value v -- the
    model update the reference performs per point (modellearning.py:227-232); the pulses are shared.

    `col_ops_of(v)` [C,D,D]: the sweep runs the open-system branch with the collapse operators of every point (a sweep over T1, T2* or
    the bath temperature).  `psi_init_of(v)`: the initial state of every point (a ket [D] or a density vector [D^2], e.g.
    `thermal_initial_state` at the swept temperature) instead of `psi_init`."""
    vals = list(sweep_values)
    P = len(vals)
    h0 = np.stack([np.asarray(h0_of(v), dtype=np.complex128) for v in vals])
    hks = np.stack([np.asarray(hks_of(v), dtype=np.complex128) for v in vals])
    sig = {g: np.broadcast_to(np.asarray(s, dtype=np.float64)[None], (P,) + tuple(np.shape(s))).copy() for g, s in gate_signals_one.items()}
    col = None if col_ops_of is None else np.stack([np.asarray(col_ops_of(v), dtype=np.complex128) for v in vals])  # [P,C,D,D]
    if psi_init_of is not None:
        psi_init = np.stack([np.asarray(psi_init_of(v), dtype=np.complex128).reshape(-1) for v in vals])  # [P,D] or [P,D^2]
        if P == 1:  # (one point: a single state, which is what a size of D or D^2 is read as)
            psi_init = psi_init[0]
    r = goal_run_batched(h0, hks, sig, dt, [data_set] * P, psi_init, label_indices, device=device, col_ops=col, readout=readout, estimator=estimator)
    return {"values": np.asarray(vals), "goals": r["goals"], "sim_vals": r["sim_vals"]}


def _bare_operator_list(hks_bare, col_ops_bare, P: int, device):
    """Control Hamiltonians [K,D,D] / [P,K,D,D] and collapse operators (None, [C,D,D] or [P,C,D,D]) as the one list `dress_batch`
    takes: (ops, K, hks_shared, col_shared); ops is [K+C,D,D] when both are shared, else [P,K+C,D,D]."""
    if device is not None:
        import torch

        conv = lambda v: v.to(device=device, dtype=torch.complex128) if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.complex128), device=device)
        cat, expand = torch.cat, (lambda v: v[None].expand((P,) + tuple(v.shape)))
    else:
        conv = lambda v: np.asarray(v.detach().cpu().numpy() if propagation._is_torch(v) else v, dtype=np.complex128)
        cat, expand = np.concatenate, (lambda v: np.broadcast_to(v[None], (P,) + tuple(v.shape)))
    hk = conv(hks_bare)
    if hk.ndim not in (3, 4):
        raise C3PropError(f"C3:Error: hks_bare has shape {tuple(hk.shape)}; expected [K,D,D] or [P,K,D,D]")
    K = int(hk.shape[-3])
    if col_ops_bare is None:
        return hk, K, hk.ndim == 3, True
    col = conv(col_ops_bare)
    if col.ndim not in (3, 4):
        raise C3PropError(f"C3:Error: col_ops_bare has shape {tuple(col.shape)}; expected [C,D,D] or [P,C,D,D]")
    hk_shared, col_shared = hk.ndim == 3, col.ndim == 3
    if hk_shared != col_shared:  # one list per set as soon as either differs between the sets
        hk = expand(hk) if hk_shared else hk
        col = expand(col) if col_shared else col
    return cat([hk, col], -3), K, hk_shared, col_shared


def goal_run_dressed_with_grad(H_bare, hks_bare, gate_signals: Dict, dt: float, data_sets: Sequence[Dict], psi_init, label_indices, *, col_ops_bare=None,
                               fr_phase: Optional[Dict] = None, device=None, readout=None, estimator: str = "g_LL_prime") -> Dict:
    """`goal_run_batched_with_grad` from the BARE model: the P drift Hamiltonians `H_bare` [P,D,D] (or one, [D,D]) are dressed on the
    device (`dressing.dress_batch`: Model.update_dressed for every set in one launch), with them the control Hamiltonians `hks_bare`
    [K,D,D] / [P,K,D,D] and, for an open system, the collapse operators `col_ops_bare` [C,D,D] / [P,C,D,D]; the goal and its
    gradient are those of `goal_run_batched_with_grad` on the dressed operators, and its cotangents grad_h0, grad_hks and grad_col_ops
    are pushed back through `dressing.dress_batch_vjp`.  With `device` nothing leaves the GPU in between.  2 <= D <= 40; `psi_init`,
    `fr_phase` and the labels refer to the dressed frame, as in `goal_run_batched_with_grad`.

    Returns that function's dict plus
      "grad_H_bare" [P,D,D]   d goal / d H_bare[p] (Hermitian; a model shared by the sets: sum over p, or `model_param_grads`);
      "grad_hks_bare", "grad_col_ops_bare"   cotangents of the bare operators: per set for per-set operators, summed over the sets
                              for shared ones ("grad_col_ops_bare" None for a closed system);
      "eigenframe" [P,D], "status" int32 [P] (dressing.RECOVERED / DEGENERATE bits of the two dressing calls).

    The bare Hamiltonian of the chip models is linear in the parameters, H = sum_t theta_t G_t with constant matrices G [T,D,D]
    (`workloads.bare_drift`), so the exact parameter gradient needs no derivative of the eigendecomposition:

        r = goal_run_dressed_with_grad(H_bare, hks_bare, signals, dt, data_sets, psi0, labels)
        grad_theta = model_param_grads(r["grad_H_bare"], r["grad_hks_bare"], dh0=G)
    """
    from . import dressing

    P = len(data_sets)
    if device is not None:
        import torch

        H = H_bare.to(device=device, dtype=torch.complex128) if torch.is_tensor(H_bare) else torch.as_tensor(np.asarray(H_bare, dtype=np.complex128), device=device)
        H = H[None].expand(P, -1, -1).contiguous() if H.ndim == 2 else H
    else:
        H = np.asarray(H_bare.detach().cpu().numpy() if propagation._is_torch(H_bare) else H_bare, dtype=np.complex128)
        H = np.broadcast_to(H[None], (P,) + H.shape).copy() if H.ndim == 2 else H
    if H.ndim != 3 or int(H.shape[0]) != P:
        raise C3PropError(f"C3:Error: H_bare has shape {tuple(H.shape)}, but there are {P} data sets")
    ops, K, hk_shared, col_shared = _bare_operator_list(hks_bare, col_ops_bare, P, device)
    d = dressing.dress_batch(H, ops)
    hks = d["ops"][:, :K]
    col = None if col_ops_bare is None else d["ops"][:, K:]
    r = goal_run_batched_with_grad(d["h0"], hks, gate_signals, dt, data_sets, psi_init, label_indices, fr_phase=fr_phase, device=device, col_ops=col, readout=readout,
                                   estimator=estimator)
    g_ops = r["grad_hks"]
    if col is not None:
        g_ops = (torch.cat if device is not None else np.concatenate)([g_ops, r["grad_col_ops"]], 1)
    v = dressing.dress_batch_vjp(d["transform"], d["eigenframe"], ops, grad_h0=r["grad_h0"], grad_ops=g_ops)
    gb = v["grad_ops"]
    per_set = gb.ndim == 4
    g_hk = gb[..., :K, :, :]
    g_col = None if col is None else gb[..., K:, :, :]
    if per_set and hk_shared:
        g_hk = g_hk.sum(0)
    if per_set and col is not None and col_shared:
        g_col = g_col.sum(0)
    out = dict(r)
    st = np.asarray(dressing._host(d["status"])) | np.asarray(dressing._host(v["status"]))
    out.update({"grad_H_bare": v["grad_H"], "grad_hks_bare": g_hk, "grad_col_ops_bare": g_col, "eigenframe": d["eigenframe"], "status": st})
    return out


def sensitivity_sweep_dressed(H_bare_of, hks_bare, sweep_values: Sequence[float], gate_signals_one: Dict, dt: float, data_set: Dict, psi_init, label_indices, *,
                              device=None, col_ops_bare_of=None, psi_init_of=None, readout=None, estimator: str = "g_LL_prime") -> Dict:
    """`sensitivity_sweep` from the bare model: `H_bare_of(v)` builds the bare drift Hamiltonian at sweep value v, and ONE batched
    `dressing.dress_batch` call dresses every point (with the control Hamiltonians `hks_bare` [K,D,D] and, for an open system, the
    bare collapse operators `col_ops_bare_of(v)` [C,D,D]) instead of one host eigendecomposition per point.  `psi_init_of` as in
    `sensitivity_sweep`.  Also returns the "eigenframe" [P,D] of the points."""
    from . import dressing

    vals = list(sweep_values)
    P = len(vals)
    H = np.stack([np.asarray(H_bare_of(v), dtype=np.complex128) for v in vals])
    col_bare = None if col_ops_bare_of is None else np.stack([np.asarray(col_ops_bare_of(v), dtype=np.complex128) for v in vals])
    ops, K, _, _ = _bare_operator_list(hks_bare, col_bare, P, device)
    if device is not None:
        import torch

        H = torch.as_tensor(H, device=device)
    d = dressing.dress_batch(H, ops)
    sig = {g: np.broadcast_to(np.asarray(s, dtype=np.float64)[None], (P,) + tuple(np.shape(s))).copy() for g, s in gate_signals_one.items()}
    if psi_init_of is not None:
        psi_init = np.stack([np.asarray(psi_init_of(v), dtype=np.complex128).reshape(-1) for v in vals])  # [P,D] or [P,D^2]
        if P == 1:
            psi_init = psi_init[0]
    col = None if col_bare is None else d["ops"][:, K:]
    r = goal_run_batched(d["h0"], d["ops"][:, :K], sig, dt, [data_set] * P, psi_init, label_indices, device=device, col_ops=col, readout=readout,
                         estimator=estimator)
    return {"values": np.asarray(vals), "goals": r["goals"], "sim_vals": r["sim_vals"], "eigenframe": dressing._host(d["eigenframe"])}
