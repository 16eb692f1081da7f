"""Batched goal-with-gradient for pulse parameters -- the loop body of the reference's optimizers.

Reference: `Optimizer.goal_run_with_grad` tapes the goal (optimizers/optimizer.py:206-216),
`OptimalControl.goal_run` is `fid_func(compute_propagators())` (optimalcontrol.py:200-228) and
`OptimalControlRobust.goal_run_with_grad` averages goal and gradient over noise instances in a
serial Python loop (optimalcontrol_robust.py:49-70).  Here the B instances are one batch:

  envelope rows --synthesize--> signals --propagate--> U --fidelity--> goal[b]
  d goal/d rows <--synth vjp-- d/d signals <--adjoint sweep-- U_bar <--cotangent--

everything resident in HBM.  The mapping between optimizer coordinates and physical parameter values
(`Quantity` scaling, c3objs.py) stays with the caller: it is element-wise host arithmetic.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import fidelities, propagation, signals
from ._lib import C3PropError

_COTANGENTS = {"unitary_infid": fidelities.unitary_infid_cotangent, "average_infid": fidelities.average_infid_cotangent,
               "lindbladian_unitary_infid": fidelities.lindbladian_unitary_infid_cotangent}


def goal_run_with_grad(
    h0,
    hks,
    env_params,
    env_shapes,
    carrier,
    t_start: float,
    t_end: float,
    awg_res: float,
    sim_res: float,
    ideal,
    index,
    dims,
    *,
    fr_phase=None,
    fid_func: str = "unitary_infid",
    col_ops=None,
    device="cuda:0",
    fused: Optional[bool] = None,
    line_kinds=None,
    line_params=None,
    env_tables=None,
    table_index=None,
    line_filters=None,
    dc_offset=None,
    crosstalk=None,
) -> Dict:
    """goals [B] and their gradients w.r.t. every envelope row, carrier pair and frame-rotation phase.

    Returns {"goal": [B], "grad_env": [B,K,E,NPAR], "grad_carrier": [B,K,2], "grad_fr_phase": [B,D] or None,
    "U": [B,D,D]} as torch CUDA tensors.

    `col_ops` [C,D,D] switches to the open-system path (model.lindbladian, propagation.py:551-585): U are the D^2 x D^2
    superoperators, `fid_func` an open-system goal ("lindbladian_unitary_infid", fidelities.py:221-249), `fr_phase` [B,D^2]
    the row phases of the superoperator, and the control gradient comes from `propagate_batch_lindblad_vjp`.

    `line_kinds` [K] / `line_params` [B,K,LINE_NPAR] (signals.pack_lines) send every line through the chain AWG -> DAC ->
    Response -> Mixer -> VoltsToHertz | FluxTuning instead of the standard drive line; the result then also holds
    "grad_line" [B,K,LINE_NPAR] (phi_0, phi, omega_0, anhar, d; rise_time is not differentiated), on every route below.

    `env_tables` [B,T] / `table_index` [K,E,2] (signals.pack_table_components) bring the coefficients of sampled and Fourier
    envelopes (pwc, pwc_shape, pwc_symmetric, fourier_sin, fourier_cos): the result then holds "grad_tables" [B,T], the
    gradient w.r.t. every coefficient in the layout of env_tables -- what a GRAPE-style optimiser of the AWG samples steps along.

    `line_filters` = (filt_kind [K,F], filt_params [B,K,F,FILT_NPAR]) (signals.pack_line_filters), `dc_offset` [B,K] and
    `crosstalk` [K,K] | [B,K,K] (signals.pack_crosstalk) add distortion stages between DAC and Mixer, an offset behind the
    Mixer and a mixing matrix over the finished lines (`signals.synthesize_signals`); the result then holds "grad_filters"
    [B,K,F,FILT_NPAR], "grad_dc_offset" [B,K] and "grad_crosstalk" [B,K,K] for those passed, on every route below.

    `fused` (closed systems; default: wherever the library serves the shape) takes goal and gradient from ONE pass over the
    chains (`propagation.propagate_batch_goal_vjp`); False runs forward pass, cotangent and vector-Jacobian product as three
    calls -- same numbers, the forward segment products computed twice.
    """
    import torch

    if fid_func not in _COTANGENTS:
        raise C3PropError(f"C3:Error: no cotangent for fidelity '{fid_func}' (have {sorted(_COTANGENTS)})")
    ts = signals.create_ts(t_start, t_end, sim_res)
    if ts.shape[0] < 2:
        raise C3PropError("C3:Error: need at least two time slices")
    dt = float(ts[1] - ts[0])  # propagation.py:310
    as_dev = lambda x, dt_: x.to(device) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=dt_), device=device)
    env = as_dev(env_params, np.float64)
    car = as_dev(carrier, np.float64)
    h0d, hkd = as_dev(h0, np.complex128), as_dev(hks, np.complex128)
    ph = None if fr_phase is None else as_dev(fr_phase, np.float64)
    chain = {}
    if line_kinds is not None or line_params is not None:
        if line_kinds is None or line_params is None:
            raise C3PropError("C3:Error: line_kinds and line_params go together")
        chain = {"line_kinds": line_kinds, "line_params": as_dev(line_params, np.float64)}
    names = ("grad_env", "grad_carrier") + (("grad_line",) if chain else ())
    if env_tables is not None or table_index is not None:
        if env_tables is None or table_index is None:
            raise C3PropError("C3:Error: env_tables and table_index go together")
        chain = dict(chain, env_tables=as_dev(env_tables, np.float64), table_index=table_index)
        names += ("grad_tables",)
    if line_filters is not None:
        chain = dict(chain, line_filters=(line_filters[0], as_dev(line_filters[1], np.float64)))
        names += ("grad_filters",)
    if dc_offset is not None:
        chain = dict(chain, dc_offset=as_dev(dc_offset, np.float64))
        names += ("grad_dc_offset",)
    if crosstalk is not None:
        chain = dict(chain, crosstalk=as_dev(crosstalk, np.float64))
        names += ("grad_crosstalk",)
    sig = signals.synthesize_signals(env, env_shapes, car, t_start, t_end, awg_res, sim_res, **chain)

    def synth_vjp(g_sig):
        """{"grad_env", "grad_carrier"[, "grad_line"][, "grad_tables"][, "grad_filters"][, "grad_dc_offset"][, "grad_crosstalk"]}
        from d goal / d signals"""
        g = signals.synthesize_signals_vjp(env, env_shapes, car, t_start, t_end, awg_res, sim_res, g_sig, **chain)
        return dict(zip(names, g))

    if col_ops is not None:
        if not fid_func.startswith("lindbladian"):
            raise C3PropError(f"C3:Error: '{fid_func}' is a closed-system goal; the Lindblad path needs a lindbladian_* one")
        cold = as_dev(col_ops, np.complex128)
        B, K, N, D = int(sig.shape[0]), int(sig.shape[1]), int(sig.shape[2]), int(h0d.shape[-1])
        tape = None
        if fused is not False and propagation.lindblad_tape_supported(B, K, N, D):
            # ONE forward pass: the superoperators and, on the tape, what their vector-Jacobian product reads (D = 2, 3, 7, 8, 9)
            try:
                r = propagation.propagate_batch_lindblad_taped(h0d, hkd, sig, dt, cold, fr_phase=ph)
                U, tape = r["U"], r["tape"]
            except C3PropError as e:  # a non-Hermitian Hamiltonian: the untaped pair serves it
                if "Hermitian" not in str(e):
                    raise
        if tape is None:
            U = propagation.propagate_batch(h0d, hkd, sig, dt, col_ops=cold, lindbladian=True, fr_phase=ph)["U"]
        U_bar, goal = _COTANGENTS[fid_func](ideal, U, index, dims)
        if tape is not None:
            g_sig = tape.vjp(U_bar)
        else:
            g_sig = propagation.propagate_batch_lindblad_vjp(h0d, hkd, sig, dt, cold, U_bar, fr_phase=ph)
    else:
        if fid_func.startswith("lindbladian"):
            raise C3PropError(f"C3:Error: '{fid_func}' needs collapse operators (col_ops)")
        B, D = int(sig.shape[0]), int(h0d.shape[-1])
        if fused is None:
            fused = propagation.goal_vjp_is_fused(B, D)
        if fused:
            # ONE pass over the chains: the backward pass's scan of the segment products evaluates the goal and starts the
            # adjoint sweep from its cotangent (c3p_pwc_unitary_goal_vjp); no second forward pass, no host-framework ops
            r = propagation.propagate_batch_goal_vjp(h0d, hkd, sig, dt, ideal, index, dims, kind="unitary" if fid_func == "unitary_infid" else "average", fr_phase=ph)
            return {"goal": r["goal"], **synth_vjp(r["grad_signals"]), "grad_fr_phase": r["grad_fr_phase"], "U": r["U"]}
        U = propagation.propagate_batch(h0d, hkd, sig, dt, fr_phase=ph)["U"]
        U_bar, goal = _COTANGENTS[fid_func](ideal, U, index, dims)
        g_sig = propagation.propagate_batch_vjp(h0d, hkd, sig, dt, U_bar, fr_phase=ph)
    g_ph = None
    if ph is not None:
        # U = diag(e^{i phi}) P  =>  d loss/d phi_i = Re sum_j conj(U_bar_ij) (i U_ij) = -Im sum_j conj(U_bar_ij) U_ij
        g_ph = -(torch.conj(U_bar) * U).sum(dim=-1).imag
    return {"goal": goal, **synth_vjp(g_sig), "grad_fr_phase": g_ph, "U": U}


def goal_run_ode_with_grad(
    h0,
    hks,
    env_params,
    env_shapes,
    carrier,
    t_start: float,
    t_end: float,
    awg_res: float,
    sim_res: float,
    init_state,
    target,
    *,
    solver: str = "rk4",
    step_function: str = "schrodinger",
    col_ops=None,
    device="cuda:0",
    env_tables=None,
    table_index=None,
) -> Dict:
    """State-transfer goals [B] and their gradients through the ODE state solvers -- the body of `goal_run_ode_only_final`
    (optimalcontrol.py:262-292: compute_final_state with an RK solver, then state_transfer_from_states, fidelities.py:793-816)
    under the tape of `goal_run_with_grad` (optimizer.py:206-216):

      envelope rows --synthesize--> signals --ode_goal_vjp--> goal[b], d/d signals --synth vjp--> d goal/d rows

    `init_state` [D,M] or [B,D,M] (M = 1: state vector; M = D: density matrix, steps "von_neumann" / "lindblad"), `target` a
    ket [D,1] or [B,D,1].  Returns {"goal": [B], "grad_env": [B,K,E,NPAR], "grad_carrier": [B,K,2], "init_bar": [B,D,M] (the
    cotangent of the initial state: a preceding gate's sweep starts from it), "states": [B,D,M] (the final states)} as
    torch CUDA tensors; with `env_tables` / `table_index` (as in `goal_run_with_grad`) also "grad_tables" [B,T]."""
    import torch

    ts = signals.create_ts(t_start, t_end, sim_res)
    if ts.shape[0] < 2:
        raise C3PropError("C3:Error: need at least two time slices")
    dt = float(ts[1] - ts[0])
    as_dev = lambda x, dt_: x.to(device) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=dt_), device=device)
    env = as_dev(env_params, np.float64)
    car = as_dev(carrier, np.float64)
    h0d, hkd = as_dev(h0, np.complex128), as_dev(hks, np.complex128)
    cold = None if col_ops is None else as_dev(col_ops, np.complex128)
    tab = {}
    if env_tables is not None or table_index is not None:
        if env_tables is None or table_index is None:
            raise C3PropError("C3:Error: env_tables and table_index go together")
        tab = {"env_tables": as_dev(env_tables, np.float64), "table_index": table_index}
    sig = signals.synthesize_signals(env, env_shapes, car, t_start, t_end, awg_res, sim_res, **tab)
    r = propagation.ode_goal_vjp(h0d, hkd, sig, dt, as_dev(init_state, np.complex128), as_dev(target, np.complex128),
                                 solver=solver, step_function=step_function, col_ops=cold)
    g = signals.synthesize_signals_vjp(env, env_shapes, car, t_start, t_end, awg_res, sim_res, r["grad_signals"], **tab)
    out = {"goal": r["goal"], "grad_env": g[0], "grad_carrier": g[1], "init_bar": r["init_bar"], "states": r["states"]}
    if tab:
        out["grad_tables"] = g[2]
    return out


def robust_goal_run_with_grad(*args, **kwargs) -> Dict:
    """Mean goal and mean gradient over the batch of noise instances (optimalcontrol_robust.py:49-70),
    plus the per-instance values and their standard deviation the reference logs (:64-69)."""
    r = goal_run_with_grad(*args, **kwargs)
    out = {"goal": r["goal"].mean(), "goals_individual": r["goal"], "goal_std": r["goal"].std(unbiased=False),
           "grad_env": r["grad_env"].mean(dim=0), "grad_carrier": r["grad_carrier"].mean(dim=0),
           "gradient_std": r["grad_env"].std(dim=0, unbiased=False)}
    if r["grad_fr_phase"] is not None:
        out["grad_fr_phase"] = r["grad_fr_phase"].mean(dim=0)
    if "grad_line" in r:
        out["grad_line"] = r["grad_line"].mean(dim=0)
    for key in ("grad_tables", "grad_filters", "grad_dc_offset", "grad_crosstalk"):
        if key in r:
            out[key] = r[key].mean(dim=0)
    return out
