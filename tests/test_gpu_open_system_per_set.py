"""Open-system model learning with one set of collapse operators and one initial state PER PARAMETER SET on the GPU
(model_learning.goal_run_batched[_with_grad] with col_ops [P,C,D,D] and psi_init [P,D^2]; sensitivity_sweep with col_ops_of).

One qutrit, the model of test_open_system_goal_gradient in tests/test_gpu_lindblad_model_grad.py: D = 3, two gates, N = 20, P = 3,
five sequences of up to six gates.  Set p has its own T1 (the collapse operator sqrt(1 / T1_p) a, beside a fixed dephasing operator)
and its own temperature (thermal_initial_state).  Reference: the numpy restatement on the oracle, evaluated per set.  Bars as in that
test: 1e-10 on sim_vals and goals; derivatives against central differences with a relative step of 1e-5, agreement 1e-6 max|fd|."""
import functools

import numpy as np
import pytest

from c3_amd import _lib
from oracle import c3_oracle as o

pytestmark = pytest.mark.gpu

T1 = np.array([8.0, 15.0, 30.0])  # in the time unit of dt
TEMP = np.array([0.1, 0.15, 0.25])  # K: kb T / hbar of the order of the level spacing, visibly mixed states
LEVELS = 2 * np.pi * np.array([0.0, 5.0e9, 9.8e9])
D, P, K, N, DT = 3, 3, 1, 20, 0.25
A = np.diag(np.sqrt(np.arange(1, D)), 1).astype(complex)
DEPH = 0.1 * np.diag(np.arange(D)).astype(complex)


@pytest.fixture(scope="module")
def ml(lib):
    from c3_amd import model_learning

    _lib.require_gpu()
    return model_learning


def _col(t1):
    return np.stack([np.sqrt(1.0 / t1) * A, DEPH])


@functools.lru_cache(maxsize=None)
def _problem():
    rng = np.random.default_rng(23)
    herm = lambda s: (lambda a: s * (a + a.conj().T) / 2)(rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D)))
    h0 = herm(0.3) + np.diag([0.0, 1.0, 1.8])
    hks = np.stack([herm(0.5)])
    sigs = {"rx90p": rng.uniform(-1, 1, size=(P, K, N)), "ry90p": rng.uniform(-1, 1, size=(P, K, N))}
    seqs = [[], ["rx90p"], ["ry90p", "rx90p", "rx90p"], ["rx90p", "ry90p", "ry90p", "rx90p", "ry90p"], ["ry90p", "ry90p", "rx90p", "ry90p", "rx90p", "rx90p"]]
    return dict(h0=h0, hks=hks, sigs=sigs, seqs=seqs, labels=[0])


def _rho0(ml, temps):
    return np.stack([ml.thermal_initial_state(LEVELS, t) for t in temps])


def _cpu_goal(ml, q, t1s, temps, sigs, data_sets=None):
    """numpy restatement on the oracle, per set with its own collapse operators and initial state: (goal, goals [P], sim_vals [P,S])"""
    sim = np.zeros((P, len(q["seqs"])))
    for p in range(P):
        rho0 = ml.thermal_initial_state(LEVELS, temps[p])
        Us = {g: o.propagate_batch(q["h0"], q["hks"], s[p : p + 1], DT, col_ops=_col(t1s[p]), lindbladian=True)[0] for g, s in sigs.items()}
        for si, S in enumerate(o.evaluate_sequences(Us, q["seqs"])):
            sim[p, si] = o.populations(S @ rho0, True)[q["labels"]].sum()
    if data_sets is None:
        return None, None, sim
    goals = np.array([ml.g_LL_prime(d["results"], sim[p], d["results_std"], d["shots"]) for p, d in enumerate(data_sets)])
    return ml.g_LL_prime_combined(goals, [len(q["seqs"])] * P), goals, sim


def _data(ml, q, sigs):
    sim = _cpu_goal(ml, q, T1, TEMP, sigs)[2]
    S = len(q["seqs"])
    off = np.array([[0.02, -0.015, 0.01, -0.02, 0.015], [-0.01, 0.02, -0.02, 0.015, -0.02], [0.015, -0.02, 0.02, -0.01, 0.01]])
    return [{"seqs": q["seqs"], "results": sim[p] + off[p], "results_std": np.full(S, 0.01), "shots": np.full(S, 1000.0)} for p in range(P)]


def test_forward_per_set(ml):
    q = _problem()
    ds = _data(ml, q, q["sigs"])
    goal, goals, sim = _cpu_goal(ml, q, T1, TEMP, q["sigs"], ds)
    assert 0.01 < sim.min() and sim.max() < 0.99
    # the sets differ through their decoherence and temperature alone as well: with set 0's values everywhere the reference moves
    assert np.abs(_cpu_goal(ml, q, T1[[0, 0, 0]], TEMP[[0, 0, 0]], q["sigs"])[2] - sim).max() > 1e-3
    col = np.stack([_col(t) for t in T1])
    rho0 = _rho0(ml, TEMP)
    assert col.shape == (P, 2, D, D) and rho0.shape == (P, D * D)
    for fn, dev in ((ml.goal_run_batched, None), (ml.goal_run_batched, "cuda:0"), (ml.goal_run_batched_with_grad, None)):
        r = fn(q["h0"], q["hks"], q["sigs"], DT, ds, rho0, q["labels"], col_ops=col, device=dev)
        e_sim, e_goals = np.abs(r["sim_vals"] - sim).max(), np.abs(r["goals"] - goals).max()
        print(f"{fn.__name__} device={dev}: max|sim - ref| = {e_sim:.3e}, max|goals - ref| = {e_goals:.3e}, |goal - ref| = {abs(r['goal'] - goal):.3e}")
        assert e_sim < 1e-10
        assert e_goals < 1e-10 * max(1.0, np.abs(goals).max())
        assert abs(r["goal"] - goal) < 1e-10 * max(1.0, abs(goal))


def test_sensitivity_sweep_over_t1(ml):
    """the sweep builds col_ops (and the initial state) of every point: the goals of goal_run_batched's reference with the pulses and
    the data of one set at every point"""
    q = _problem()
    one = {g: s[0] for g, s in q["sigs"].items()}
    sigs = {g: np.broadcast_to(s[None], (P,) + s.shape).copy() for g, s in one.items()}
    ds = _data(ml, q, sigs)[0]
    _, goals, sim = _cpu_goal(ml, q, T1, TEMP, sigs, [ds] * P)
    assert np.abs(goals - goals[0]).max() > 1e-3 * np.abs(goals).max()
    temp_of = dict(zip(T1, TEMP))
    r = ml.sensitivity_sweep(lambda v: q["h0"], lambda v: q["hks"], T1, one, DT, ds, None, q["labels"], col_ops_of=_col,
                             psi_init_of=lambda v: ml.thermal_initial_state(LEVELS, temp_of[v]))
    print(f"sweep: max|sim - ref| = {np.abs(r['sim_vals'] - sim).max():.3e}, max|goals - ref| = {np.abs(r['goals'] - goals).max():.3e}")
    assert np.array_equal(r["values"], T1)
    assert np.abs(r["sim_vals"] - sim).max() < 1e-10
    assert np.abs(r["goals"] - goals).max() < 1e-10 * max(1.0, np.abs(goals).max())


def test_gradient_of_t1_and_temperature_per_set(ml):
    """grad_col_ops[p] contracted with d col_ops / d T1 (model_param_grads) and grad_psi_init[p] pushed through
    thermal_initial_state_vjp to d goal / d T, each against central differences of the restatement on the oracle"""
    q = _problem()
    ds = _data(ml, q, q["sigs"])
    col = np.stack([_col(t) for t in T1])
    r = ml.goal_run_batched_with_grad(q["h0"], q["hks"], q["sigs"], DT, ds, _rho0(ml, TEMP), q["labels"], col_ops=col)
    assert np.asarray(r["grad_col_ops"]).shape == (P, 2, D, D) and np.asarray(r["grad_psi_init"]).shape == (P, D * D)
    # d col / d T1: -1/2 T1^{-3/2} a on the first collapse operator, per set
    dcol = np.stack([np.stack([-0.5 * t ** -1.5 * A, np.zeros_like(A)])[None] for t in T1])  # [P,1,C,D,D]
    zeros0 = np.zeros((P, 1, D, D), dtype=complex)
    got_t1 = ml.model_param_grads(r["grad_h0"], r["grad_hks"], zeros0, None, r["grad_col_ops"], dcol)[:, 0]
    got_temp = np.array([ml.thermal_initial_state_vjp(LEVELS, TEMP[p], np.asarray(r["grad_psi_init"])[p])[0] for p in range(P)])
    eps = 1e-5
    at = lambda t1s, temps: _cpu_goal(ml, q, t1s, temps, q["sigs"], ds)[0]
    e = np.eye(P)
    fd_t1 = np.array([(at(T1 * (1 + eps * e[p]), TEMP) - at(T1 * (1 - eps * e[p]), TEMP)) / (2 * eps * T1[p]) for p in range(P)])
    fd_temp = np.array([(at(T1, TEMP * (1 + eps * e[p])) - at(T1, TEMP * (1 - eps * e[p]))) / (2 * eps * TEMP[p]) for p in range(P)])
    for what, got, fd in (("d goal / d T1", got_t1, fd_t1), ("d goal / d T", got_temp, fd_temp)):
        bar = 1e-6 * np.abs(fd).max()
        print(f"{what}: got {got}, finite differences {fd}, max diff {np.abs(got - fd).max():.3e} (bar {bar:.3e})")
        assert np.abs(got - fd).max() < bar
        # the three sets have different derivatives, far above the bar: reading another set's operators or state cannot pass
        gaps = [abs(fd[a] - fd[b]) for a in range(P) for b in range(a)]
        assert min(gaps) > 100 * bar, (what, fd)
