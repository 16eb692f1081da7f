"""CPU checks of the ODE adjoint: the numpy restatement of the discrete adjoint (tests/ode_adjoint_ref.py) against central
differences of the oracle's solvers, its interpolation weights against interpolate_signal, the C ABI declaration and binding,
and the state fidelities with their cotangents."""
import os
import re

import numpy as np
import pytest

import ode_adjoint_ref as ref
from oracle import c3_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _herm(rng, D, s):
    a = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    return s * (a + a.conj().T) / 2


def _problem(D, K, N, seed, lossy=True):
    """Operators at the scale of tests/test_gpu_round3.py::_ode_problem, with a non-Hermitian drift."""
    rng = np.random.default_rng(seed)
    h0 = _herm(rng, D, 0.3)
    if lossy:
        h0 = h0 - 0.05j * np.diag(rng.uniform(0, 1, D))
    hks = np.stack([_herm(rng, D, 0.2) for _ in range(K)])
    sig = rng.uniform(-1, 1, size=(K, N))
    ts = (np.arange(N) + 0.5) * 0.05
    return rng, h0, hks, sig, ts


def _state(rng, D, step):
    if step == "schrodinger":
        return rng.normal(size=(D, 1)) + 1j * rng.normal(size=(D, 1))
    a = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    return a @ a.conj().T / np.trace(a @ a.conj().T).real


@pytest.mark.parametrize("step", ["schrodinger", "von_neumann", "lindblad"])
@pytest.mark.parametrize("solver", ["rk4", "rk38", "rk5", "tsit5"])
def test_helper_forward_reproduces_the_oracle(solver, step):
    D, K, N = 4, 2, 9
    rng, h0, hks, sig, ts = _problem(D, K, N, 11)
    col = [0.1 * (rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))) for _ in range(2)] if step == "lindblad" else None
    y0 = _state(rng, D, step)
    want = o.ode_solver_arrays(h0, hks, sig, ts, y0, solver, step, col=col)["states"]
    got = ref.forward(h0, hks, sig, ts[1] - ts[0], y0, solver, step, col)
    assert np.abs(got - want).max() < 1e-13


@pytest.mark.parametrize("step", ["schrodinger", "von_neumann", "lindblad"])
@pytest.mark.parametrize("solver", ["rk4", "rk38", "rk5", "tsit5"])
def test_helper_against_central_differences_of_the_oracle(solver, step):
    """Bar 1e-6 max|g| (the figure of tests/test_gradient.py); the issue's prototype measured 6.4e-8 (signals) and 4e-10
    (initial state) on this problem class."""
    D, K, N = 4, 2, 9
    rng, h0, hks, sig, ts = _problem(D, K, N, 5)
    col = [0.1 * (rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))) for _ in range(2)] if step == "lindblad" else None
    y0 = _state(rng, D, step)
    ybar = rng.normal(size=y0.shape) + 1j * rng.normal(size=y0.shape)
    dt = ts[1] - ts[0]
    g, ib = ref.vjp(h0, hks, sig, dt, y0, solver, step, ybar, col)

    def loss(s, y):
        fin = o.ode_solver_arrays(h0, hks, s, ts, y, solver, step, col=col, final_only=True)["states"]
        return np.real(np.vdot(ybar, fin))

    eps = 1e-6
    worst = 0.0
    for k in range(K):
        for n in range(N):
            sp, sm = sig.copy(), sig.copy()
            sp[k, n] += eps
            sm[k, n] -= eps
            fd = (loss(sp, y0) - loss(sm, y0)) / (2 * eps)
            worst = max(worst, abs(fd - g[k, n]))
    print(f"{solver} {step}: signal gradient error {worst / np.abs(g).max():.2e} of max|g|")
    assert worst < 1e-6 * np.abs(g).max()
    worst = 0.0
    for e in range(y0.size):
        for d in (1.0, 1j):
            dy = np.zeros(y0.size, dtype=complex)
            dy[e] = d
            dy = dy.reshape(y0.shape)
            fd = (loss(sig, y0 + eps * dy) - loss(sig, y0 - eps * dy)) / (2 * eps)
            worst = max(worst, abs(fd - np.real(np.vdot(ib, dy))))
    assert worst < 1e-6 * np.abs(ib).max()


def test_helper_trajectory_cotangents_against_central_differences():
    D, K, N = 3, 2, 7
    rng, h0, hks, sig, ts = _problem(D, K, N, 9)
    y0 = _state(rng, D, "schrodinger")
    bar = rng.normal(size=(N, D, 1)) + 1j * rng.normal(size=(N, D, 1))
    g, _ = ref.vjp(h0, hks, sig, ts[1] - ts[0], y0, "tsit5", "schrodinger", bar, bar_all=True)

    def loss(s):
        return np.real(np.vdot(bar, o.ode_solver_arrays(h0, hks, s, ts, y0, "tsit5", "schrodinger")["states"]))

    eps = 1e-6
    for k in range(K):
        for n in range(N):
            sp, sm = sig.copy(), sig.copy()
            sp[k, n] += eps
            sm[k, n] -= eps
            assert abs((loss(sp) - loss(sm)) / (2 * eps) - g[k, n]) < 1e-6 * np.abs(g).max()


@pytest.mark.parametrize("solver,interp", [("rk4", 2), ("rk38", 3), ("rk5", -1), ("tsit5", -2)])
def test_interpolation_weights_reproduce_interpolate_signal(solver, interp):
    """(lo, tau) of the helper against the oracle's interpolate_signal on its own stage grid, the extrapolated nodes of the
    last step included."""
    N = 11
    rng = np.random.default_rng(3)
    sig = rng.uniform(-1, 1, N)
    ts = (np.arange(N) + 0.5) * 0.05
    grid = o.interpolate_signal(ts, sig, interp)
    times = o.interpolation_times(ts, interp)
    nodes = ref.TABLEAUX[solver][2]
    dt = ts[1] - ts[0]
    seen_extrapolation = False
    for n in range(N):
        for node in nodes:
            lo, tau = ref.interp_weights(n, node, N)
            assert 0 <= lo <= N - 2
            seen_extrapolation |= tau > 1
            c = (1 - tau) * sig[lo] + tau * sig[lo + 1]
            j = np.argmin(np.abs(times - (ts[0] + (n + node) * dt)))
            assert abs(times[j] - (ts[0] + (n + node) * dt)) < 1e-12
            assert abs(grid[j] - c) < 1e-13
    assert seen_extrapolation


def test_header_binding_and_kernel_id():
    from c3_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "c3prop.h")).read()
    assert re.search(r"#define C3P_KERNEL_ODE_VJP 11\b", hdr)
    m = re.search(r"int c3p_ode_solve_vjp\(([^;]*)\);", hdr)
    assert m, "c3p_ode_solve_vjp is not declared"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert "c3p_ode_solve_vjp" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["c3p_ode_solve_vjp"][1]) == nargs == 24
    assert _lib.KERNEL_NAMES[11] == "ode_vjp"
    # the header comment cites the reference's loop bodies and the state fidelity
    doc = hdr[hdr.index("Discrete adjoint of c3p_ode_solve") : m.start()]
    for cite in ("optimalcontrol.py:230-292", "optimizer.py:206-216", "fidelities.py:793-816", "tf_utils.py:325-327", "tf_utils.py:320-322"):
        assert cite in doc
    api = open(os.path.join(ROOT, "c3_amd", "csrc", "c3p_api.hip")).read()
    assert "int c3p_ode_solve_vjp(" in api
    import __graft_entry__ as g

    assert "c3p_ode_vjp.hip" in g.HIP_SOURCES


def test_entries_raise_without_a_gpu():
    import torch

    from c3_amd import optimal_control, propagation
    from c3_amd._lib import C3PropError

    assert callable(optimal_control.goal_run_ode_with_grad)
    if torch.cuda.is_available():
        return  # (with a GPU the entries are exercised by tests/test_gpu_ode_vjp.py)

    rng, h0, hks, sig, ts = _problem(3, 1, 5, 1)
    psi = np.ones((3, 1), dtype=complex)
    with pytest.raises(C3PropError):
        propagation.ode_solve_batch_vjp(h0, hks, sig[None], 0.05, psi, psi[None])
    with pytest.raises(C3PropError):
        propagation.ode_goal_vjp(h0, hks, sig[None], 0.05, psi, psi)


def test_state_fidelities_and_cotangents_against_directional_differences():
    from c3_amd import fidelities as F

    for name in ("calculate_state_overlap", "state_transfer_from_states", "state_transfer_infid", "state_transfer_infid_set"):
        assert name in F.fidelities
    rng = np.random.default_rng(2)
    D = 4
    t = rng.normal(size=(D, 1)) + 1j * rng.normal(size=(D, 1))
    t /= np.linalg.norm(t)
    psi = rng.normal(size=(D, 1)) + 1j * rng.normal(size=(D, 1))
    assert abs(F.calculate_state_overlap(psi, t) - abs(np.vdot(t, psi))) < 1e-14
    a = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    rho = a @ a.conj().T
    rho /= np.trace(rho).real
    assert abs(F.calculate_state_overlap(rho, t) - np.sqrt(np.real(t.conj().T @ rho @ t)).item()) < 1e-14
    traj = np.stack([rng.normal(size=(D, 1)) + 1j * rng.normal(size=(D, 1)) for _ in range(3)] + [psi])
    assert abs(F.state_transfer_from_states(traj, None, None, {"target": t}) - (1 - abs(np.vdot(t, psi)))) < 1e-14
    assert abs(F.state_transfer_from_states(psi, None, None, {"target": t}) - (1 - abs(np.vdot(t, psi)))) < 1e-14
    # cotangents of the helper (what the kernels start their sweep from) along random directions
    eps = 1e-6
    f0, bar = ref.ketket_infid_and_bar(t, psi)
    d = rng.normal(size=psi.shape) + 1j * rng.normal(size=psi.shape)
    fd = (ref.ketket_infid_and_bar(t, psi + eps * d)[0] - ref.ketket_infid_and_bar(t, psi - eps * d)[0]) / (2 * eps)
    assert abs(fd - np.real(np.vdot(bar, d))) < 1e-8
    f0, bar = ref.dmket_infid_and_bar(t, rho)
    d = rng.normal(size=rho.shape) + 1j * rng.normal(size=rho.shape)
    d = d + d.conj().T
    fd = (ref.dmket_infid_and_bar(t, rho + eps * d)[0] - ref.dmket_infid_and_bar(t, rho - eps * d)[0]) / (2 * eps)
    assert abs(fd - np.real(np.vdot(bar, d))) < 1e-8
    # state_transfer_infid on a propagator and its rank-one cotangent (qubit in a qutrit: dims [3], index [0])
    dims, index = [3], [0]
    U = np.linalg.qr(rng.normal(size=(3, 3)) + 1j * rng.normal(size=(3, 3)))[0]
    G = np.array([[0, 1], [1, 0]], dtype=complex)
    psi0 = np.array([[1], [0]], dtype=complex)
    P = np.eye(3)[:, :2]
    want = 1 - abs(np.vdot(G @ psi0, P.T @ U @ P @ psi0))
    assert abs(F.state_transfer_infid(G, U, index, dims, psi0) - want) < 1e-14
    assert abs(F.state_transfer_infid_set({"x": U}, {"x": G}, index, dims, psi0) - want) < 1e-14
    Ubar, infid = F.state_transfer_infid_cotangent(G, U, index, dims, psi0)
    assert abs(infid - want) < 1e-14
    dU = rng.normal(size=(3, 3)) + 1j * rng.normal(size=(3, 3))
    fd = (F.state_transfer_infid(G, U + eps * dU, index, dims, psi0) - F.state_transfer_infid(G, U - eps * dU, index, dims, psi0)) / (2 * eps)
    assert abs(fd - np.real(np.vdot(Ubar, dU))) < 1e-8
    assert np.linalg.matrix_rank(Ubar) == 1
