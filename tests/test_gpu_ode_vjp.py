"""GPU checks of the discrete adjoint of the ODE state solvers (c3p_ode_solve_vjp, c3p_ode_vjp.hip) against the numpy
restatement of tests/ode_adjoint_ref.py (bar 1e-10 max|want|) and against finite differences of the GPU forward solver
(2e-6 relative)."""
import numpy as np
import pytest

import ode_adjoint_ref as ref
from c3_amd import _lib, workloads
from oracle import c3_oracle as o

pytestmark = pytest.mark.gpu
TOL = 1e-10
SOLVERS = ["rk4", "rk38", "rk5", "tsit5"]


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import _lib, propagation

    _lib.require_gpu()
    return propagation


def _herm(rng, D, s):
    a = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    return s * (a + a.conj().T) / 2


def _problem(D, K, B, N, seed, lossy=False):
    """Operators at the scale of tests/test_gpu_round3.py::_ode_problem; lossy: a non-Hermitian drift."""
    rng = np.random.default_rng(seed)
    h0 = _herm(rng, D, 0.3)
    if lossy:
        h0 = h0 - 0.05j * np.diag(rng.uniform(0, 1, D))
    hks = np.stack([_herm(rng, D, 0.2) for _ in range(K)]).reshape(K, D, D)
    sig = rng.uniform(-1, 1, size=(B, K, N))
    return rng, h0, hks, sig, 0.05


def _cplx(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _rho(rng, B, D):
    a = _cplx(rng, (B, D, D))
    r = a @ np.conj(np.swapaxes(a, -1, -2))
    return r / np.trace(r, axis1=-2, axis2=-1).real[:, None, None]


def _close(got, want, what, tol=TOL):
    got, want = np.asarray(got), np.asarray(want)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{what}: {err:.2e} of max|want|")
    assert err < tol, (what, err)


# 1. lane-row class -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("D", [2, 3, 5, 9, 12, 16])
def test_lane_row_class(prop, D, K, solver):
    """Schroedinger step, D <= 16, K <= 4: Hermitian operators with a shared initial state (the instance that shares the
    operator rows with the adjoint) and a lossy drift with per-sample initial states (the general instance)."""
    B, N = 7, 33
    for lossy, per_sample in [(False, False), (True, True)]:
        rng, h0, hks, sig, dt = _problem(D, K, B, N, 100 * D + K, lossy)
        init = _cplx(rng, (B, D, 1)) if per_sample else _cplx(rng, (D, 1))
        bar = _cplx(rng, (B, D, 1))
        r = prop.ode_solve_batch_vjp(h0, hks, sig, dt, init, bar, solver, "schrodinger")
        assert _lib.last_kernel() == "ode_vjp"
        detail = _lib.last_kernel_detail()
        assert "ode_vjp_row_kernel" in detail and "checkpoint interval C=" in detail, detail
        g, ib = ref.vjp_batch(h0, hks, sig, dt, init, solver, "schrodinger", bar)
        _close(r["grad_signals"], g, f"grad_signals lossy={lossy}")
        _close(r["init_bar"], ib, f"init_bar lossy={lossy}")
        fin = prop.ode_solve_batch(h0, hks, sig, dt, init, solver, "schrodinger", final_only=True)
        assert np.abs(np.asarray(r["states"]) - np.asarray(fin)).max() < 1e-13


# 2. general path ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("solver", ["rk4", "tsit5"])
@pytest.mark.parametrize("D,C", [(3, 0), (3, 1), (4, 2), (9, 0), (9, 1), (4, 0), (9, 2), (3, 2), (4, 1)])
def test_general_path_density_matrices(prop, D, C, solver):
    """von Neumann (C = 0) and Lindblad steps on the workgroup-per-sample kernel, lossy drift."""
    B, K, N = 3, 2, 11
    rng, h0, hks, sig, dt = _problem(D, K, B, N, 7 * D + C, lossy=True)
    col = 0.1 * _cplx(rng, (C, D, D)) if C else None
    step = "lindblad" if C else "von_neumann"
    init = _rho(rng, B, D)
    bar = _cplx(rng, (B, D, D))
    r = prop.ode_solve_batch_vjp(h0, hks, sig, dt, init, bar, solver, step, col_ops=col)
    assert _lib.last_kernel() == "ode_vjp" and "ode_vjp_wg_kernel" in _lib.last_kernel_detail()
    g, ib = ref.vjp_batch(h0, hks, sig, dt, init, solver, step, bar, col=col)
    _close(r["grad_signals"], g, "grad_signals")
    _close(r["init_bar"], ib, "init_bar")
    fin = prop.ode_solve_batch(h0, hks, sig, dt, init, solver, step, col_ops=col, final_only=True)
    assert np.abs(np.asarray(r["states"]) - np.asarray(fin)).max() < 1e-12


@pytest.mark.parametrize("D,K", [(20, 2), (33, 1), (5, 6)])
def test_general_path_vector_states(prop, D, K):
    """Schroedinger step outside the lane-row class: D > 16, and more than four control lines."""
    B, N = 3, 9
    rng, h0, hks, sig, dt = _problem(D, K, B, N, D + K, lossy=True)
    init = _cplx(rng, (D, 1))
    bar = _cplx(rng, (B, D, 1))
    for solver in ("rk38", "rk5"):
        r = prop.ode_solve_batch_vjp(h0, hks, sig, dt, init, bar, solver, "schrodinger")
        assert "ode_vjp_wg_kernel" in _lib.last_kernel_detail()
        g, ib = ref.vjp_batch(h0, hks, sig, dt, init, solver, "schrodinger", bar)
        _close(r["grad_signals"], g, "grad_signals")
        _close(r["init_bar"], ib, "init_bar")


# 3. trajectory cotangents ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("step,D,K", [("schrodinger", 5, 2), ("schrodinger", 16, 3), ("von_neumann", 3, 1), ("lindblad", 4, 2), ("schrodinger", 20, 1)])
def test_trajectory_cotangents(prop, step, D, K):
    B, N = 5, 21
    rng, h0, hks, sig, dt = _problem(D, K, B, N, 3 * D + K, lossy=True)
    M = 1 if step == "schrodinger" else D
    col = 0.1 * _cplx(rng, (2, D, D)) if step == "lindblad" else None
    init = _cplx(rng, (B, D, 1)) if M == 1 else _rho(rng, B, D)
    bar = _cplx(rng, (B, N, D, M))
    for solver in ("rk4", "tsit5"):
        r = prop.ode_solve_batch_vjp(h0, hks, sig, dt, init, bar, solver, step, col_ops=col)
        g, ib = ref.vjp_batch(h0, hks, sig, dt, init, solver, step, bar, col=col, bar_all=True)
        _close(r["grad_signals"], g, "grad_signals")
        _close(r["init_bar"], ib, "init_bar")


# 4. target mode ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("step,D", [("schrodinger", 3), ("schrodinger", 9), ("schrodinger", 20), ("von_neumann", 3), ("lindblad", 4)])
def test_target_mode(prop, step, D):
    """The call forms the state-transfer goal from its own final state and starts the sweep from its cotangent."""
    B, K, N = 5, 2, 17
    rng, h0, hks, sig, dt = _problem(D, K, B, N, 5 * D, lossy=True)
    M = 1 if step == "schrodinger" else D
    col = 0.1 * _cplx(rng, (2, D, D)) if step == "lindblad" else None
    init = _cplx(rng, (B, D, 1)) / np.sqrt(2 * D) if M == 1 else _rho(rng, B, D)
    for tgt in (_cplx(rng, (D, 1)), _cplx(rng, (B, D, 1))):
        tgt = tgt / np.linalg.norm(tgt, axis=-2, keepdims=True)
        r = prop.ode_goal_vjp(h0, hks, sig, dt, init, tgt, "tsit5", step, col_ops=col)
        fin = np.asarray(prop.ode_solve_batch(h0, hks, sig, dt, init, "tsit5", step, col_ops=col, final_only=True))
        bars, want = [], []
        for b in range(B):
            t = tgt[b] if tgt.ndim == 3 else tgt
            f, bar = (ref.ketket_infid_and_bar if M == 1 else ref.dmket_infid_and_bar)(t, fin[b])
            want.append(f)
            bars.append(bar.reshape(D, M))
        assert np.abs(np.asarray(r["goal"]) - np.asarray(want)).max() < 1e-13
        e = prop.ode_solve_batch_vjp(h0, hks, sig, dt, init, np.stack(bars), "tsit5", step, col_ops=col)
        _close(r["grad_signals"], e["grad_signals"], "grad_signals", 1e-12)
        _close(r["init_bar"], e["init_bar"], "init_bar", 1e-12)


def test_target_mode_zero_overlap_gives_a_zero_cotangent(prop):
    D, B, K, N = 3, 2, 1, 5
    rng, h0, hks, sig, dt = _problem(D, K, B, N, 1)
    h0 = np.diag([0.1, 0.2, 0.3]).astype(complex)
    hks = np.zeros((K, D, D), dtype=complex)
    init = np.array([[1], [0], [0]], dtype=complex)
    tgt = np.array([[0], [1], [0]], dtype=complex)
    r = prop.ode_goal_vjp(h0, hks, sig, dt, init, tgt, "rk4", "schrodinger")
    assert np.array_equal(np.asarray(r["goal"]), np.ones(B))
    assert not np.asarray(r["grad_signals"]).any() and not np.asarray(r["init_bar"]).any()


# 5. finite differences of the GPU forward solver -------------------------------------------------------------------


@pytest.mark.parametrize("step,D,K", [("schrodinger", 9, 2), ("schrodinger", 16, 4), ("lindblad", 4, 2), ("schrodinger", 24, 1)])
def test_directional_derivative_of_the_gpu_forward_solver(prop, step, D, K):
    B, N = 4, 40
    rng, h0, hks, sig, dt = _problem(D, K, B, N, 11 * D, lossy=True)
    M = 1 if step == "schrodinger" else D
    col = 0.1 * _cplx(rng, (1, D, D)) if step == "lindblad" else None
    init = _cplx(rng, (B, D, 1)) if M == 1 else _rho(rng, B, D)
    bar = _cplx(rng, (B, D, M))
    ds, dy = rng.normal(size=sig.shape), _cplx(rng, init.shape)
    r = prop.ode_solve_batch_vjp(h0, hks, sig, dt, init, bar, "tsit5", step, col_ops=col)
    want = (np.asarray(r["grad_signals"]) * ds).sum(axis=(1, 2)) + np.real(np.conj(np.asarray(r["init_bar"])) * dy).sum(axis=(1, 2))

    def loss(e):
        fin = np.asarray(prop.ode_solve_batch(h0, hks, sig + e * ds, dt, init + e * dy, "tsit5", step, col_ops=col, final_only=True))
        return np.real(np.conj(bar) * fin).sum(axis=(1, 2))

    eps = 1e-5
    fd = (loss(eps) - loss(-eps)) / (2 * eps)
    rel = np.abs(fd - want) / np.abs(fd)
    print("finite-difference relative errors", rel)
    assert rel.max() < 2e-6


# 6. full size ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("solver", ["rk4", "tsit5"])
def test_full_size_cfg2(prop, solver):
    """cfg2 operators, N = 1000, B = 256, device resident: four samples against the helper (its own rounding was measured at
    7e-14 of max|g| against extended precision), every sample finite, two calls bitwise equal."""
    import torch

    w = workloads.make_workload(2, B=256, N=1000)
    D = w.h0.shape[-1]
    rng = np.random.default_rng(4)
    init = np.zeros((D, 1), dtype=complex)
    init[0] = 1
    bar = _cplx(rng, (256, D, 1))
    dev = torch.device("cuda:0")
    args = [torch.as_tensor(x, device=dev) for x in (w.h0, w.hks, w.signals)]
    r = prop.ode_solve_batch_vjp(*args, w.dt, torch.as_tensor(init, device=dev), torch.as_tensor(bar, device=dev), solver, "schrodinger")
    assert r["grad_signals"].is_cuda and r["init_bar"].is_cuda
    assert "ode_vjp_row_kernel" in _lib.last_kernel_detail()
    r2 = prop.ode_solve_batch_vjp(*args, w.dt, torch.as_tensor(init, device=dev), torch.as_tensor(bar, device=dev), solver, "schrodinger")
    g, ib = r["grad_signals"].cpu().numpy(), r["init_bar"].cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(ib).all()
    assert np.array_equal(g, r2["grad_signals"].cpu().numpy()) and np.array_equal(ib, r2["init_bar"].cpu().numpy())
    for b in (0, 85, 170, 255):
        gw, iw = ref.vjp(w.h0, w.hks, w.signals[b], w.dt, init, solver, "schrodinger", bar[b])
        _close(g[b], gw, f"sample {b} grad_signals")
        _close(ib[b], iw, f"sample {b} init_bar")


# 7. edges ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("N", [2, 3, 16, 17, 25, 26, 36, 37])
@pytest.mark.parametrize("step,D", [("schrodinger", 4), ("von_neumann", 3)])
def test_edges_in_the_number_of_samples(prop, step, D, N):
    """N = 2, and N at and one past a multiple of the checkpoint interval C = ceil(sqrt(N)) (N = 16: C = 4; 25: 5; 36: 6)."""
    B, K = 5, 2
    rng, h0, hks, sig, dt = _problem(D, K, B, N, N + D, lossy=True)
    M = 1 if step == "schrodinger" else D
    init = _cplx(rng, (B, D, M))
    bar = _cplx(rng, (B, D, M))
    r = prop.ode_solve_batch_vjp(h0, hks, sig, dt, init, bar, "rk5", step)
    g, ib = ref.vjp_batch(h0, hks, sig, dt, init, "rk5", step, bar)
    _close(r["grad_signals"], g, "grad_signals")
    _close(r["init_bar"], ib, "init_bar")


def test_checkpoint_interval_is_reported(prop):
    rng, h0, hks, sig, dt = _problem(4, 2, 3, 36, 2)
    prop.ode_solve_batch_vjp(h0, hks, sig, dt, _cplx(rng, (4, 1)), _cplx(rng, (3, 4, 1)), "rk4", "schrodinger")
    assert "checkpoint interval C=6 " in _lib.last_kernel_detail() + " "
    rng, h0, hks, sig, dt = _problem(4, 2, 3, 1200, 2)
    prop.ode_solve_batch_vjp(h0, hks, sig, dt, _cplx(rng, (4, 1)), _cplx(rng, (3, 4, 1)), "rk4", "schrodinger")
    assert "checkpoint interval C=32 " in _lib.last_kernel_detail() + " "  # the cap


@pytest.mark.parametrize("step,D", [("schrodinger", 5), ("schrodinger", 20), ("lindblad", 3)])
def test_zero_cotangent_gives_exact_zeros_and_empty_batch(prop, step, D):
    B, K, N = 3, 2, 12
    rng, h0, hks, sig, dt = _problem(D, K, B, N, D)
    M = 1 if step == "schrodinger" else D
    col = 0.1 * _cplx(rng, (1, D, D)) if step == "lindblad" else None
    init = _cplx(rng, (D, M))
    r = prop.ode_solve_batch_vjp(h0, hks, sig, dt, init, np.zeros((B, D, M), dtype=complex), "tsit5", step, col_ops=col)
    assert not np.asarray(r["grad_signals"]).any() and not np.asarray(r["init_bar"]).any()
    r = prop.ode_solve_batch_vjp(h0, hks, sig[:0], dt, init, np.zeros((0, D, M), dtype=complex), "tsit5", step, col_ops=col)
    assert np.asarray(r["grad_signals"]).shape == (0, K, N) and np.asarray(r["init_bar"]).shape == (0, D, M)


# 8. errors ---------------------------------------------------------------------------------------------------------


def test_errors(prop, lib):
    import ctypes as C

    from c3_amd._lib import C3PropError

    D, B, K, N = 3, 2, 1, 6
    rng, h0, hks, sig, dt = _problem(D, K, B, N, 1)
    psi, bar = _cplx(rng, (D, 1)), _cplx(rng, (B, D, 1))
    # both / neither of states_bar and target: at the C ABI and in the host layer
    grad = np.empty((B, K, N))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for sb, tg in ((p(bar), p(psi)), (None, None)):
        rc = lib.c3p_ode_solve_vjp(p(h0), p(hks), p(sig), None, 0, dt, B, K, N, D, 0, 0, p(psi), 0, sb, 0, tg, 0, _lib.HOST_PTRS, p(grad), None, None, None, None)
        assert rc != 0 and b"exactly one" in lib.c3p_last_error()
    with pytest.raises(C3PropError, match="exactly one"):
        prop._ode_vjp_call(h0, hks, sig, dt, psi, "rk4", "schrodinger", None, bar, psi, True)
    with pytest.raises(C3PropError, match="exactly one"):
        prop._ode_vjp_call(h0, hks, sig, dt, psi, "rk4", "schrodinger", None, None, None, True)
    with pytest.raises(C3PropError, match="states_bar must be"):
        prop.ode_solve_batch_vjp(h0, hks, sig, dt, psi, bar[:, :2], "rk4", "schrodinger")
    with pytest.raises(C3PropError, match="target must be"):
        prop.ode_goal_vjp(h0, hks, sig, dt, psi, np.ones((D, D), dtype=complex), "rk4", "schrodinger")
    with pytest.raises(C3PropError, match="initial state must be"):
        prop.ode_solve_batch_vjp(h0, hks, sig, dt, _cplx(rng, (D, D)), bar, "rk4", "schrodinger")
    with pytest.raises(C3PropError, match="control Hamiltonians"):
        prop.ode_solve_batch_vjp(h0, hks[:, :2, :2], sig, dt, psi, bar, "rk4", "schrodinger")
    with pytest.raises(C3PropError, match="unknown solver"):
        prop.ode_solve_batch_vjp(h0, hks, sig, dt, psi, bar, "euler", "schrodinger")
    with pytest.raises(C3PropError, match="collapse operators"):
        prop.ode_solve_batch_vjp(h0, hks, sig, dt, _cplx(rng, (D, D)), _cplx(rng, (B, D, D)), "rk4", "lindblad")
    with pytest.raises(C3PropError, match="at least two time samples"):
        prop.ode_solve_batch_vjp(h0, hks, sig[:, :, :1], dt, psi, bar, "rk4", "schrodinger")


# 9. goal_run_ode_with_grad -----------------------------------------------------------------------------------------


def test_goal_run_ode_with_grad_on_a_qutrit(prop):
    """envelope rows -> state-transfer goal and d goal / d (amp, xy_angle, freq_offset, delta) on the device, against the
    oracle pipeline (generate_signal -> ode_solver_arrays -> 1 - |<t|psi>|) and its central differences."""
    from c3_amd import optimal_control as oc, signals as sg

    TWO_PI = 2 * np.pi
    D = 3
    a = np.diag(np.sqrt(np.arange(1, D)), 1).astype(complex)
    n = a.conj().T @ a
    h0 = TWO_PI * (5e9 * n - 0.5 * 210e6 * (n @ n - n))
    hks = TWO_PI * (a + a.conj().T)[None]
    T, awg_res, sim_res = 3e-9, 2e9, 400e9
    B = 2
    amps = np.array([0.4e8, 0.6e8])
    chans = [[dict(shape="gaussian_nonorm", amp=amps, xy_angle=0.3, freq_offset=-30e6 * TWO_PI, delta=-0.5, t_final=T, sigma=T / 4, use_t_before=True, drag=True)]]
    env, shapes = sg.pack_components(chans, B=B)
    carrier = np.tile(np.array([[5.0e9 * TWO_PI, 1.0]]), (B, 1, 1))
    init = np.array([[1], [0], [0]], dtype=complex)
    tgt = np.array([[1], [-1j], [0]], dtype=complex) / np.sqrt(2)
    r = oc.goal_run_ode_with_grad(h0, hks, env, shapes, carrier, 0.0, T, awg_res, sim_res, init, tgt, solver="rk4")
    goal, genv = r["goal"].cpu().numpy(), r["grad_env"].cpu().numpy()
    assert tuple(r["init_bar"].shape) == (B, D, 1) and tuple(r["states"].shape) == (B, D, 1)
    ts = o.create_ts(0.0, T, sim_res)

    def oracle_goal(env_b, b):
        c = {name: env_b[0, 0, slot] for name, slot in sg.ENV_SLOTS.items() if name != "flags"}
        fl = int(env_b[0, 0, sg.ENV_SLOTS["flags"]])
        c.update(shape=int(shapes[0, 0]), use_t_before=bool(fl & 1), drag=bool(fl & 2))
        s = o.generate_signal([c], carrier[b, 0, 0], carrier[b, 0, 1], 0.0, T, awg_res, sim_res)["values"]
        fin = o.ode_solver_arrays(h0, hks, s[None], ts, init, "rk4", "schrodinger", final_only=True)["states"]
        return 1 - abs(np.vdot(tgt, fin))

    for b in range(B):
        assert abs(goal[b] - oracle_goal(env[b], b)) < 1e-11
        for name, h in [("amp", 1e2), ("xy_angle", 1e-6), ("delta", 1e-5), ("freq_offset", 1e3)]:
            ep, em = env[b].copy(), env[b].copy()
            ep[0, 0, sg.ENV_SLOTS[name]] += h
            em[0, 0, sg.ENV_SLOTS[name]] -= h
            fd = (oracle_goal(ep, b) - oracle_goal(em, b)) / (2 * h)
            got = genv[b, 0, 0, sg.ENV_SLOTS[name]]
            print(name, fd, got, abs(fd - got) / abs(fd))
            assert abs(fd - got) < 2e-6 * abs(fd) + 1e-16, (b, name)
