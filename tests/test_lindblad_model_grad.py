"""Model-operator cotangents of the Lindblad path, host side: the numpy reference (tests/lindblad_model_grad_ref.py) pinned by
finite differences of the pinned propagator oracle, argument validation of the new keyword arguments, the thermal initial state."""
import numpy as np
import pytest

import lindblad_model_grad_ref as ref


def _problem(D=2, C=2, K=2, N=4, seed=7):
    rng = np.random.default_rng(seed)
    cx = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)
    herm = lambda s: (lambda a: s * (a + a.conj().T) / 2)(cx(D, D))
    h0, hks = herm(0.8), np.stack([herm(0.5) for _ in range(K)])
    col = 0.25 * cx(C, D, D)
    sig = rng.uniform(-1, 1, size=(K, N))
    Dm = D * D
    return h0, hks, col, sig, 0.3, cx(Dm, Dm), rng.uniform(0, 2 * np.pi, size=Dm)


def test_reference_cotangents_match_finite_differences():
    """Every entry of h0, hks and col_ops, real and imaginary direction (D = 2, C = 2, K = 2, N = 4, random complex U_bar, row
    phases): central differences of o.propagate_batch(..., lindbladian=True) within 1e-6 max|grad|, the bar of
    test_oracle_lindblad_gradient_matches_finite_differences.  The operators are perturbed as general complex matrices: the
    cotangents assume nothing Hermitian."""
    h0, hks, col, sig, dt, Ubar, ph = _problem()
    g0, gk, gc = ref.lindblad_model_cotangents(h0, hks, col, sig, dt, Ubar, ph)
    ops = {"h0": h0, "hks": hks, "col": col}
    eps = 1e-5
    for name, g in (("h0", g0), ("hks", gk), ("col", gc)):
        assert np.abs(g).max() > 1e-3  # not vacuous
        for idx in np.ndindex(*g.shape):
            fd = 0.0
            for v in (1.0, 1.0j):
                vals = []
                for sgn in (+1, -1):
                    p = {k: a.copy() for k, a in ops.items()}
                    p[name][idx] += sgn * eps * v
                    vals.append(ref.loss(p["h0"], p["hks"], p["col"], sig, dt, Ubar, ph))
                fd = fd + v * (vals[0] - vals[1]) / (2 * eps)
            assert abs(fd - g[idx]) < 1e-6 * np.abs(g).max(), (name, idx, fd, g[idx])


@pytest.fixture
def no_device_needed(lib, monkeypatch):
    """the checks below raise before any library call: let the binding get as far as its argument checks without a GPU"""
    from c3_amd import _lib

    monkeypatch.setattr(_lib, "require_gpu", lambda: None)


def test_lindblad_vjp_model_grads_argument_checks(no_device_needed):
    from c3_amd import propagation
    from c3_amd._lib import C3PropError

    h0, hks, col, sig, dt, Ubar, ph = _problem()
    with pytest.raises(C3PropError, match=r"U_bar must be \[1,4,4\]"):
        propagation.propagate_batch_lindblad_vjp(h0, hks, sig[None], dt, col, Ubar[None, :2, :2], want_model_grads=True)
    with pytest.raises(C3PropError, match="needs collapse operators"):
        propagation.propagate_batch_lindblad_vjp(h0, hks, sig[None], dt, None, Ubar[None], want_model_grads=True)
    with pytest.raises(C3PropError, match=r"fr_phase must be \[1,4\]"):
        propagation.propagate_batch_lindblad_vjp(h0, hks, sig[None], dt, col, Ubar[None], fr_phase=ph[None, :2], want_model_grads=True)


def test_open_system_goal_argument_checks(no_device_needed):
    from c3_amd import model_learning as ml
    from c3_amd._lib import C3PropError

    h0, hks, col, sig, dt, _, _ = _problem()
    sigs = {"rx90p": np.stack([sig, sig])}
    ds = {"seqs": [["rx90p"]], "results": [0.4], "results_std": [0.01], "shots": [1000]}
    for fn in (ml.goal_run_batched, ml.goal_run_batched_with_grad):
        with pytest.raises(C3PropError, match=r"expected a ket \[2\] or a density vector \[4\]"):
            fn(h0, hks, sigs, dt, [ds, ds], np.ones(3), [0], col_ops=col)
        with pytest.raises(C3PropError, match="2 parameter sets, but there are 3 data sets"):
            fn(h0, hks, sigs, dt, [ds, ds, ds], [1, 0], [0], col_ops=col)
        with pytest.raises(C3PropError, match="same sequences"):
            fn(h0, hks, sigs, dt, [ds, dict(ds, seqs=[[]])], [1, 0], [0], col_ops=col)


def test_model_param_grads_with_collapse_operators():
    from c3_amd import model_learning as ml
    from c3_amd._lib import C3PropError

    rng = np.random.default_rng(2)
    cx = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)
    P, T, K, C, D = 3, 2, 2, 2, 3
    g0, gk, gc = cx(P, D, D), cx(P, K, D, D), cx(P, C, D, D)
    dh0, dcol = cx(T, D, D), cx(T, C, D, D)
    want = np.array([sum(np.real(np.vdot(g0[p], dh0[t]) + np.vdot(gc[p], dcol[t])) for p in range(P)) for t in range(T)])
    got = ml.model_param_grads(g0, gk, dh0, grad_col_ops=gc, dcol_ops=dcol)
    assert got.shape == (T,) and np.abs(got - want).max() < 1e-13 * np.abs(want).max()
    dh0p, dcolp = cx(P, T, D, D), cx(P, T, C, D, D)
    want = np.array([[np.real(np.vdot(g0[p], dh0p[p, t]) + np.vdot(gc[p], dcolp[p, t])) for t in range(T)] for p in range(P)])
    got = ml.model_param_grads(g0, gk, dh0p, grad_col_ops=gc, dcol_ops=dcolp)
    assert got.shape == (P, T) and np.abs(got - want).max() < 1e-13 * np.abs(want).max()
    assert np.array_equal(ml.model_param_grads(g0, gk, dh0), ml.model_param_grads(g0, gk, dh0, None, None, None))
    with pytest.raises(C3PropError, match="go together"):
        ml.model_param_grads(g0, gk, dh0, dcol_ops=dcol)


def test_thermal_initial_state():
    from c3_amd import model_learning as ml
    from c3_amd._lib import C3PropError

    D = 3
    freqs = 2 * np.pi * np.array([0.0, 5.0e9, 9.8e9])  # a transmon's levels, rad/s
    h0 = np.diag(freqs).astype(complex) + 0.1 * (np.ones((D, D)) - np.eye(D))  # only the diagonal is read
    vec0 = np.zeros(D * D, dtype=complex)
    vec0[0] = 1.0
    for arg in (h0, freqs):
        v = ml.thermal_initial_state(arg, 0.0)
        assert v.shape == (D * D,) and np.array_equal(v, vec0)
    ket = ml.thermal_initial_state(h0, 0.0, lindbladian=False)
    assert np.array_equal(ket, np.array([1, 0, 0], dtype=complex))
    T = 0.1  # K: kb T / hbar = 2 pi 2.08 GHz, a visible excited population
    w = np.exp(-1.054571817e-34 * (freqs - freqs[0]) / (1.380649e-23 * T))
    w = w / w.sum()
    assert 0.05 < w[1] < 0.2
    for arg in (h0, freqs):
        v = ml.thermal_initial_state(arg, T)
        assert v.shape == (D * D,) and v.dtype == np.complex128
        rho = v.reshape(D, D).T  # vec_to_dm
        assert np.abs(rho - np.diag(w)).max() < 1e-15
        assert abs(np.trace(rho) - 1) < 1e-15
    with pytest.raises(C3PropError, match="needs the Lindblad path"):
        ml.thermal_initial_state(h0, T, lindbladian=False)
