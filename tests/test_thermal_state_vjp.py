"""model_learning.thermal_initial_state_vjp against central differences of thermal_initial_state (host numpy, no GPU).

The scalar differentiated is L = Re sum conj(rho0_bar) vec(rho0) for a random complex cotangent rho0_bar.  Central differences with
a relative step h = 1e-5: truncation O(h^2) ~ 1e-10, rounding eps / h ~ 1e-11 (both relative to the derivative's scale), so the bar
of 1e-7 of the largest derivative sits far above both."""
import numpy as np
import pytest

from c3_amd import model_learning as ml

BAR = 1e-7
H = 1e-5


def _energies(D):
    """a weakly anharmonic ladder: a few GHz * 2 pi between neighbours, E_0 not zero (the state depends on differences only)"""
    n = np.arange(D)
    return 2 * np.pi * (1.0e9 + 4.9e9 * n - 0.12e9 * n * (n - 1))


def _scalar(bar, diag, T):
    return float(np.sum(np.conj(bar) * ml.thermal_initial_state(diag, T)).real)


@pytest.mark.parametrize("D", [3, 9])
@pytest.mark.parametrize("T", [0.05, 0.3])
def test_thermal_state_vjp_matches_central_differences(D, T):
    rng = np.random.default_rng(10 * D + int(1000 * T))
    diag = _energies(D)
    bar = rng.normal(size=D * D) + 1j * rng.normal(size=D * D)
    g_T, g_E = ml.thermal_initial_state_vjp(diag, T, bar)
    assert np.shape(g_E) == (D,) and np.isrealobj(g_E)
    fd_T = (_scalar(bar, diag, T * (1 + H)) - _scalar(bar, diag, T * (1 - H))) / (2 * T * H)
    print(f"D={D} T={T}: d/dT {g_T:.9e} fd {fd_T:.9e} rel err {abs(g_T - fd_T) / abs(fd_T):.2e}")
    assert abs(fd_T) > 0
    assert abs(g_T - fd_T) <= BAR * abs(fd_T)
    fd_E = np.zeros(D)
    for k in range(D):
        e = np.zeros(D)
        e[k] = H * diag[k]
        fd_E[k] = (_scalar(bar, diag + e, T) - _scalar(bar, diag - e, T)) / (2 * e[k])
    err = np.abs(g_E - fd_E).max()
    print(f"D={D} T={T}: d/dE max err {err:.2e} of max|fd| {np.abs(fd_E).max():.2e}")
    assert np.abs(fd_E).max() > 0
    assert err <= BAR * np.abs(fd_E).max()
    # a matrix is read by its diagonal, as thermal_initial_state reads it
    g_T2, g_E2 = ml.thermal_initial_state_vjp(np.diag(diag) + 0.1 * (np.ones((D, D)) - np.eye(D)), T, bar)
    assert g_T2 == g_T and np.array_equal(g_E2, g_E)


@pytest.mark.parametrize("D", [3, 9])
def test_zero_temperature_has_zero_derivative(D):
    bar = np.arange(D * D) + 1j
    g_T, g_E = ml.thermal_initial_state_vjp(_energies(D), 0.0, bar)
    assert g_T == 0.0 and np.array_equal(g_E, np.zeros(D))


@pytest.mark.parametrize("D", [3, 9])
@pytest.mark.parametrize("T", [0.05, 0.3])
def test_weights_sum_to_one(D, T):
    rho = ml.thermal_initial_state(_energies(D), T)
    w = rho[:: D + 1]
    assert abs(np.sum(w) - 1.0) <= 1e-15
    # the cotangent of the trace gives no derivative: sum_i w_i = 1 for every T and every energy
    ones = np.zeros(D * D)
    ones[:: D + 1] = 1.0
    g_T, g_E = ml.thermal_initial_state_vjp(_energies(D), T, ones)
    # (rounding of a D-term sum whose terms w_i a_i stay below ~40: D eps 40 < 1e-13)
    assert abs(g_T) <= 1e-13 / T and np.abs(g_E).max() <= 1e-13 * ml.HBAR / (ml.KB * T)


def test_wrong_cotangent_size_is_an_error():
    with pytest.raises(ml.C3PropError, match="rho0_bar"):
        ml.thermal_initial_state_vjp(_energies(3), 0.1, np.zeros(3))
