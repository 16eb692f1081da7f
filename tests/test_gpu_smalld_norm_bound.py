"""The column-wise norm bound of the small-D chain kernels (c3p_smalld.hip: c3p_sd_segment_norm) on problems where it decides
differently from the sum of norms it replaced: the degree-6 pair instead of the degree-8 pair (radius 0.83), no squaring instead of
one (radius 1.85) -- against the CPU oracle at the tolerance of tests/test_gpu_parity.py.  The bounds of every case are asserted
on the CPU first (tests/norm_bound_model.py); all control amplitudes have constant magnitude per channel, so the bounds are the same
for every segment however the time axis is split."""
import numpy as np
import pytest

from norm_bound_model import MM6_THETA, MM8_THETA, bounds, column_sums, segments
from oracle import c3_oracle as o

pytestmark = pytest.mark.gpu

TOL = 1e-10  # tests/test_gpu_parity.py: |U_gpu - U_ref|_F < 1e-10 per sample
S, N, B = 32, 131, 3  # eight waves of four chains: the workgroup-per-sample kernel; N = 131: unequal segments in a wave
MW = "c3p_smalld.hip: smalld_chain_kernel<%d, false, false, false, true, "


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


def star(rng, D, j, weight, imag=False):
    """a Hermitian operator with zero diagonal whose column j (and row j) carries `weight`, the rest 5 % noise: its widest column is j"""
    m = 0.05 * rng.uniform(0.2, 1.0, size=(D, D))
    if imag:
        m = m * np.exp(1j * rng.uniform(0, 6.28, size=(D, D)))
    m = np.triu(m, 1)
    m = m + m.conj().T
    m[:, j] = m[j, :] = 0.0
    col = weight * rng.uniform(0.5, 1.0, size=D) * (np.exp(1j * rng.uniform(0, 6.28, size=D)) if imag else 1.0)
    col[j] = 0.0
    m[:, j] += col
    m[j, :] += col.conj()
    return m.astype(np.complex128)


def straddling(rng, D, K, theta, imag=False, diag=True):
    """operators whose widest columns are columns 0 .. K (one each), amplitudes +-a_k; dt such that the sum of norms is
    >= 1.02 theta and the column-wise bound <= 0.98 theta on every segment"""
    h0 = star(rng, D, 0, 1.0) + (np.diag(rng.uniform(-0.3, 0.3, D)) if diag else 0.0)
    hks = np.stack([star(rng, D, k + 1, 1.0, imag and k == 0) for k in range(K)])
    amp = rng.uniform(0.7, 1.0, size=(1, K, 1))
    sig = amp * rng.choice([-1.0, 1.0], size=(B, K, N))
    cs = column_sums(h0, hks, 1.0)
    assert sorted(cs.argmax(axis=1)) == list(range(K + 1))  # the widest columns sit in different columns
    _, col, son = bounds(h0, hks, sig[0], 1.0, 0, N)
    dt = theta / np.sqrt(col * son)
    return h0, hks, sig, dt


def check_straddle(h0, hks, sig, dt, theta):
    for b in range(B):
        for n0, n1 in segments(N, S):
            exact, col, son = bounds(h0, hks, sig[b], dt, n0, n1)
            # (exact and column-wise are summed in different orders: equal ones may differ in the last bit)
            assert son >= 1.02 * theta and exact <= col * (1 + 1e-14) and col <= 0.98 * theta, (b, n0, exact, col, son, theta)


def run(prop, D, h0, hks, sig, dt, ph=None, **opts):
    from c3_amd import _lib

    with _lib.options(smalld_segments=S, **opts):
        U = np.asarray(prop.propagate_batch(h0, hks, sig, dt, fr_phase=ph)["U"])
    assert (MW % D) in _lib.last_kernel_detail(), _lib.last_kernel_detail()
    ref = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    err = max(np.linalg.norm(U[b] - ref[b]) for b in range(U.shape[0]))
    print(f"D={D} K={sig.shape[1]} max_b |U - U_ref|_F = {err:.3e}")
    return err, U


def test_a_wave_runs_a_masked_last_slot():
    lens = [n1 - n0 for n0, n1 in segments(N, S)]
    assert any(min(lens[4 * w : 4 * w + 4]) < max(lens[4 * w : 4 * w + 4]) for w in range(S // 4))


@pytest.mark.parametrize("theta", [MM6_THETA, MM8_THETA])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("D", [5, 9, 4, 12])  # core + border loop (5, 9), padded loop (4, 12)
def test_straddling_a_threshold(prop, D, K, theta):
    """sum of norms >= 1.02 theta, column-wise bound <= 0.98 theta: the kernel takes the cheaper evaluation and stays exact"""
    rng = np.random.default_rng(9300 + 100 * D + 10 * K + int(theta > 1))
    h0, hks, sig, dt = straddling(rng, D, K, theta)
    check_straddle(h0, hks, sig, dt, theta)
    ph = rng.uniform(0, 6.28, size=(B, D)) if K == 2 else None  # frame phases on and off
    assert run(prop, D, h0, hks, sig, dt, ph)[0] < TOL


@pytest.mark.parametrize("theta", [MM6_THETA, MM8_THETA])
@pytest.mark.parametrize("D", [5, 9, 4, 12])
def test_no_slack(prop, D, theta):
    """entrywise non-negative tables with the same widest column, positive constant amplitudes: the column-wise bound IS the norm
    of every slice, set to 0.999 theta -- a column sum that came out too small would put the slices beyond the radius"""
    rng = np.random.default_rng(9400 + 10 * D + int(theta > 1))
    K = 2
    h0 = star(rng, D, 1, 1.0)
    hks = np.stack([star(rng, D, 1, 1.0) for _ in range(K)])
    sig = np.broadcast_to(rng.uniform(0.7, 1.0, size=(1, K, 1)), (B, K, N)).copy()
    exact, col, _ = bounds(h0, hks, sig[0], 1.0, 0, N)
    assert abs(exact - col) <= 1e-14 * col and (column_sums(h0, hks, 1.0).argmax(axis=1) == 1).all()
    dt = 0.999 * theta / col
    assert run(prop, D, h0, hks, sig, dt)[0] < TOL


@pytest.mark.parametrize("D", [9, 12])
def test_drift_alone(prop, D):
    """K = 0: the bound is the 1-norm of the drift table"""
    rng = np.random.default_rng(9500 + D)
    h0 = star(rng, D, 2, 1.0) + np.diag(rng.uniform(-0.3, 0.3, D))
    hks, sig = np.zeros((0, D, D), complex), np.zeros((B, 0, N))
    dt = 0.999 * MM6_THETA / bounds(h0, hks, sig[0], 1.0, 0, N)[1]
    assert run(prop, D, h0, hks, sig, dt)[0] < TOL


def test_complex_hermitian_operator(prop):
    """one control complex Hermitian: the complex loop of the same launch takes its plan from the same bound"""
    rng = np.random.default_rng(9600)
    h0, hks, sig, dt = straddling(rng, 9, 2, MM6_THETA, imag=True)
    assert np.abs(hks[0].imag).max() > 0.1
    check_straddle(h0, hks, sig, dt, MM6_THETA)
    assert run(prop, 9, h0, hks, sig, dt)[0] < TOL


def test_one_qutrit_lindblad_prep_kernel_tables(prop):
    """Dm = 9 superoperators of one qutrit: the tables come from the prep kernel, their column sums are formed in the chain kernel"""
    from c3_amd import _lib, workloads

    wl = workloads.make_workload(1, B=B, N=N)
    col = workloads.qubit_collapse_op(workloads.annihilator(3).astype(complex), 27e-6, 39e-6)[None]
    with _lib.options(smalld_segments=S, no_smallr=1):
        U = np.asarray(prop.propagate_batch(wl.h0, wl.hks, wl.signals, wl.dt, col_ops=col, lindbladian=True)["U"])
    detail = _lib.last_kernel_detail()
    assert "smalld_prep_kernel<9>" in detail and "smalld_chain_kernel<9," in detail, detail
    ref = o.propagate_batch(wl.h0, wl.hks, wl.signals, wl.dt, col_ops=col, lindbladian=True)
    assert max(np.linalg.norm(U[b] - ref[b]) for b in range(B)) < TOL


@pytest.mark.parametrize("traceless", [True, False])
def test_prep_kernel_tables_against_tables_built_in_the_kernel(prop, traceless):
    """the same column sums from either source of the tables, so the same plan.  With traceless operators the two modes form the
    same tables and U is bit for bit the same.  With a trace the tables themselves differ in their last bits (the trace is summed
    across the wave in one mode and in sequence in the other; so it was before the column-wise bound, measured 5e-16 on this
    problem): there U agrees to 1e-13."""
    rng = np.random.default_rng(9700)
    h0, hks, sig, dt = straddling(rng, 9, 2, MM6_THETA, diag=not traceless)
    check_straddle(h0, hks, sig, dt, MM6_THETA)
    e0, U0 = run(prop, 9, h0, hks, sig, dt)
    e1, U1 = run(prop, 9, h0, hks, sig, dt, prep_kernel=1)
    assert e0 < TOL and e1 < TOL
    d = np.abs(U0 - U1).max()
    print(f"max |U(prep kernel) - U(inline)| = {d:.3e}")
    assert np.array_equal(U0, U1) if traceless else d < 1e-13


def test_goal_gradient_on_a_straddling_problem(prop):
    """propagate_batch_goal_vjp at D = 9, K = 2: forward segments and the real backward sweep decide on the same column-wise bound;
    against the oracle's gradient at the tolerance of tests/test_gradient.py (1e-10 of the largest entry)"""
    from c3_amd import _lib, fidelities as fid

    rng = np.random.default_rng(9800)
    D, K, index, dims = 9, 2, [0, 1], [3, 3]
    h0, hks, sig, dt = straddling(rng, D, K, MM6_THETA)
    check_straddle(h0, hks, sig, dt, MM6_THETA)
    ph = rng.uniform(0, 6, size=(B, D))
    q, _ = np.linalg.qr(rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4)))
    r = prop.propagate_batch_goal_vjp(h0, hks, sig, dt, q, index, dims, fr_phase=ph)
    assert "smalld_grad_real_kernel<9>" in _lib.last_kernel_detail(), _lib.last_kernel_detail()
    ref_U = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    Ubar, goal = fid.unitary_infid_cotangent(q, ref_U, index, dims)
    g = np.asarray(r["grad_signals"])
    for b in range(B):
        assert abs(float(r["goal"][b]) - o.unitary_infid(q, ref_U[b], index=index, dims=dims)) < 1e-11
        want = o.pwc_signal_gradient(h0, hks, sig[b], dt, np.asarray(Ubar)[b], ph[b])
        assert np.abs(g[b] - want).max() < 1e-10 * np.abs(want).max()
