"""GPU checks of the model-operator cotangents of the Lindblad path at D = 7, 8, 9 (c3p_pwc_lindblad_model_vjp_hb: the Hermitian-basis
sweep of c3p_regrg.hip keeping the sums of the real generator cotangents, and regr_model_reduce_kernel) against the numpy
restatement of tests/lindblad_model_grad_fast_ref.py: 1e-10 max|want| per output array, the bar of the model-cotangent tests at
D <= 6.  grad_h0 / grad_hks are compared against the HERMITIAN PART of the reference (a real generator only sees Hermitian
perturbations of H), grad_col_ops against the reference as it is.  Inputs as _lind_case of tests/test_gpu_round4.py."""
import functools

import numpy as np
import pytest

import lindblad_model_grad_fast_ref as fast
from c3_amd import _lib
from oracle import c3_oracle as o

pytestmark = pytest.mark.gpu
TOL = 1e-10
NAMES = ("grad_h0", "grad_hks", "grad_col_ops")


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import _lib, propagation

    _lib.require_gpu()
    return propagation


def _lind_case(D, B, K, N, C, seed, per_sample=False, hscale=0.8, cscale=0.25):
    """tests/test_gpu_round4.py::_lind_case: Hermitian h0 / hks, complex non-Hermitian col_ops, random U_bar, row phases"""
    rng = np.random.default_rng(seed)
    herm = lambda s: (lambda a: s * (a + a.conj().T) / 2)(rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D)))
    nb = B if per_sample else 1
    h0 = np.stack([herm(hscale) for _ in range(nb)])
    hks = np.stack([np.stack([herm(0.5 * hscale / 0.8) for _ in range(K)]) for _ in range(nb)])
    if not per_sample:
        h0, hks = h0[0], hks[0]
    col = np.stack([cscale * (rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))) for _ in range(C)])
    sig = rng.uniform(-1, 1, size=(B, K, N))
    Dm = D * D
    Ubar = rng.normal(size=(B, Dm, Dm)) + 1j * rng.normal(size=(B, Dm, Dm))
    ph = rng.uniform(0, 2 * np.pi, size=(B, Dm))
    return h0, hks, col, sig, Ubar, ph


def _want(h0, hks, col, sig, Ubar, ph, dt, per_sample, samples):
    """reference cotangents of the listed samples, stacked: (Hermitian part of grad_h0, of grad_hks, grad_col_ops)"""
    r = [fast.lindblad_model_cotangents(h0[b] if per_sample else h0, hks[b] if per_sample else hks, col, sig[b], dt, Ubar[b],
                                        None if ph is None else ph[b]) for b in samples]
    g0, gk, gc = (np.stack([x[i] for x in r]) for i in range(3))
    return fast.hermitian_part(g0), fast.hermitian_part(gk), gc


def _close(got, want, what, tol=TOL):
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    print(f"{what}: max|got - want| = {err:.3e}, max|want| = {np.abs(want).max():.3e}")
    assert err < tol * np.abs(want).max(), (what, err, np.abs(want).max())


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _hb(prop, h0, hks, sig, dt, col, Ubar, ph):
    return prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph, want_model_grads=True, hermitian_basis=True)


# D, N, B, K, C, per_sample, segments, dt: the shapes of test_lindblad_vjp_hermitian_basis_sweep
CLASSES = [
    (9, 9, 2, 2, 2, False, None, 0.1),   # one segment per sample, no squarings at the highest degree; border row and column hold data
    (9, 17, 3, 2, 1, True, 4, 0.3),      # several segments (partials added in the reduce kernel), per-sample operators, squarings
    (8, 12, 2, 3, 2, False, 3, 0.25),    # 64 x 64 in the zero-padded 65 class
    (7, 16, 2, 1, 1, True, 2, 0.3),      # 49 x 49
]


@functools.lru_cache(maxsize=None)
def _class_case(D, N, B, K, C, per_sample, segments, dt):
    inp = _lind_case(D, B, K, N, C, 1000 + 10 * D + N, per_sample)
    return inp, _want(*inp, dt, per_sample, range(B))


@pytest.mark.parametrize("D,N,B,K,C,per_sample,segments,dt", CLASSES)
def test_every_class_and_the_scan(prop, D, N, B, K, C, per_sample, segments, dt):
    """all three operator cotangents of every sample against the reference; the launch is the matrix-core sweep; grad_signals
    bitwise what propagate_batch_lindblad_vjp returns under the same options; a second call returns the same bits"""
    (h0, hks, col, sig, Ubar, ph), want = _class_case(D, N, B, K, C, per_sample, segments, dt)
    with _lib.options(segments=segments):
        out = _hb(prop, h0, hks, sig, dt, col, Ubar, ph)
        assert _lib.last_kernel() == "mfma"
        gs = prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph)
        assert _lib.last_kernel() == "mfma"
        again = _hb(prop, h0, hks, sig, dt, col, Ubar, ph)
    for got, w, what in zip(out[1:], want, NAMES):
        _close(got, w, what)
    assert _bits(out[0], gs)
    for a, b in zip(out, again):
        assert _bits(a, b)


@pytest.mark.parametrize("D,B,N,segments", [
    (7, 2, 75, 1),    # one chain of 75 slices crosses two 32-slice staging boundaries of the control amplitudes
    (7, 40, 16, 8),   # 320 chains on 256 workgroups: a workgroup sweeps a second chain (the sums are per chain)
])
def test_signal_chunks_and_workgroup_reuse(prop, D, B, N, segments):
    """the inputs of test_lindblad_vjp_hermitian_basis_long_chains_and_many_chains; the reference on the first and last sample"""
    h0, hks, col, sig, Ubar, ph = _lind_case(D, B, 2, N, 1, 31 * D + N, per_sample=False)
    with _lib.options(segments=segments):
        out = _hb(prop, h0, hks, sig, 0.15, col, Ubar, ph)
    assert _lib.last_kernel() == "mfma"
    want = _want(h0, hks, col, sig, Ubar, ph, 0.15, False, (0, B - 1))
    for got, w, what in zip(out[1:], want, NAMES):
        _close(np.asarray(got)[[0, B - 1]], w, what)


def _two_qutrit_col(s0=0.8, s1=0.5):
    a = np.kron(np.diag(np.sqrt(np.arange(1, 3)), 1), np.eye(3))
    return np.stack([s0 * a, s1 * np.kron(np.eye(3), np.diag(np.arange(3.0)))]).astype(complex)


def test_strong_dissipation(prop):
    """the two-qutrit operators of test_lindblad_vjp_hermitian_basis_strong_dissipation_and_long_chain: 70 slices in 5 ragged
    segments, squarings in the pair evaluation, a dissipator with a large trace; the reference on one sample"""
    D, B, K, N = 9, 2, 2, 70
    rng = np.random.default_rng(3)
    herm = lambda s: (lambda a: s * (a + a.conj().T) / 2)(rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D)))
    h0, hks = herm(1.0), np.stack([herm(0.5) for _ in range(K)])
    col = _two_qutrit_col()
    sig = rng.uniform(-1, 1, size=(B, K, N))
    Ubar = rng.normal(size=(B, 81, 81)) + 1j * rng.normal(size=(B, 81, 81))
    with _lib.options(segments=5):
        out = _hb(prop, h0, hks, sig, 0.25, col, Ubar, None)
    want = _want(h0, hks, col, sig, Ubar, None, 0.25, False, (1,))
    for got, w, what in zip(out[1:], want, NAMES):
        _close(np.asarray(got)[1:], w, what)


def test_degrees_and_chunks(prop):
    """every Taylor degree of the pair evaluation gives the default's cotangents to 2e-11 max; with the segment count fixed, sample
    chunks of two give bitwise the unchunked result in every output"""
    D, B, K, N = 9, 5, 2, 11
    h0, hks, col, sig, Ubar, ph = _lind_case(D, B, K, N, 1, 77, per_sample=True)
    ref = [np.asarray(a) for a in _hb(prop, h0, hks, sig, 0.2, col, Ubar, ph)]
    for deg in (8, 12, 16, 20):
        with _lib.options(regr_grad_degree=deg):
            g = _hb(prop, h0, hks, sig, 0.2, col, Ubar, ph)
        for a, r, what in zip(g, ref, ("grad_signals",) + NAMES):
            _close(a, r, f"degree {deg} {what}", 2e-11)
    with _lib.options(segments=3):
        one = _hb(prop, h0, hks, sig, 0.2, col, Ubar, ph)
    with _lib.options(segments=3, grad_chunk=2):
        many = _hb(prop, h0, hks, sig, 0.2, col, Ubar, ph)
    for a, b in zip(one, many):
        assert _bits(a, b)


def test_cross_check_against_the_general_sweep_at_d6(prop):
    """D = 6 zero padded in the 49 class (regr_grad_d6 = 1): the new entry against the Hermitian part (grad_h0, grad_hks) and the
    whole (grad_col_ops) of c3p_pwc_lindblad_model_vjp's results, GPU against GPU"""
    D, B, K, N = 6, 2, 2, 9
    h0, hks, col, sig, Ubar, ph = _lind_case(D, B, K, N, 2, 606, per_sample=True)
    old = prop.propagate_batch_lindblad_vjp(h0, hks, sig, 0.3, col, Ubar, fr_phase=ph, want_model_grads=True)
    with _lib.options(regr_grad_d6=1):
        new = _hb(prop, h0, hks, sig, 0.3, col, Ubar, ph)
        assert _lib.last_kernel() == "mfma"
    _close(new[1], fast.hermitian_part(old[1]), "grad_h0")
    _close(new[2], fast.hermitian_part(old[2]), "grad_hks")
    _close(new[3], np.asarray(old[3]), "grad_col_ops")
    _close(new[0], np.asarray(old[0]), "grad_signals")


def test_device_tensors_match_host_arrays(prop):
    """device-resident inputs (no staging) return what the host-pointer call returns, bit for bit"""
    import torch

    D, N, B, K, C, per_sample, segments, dt = CLASSES[1]
    (h0, hks, col, sig, Ubar, ph), _ = _class_case(*CLASSES[1])
    t = lambda a: torch.as_tensor(a, device="cuda:0")
    with _lib.options(segments=segments):
        host = _hb(prop, h0, hks, sig, dt, col, Ubar, ph)
        dev = _hb(prop, t(h0), t(hks), t(sig), dt, t(col), t(Ubar), t(ph))
    for a, b in zip(host, dev):
        assert _bits(a, b.cpu().numpy())


def test_refusals(prop):
    from c3_amd._lib import C3PropError

    h0, hks, col, sig, Ubar, ph = _lind_case(9, 1, 2, 4, 1, 9)
    with pytest.raises(C3PropError, match="Hermitian"):
        _hb(prop, h0 - 0.05j * np.diag(np.arange(9)), hks, sig, 0.2, col, Ubar, ph)
    with pytest.raises(C3PropError, match="hermitian_basis"):
        prop.propagate_batch_lindblad_vjp(h0, hks, sig, 0.2, col, Ubar, fr_phase=ph, hermitian_basis=True)
    h0, hks, col, sig, Ubar, ph = _lind_case(10, 1, 1, 2, 1, 10)
    with pytest.raises(C3PropError, match="C3:Error"):
        _hb(prop, h0, hks, sig, 0.2, col, Ubar, ph)
    h0, hks, col, sig, Ubar, ph = _lind_case(5, 1, 1, 2, 1, 5)
    with pytest.raises(C3PropError, match=r"c3p_pwc_lindblad_model_vjp\b"):
        _hb(prop, h0, hks, sig, 0.2, col, Ubar, ph)


# ---- open-system model learning at D = 9 ----


@functools.lru_cache(maxsize=None)
def _learning_problem():
    from c3_amd import model_learning as ml

    rng = np.random.default_rng(19)
    D, P, K, N, dt = 9, 2, 2, 12, 0.25
    herm = lambda s: (lambda a: s * (a + a.conj().T) / 2)(rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D)))
    levels = np.add.outer(np.array([0.0, 1.0, 1.8]), np.array([0.0, 1.3, 2.4])).reshape(-1)
    h0 = herm(0.3) + np.diag(levels)
    hks = np.stack([herm(0.5) for _ in range(K)])
    col = _two_qutrit_col(0.2, 0.125)  # the collapse operators of test_strong_dissipation, scaled down
    sigs = {"rx90p": rng.uniform(-1, 1, size=(P, K, N)), "ry90p": rng.uniform(-1, 1, size=(P, K, N))}
    seqs = [[], ["rx90p"], ["ry90p", "rx90p", "rx90p"]]
    # kb T / hbar of the order of the level spacings given to the initial state: a visibly mixed rho0
    rho0 = ml.thermal_initial_state(2 * np.pi * 5.0e9 * levels, 0.15)
    return dict(D=D, P=P, K=K, N=N, dt=dt, h0=h0, hks=hks, col=col, sigs=sigs, seqs=seqs, rho0=rho0, labels=[0])


_PROPS = {}


def _cpu_goal(q, h0, hks, col, sigs, data_sets=None):
    """_cpu_goal of tests/test_gpu_lindblad_model_grad.py, the numpy restatement on the oracle: (goal, goals [P], sim_vals [P,S]).
    The oracle's propagator of a (parameter set, gate) is kept per input: a finite difference in one pulse sample recomputes one
    propagator, not all of them (0.3 s each at D = 9)."""
    from c3_amd import model_learning as ml

    def U(s):
        key = (h0.tobytes(), hks.tobytes(), col.tobytes(), s.tobytes())
        if key not in _PROPS:
            _PROPS[key] = o.propagate_batch(h0, hks, s, q["dt"], col_ops=col, lindbladian=True)[0]
        return _PROPS[key]

    sim = np.zeros((q["P"], len(q["seqs"])))
    for p in range(q["P"]):
        Us = {g: U(np.ascontiguousarray(s[p : p + 1])) for g, s in sigs.items()}
        for si, S in enumerate(o.evaluate_sequences(Us, q["seqs"])):
            sim[p, si] = o.populations(S @ q["rho0"], True)[q["labels"]].sum()
    if data_sets is None:
        return None, None, sim
    goals = np.array([ml.g_LL_prime(d["results"], sim[p], d["results_std"], d["shots"]) for p, d in enumerate(data_sets)])
    return ml.g_LL_prime_combined(goals, [len(q["seqs"])] * q["P"]), goals, sim


@functools.lru_cache(maxsize=None)
def _learning_data():
    q = _learning_problem()
    sim = _cpu_goal(q, q["h0"], q["hks"], q["col"], q["sigs"])[2]
    S = len(q["seqs"])
    off = np.array([[0.02, -0.015, 0.01], [-0.01, 0.02, -0.02]])
    return tuple({"seqs": q["seqs"], "results": sim[p] + off[p], "results_std": np.full(S, 0.01), "shots": np.full(S, 1000.0)} for p in range(q["P"]))


def test_open_system_goal_gradient_two_qutrits(prop):
    """model_param_grads for a scale on col_ops, a shift of h0[1,1] and a scale on hks[0], and three entries of one gate's
    grad_signals, against central differences of the numpy restatement on the oracle: 1e-6 max|fd|, the shape and bar of
    test_open_system_goal_gradient"""
    from c3_amd import model_learning as ml

    q, ds = _learning_problem(), list(_learning_data())
    D, K, P = q["D"], q["K"], q["P"]
    rho = q["rho0"].reshape(D, D)
    assert 0.02 < 1 - np.real(rho[0, 0]) < 0.9  # visibly mixed
    r = ml.goal_run_batched_with_grad(q["h0"], q["hks"], q["sigs"], q["dt"], ds, q["rho0"], q["labels"], col_ops=q["col"])
    assert _lib.last_kernel() == "mfma"
    assert np.asarray(r["grad_col_ops"]).shape == (P, 2, D, D)
    assert np.asarray(r["grad_h0"]).shape == (P, D, D) and np.asarray(r["grad_hks"]).shape == (P, K, D, D)
    e11 = np.zeros((D, D), dtype=complex)
    e11[1, 1] = 1.0
    zero = lambda a: np.zeros_like(a)
    k0 = zero(q["hks"])
    k0[0] = q["hks"][0]
    dh0 = np.stack([zero(q["h0"]), e11, zero(q["h0"])])
    dhks = np.stack([zero(q["hks"]), zero(q["hks"]), k0])
    dcol = np.stack([q["col"], zero(q["col"]), zero(q["col"])])
    got = ml.model_param_grads(r["grad_h0"], r["grad_hks"], dh0, dhks, r["grad_col_ops"], dcol)
    at = lambda th, sigs=q["sigs"]: _cpu_goal(q, q["h0"] + th[1] * e11, q["hks"] + th[2] * k0, (1 + th[0]) * q["col"], sigs, ds)[0]
    eps = 1e-5
    fd = np.array([(at(eps * np.eye(3)[t]) - at(-eps * np.eye(3)[t])) / (2 * eps) for t in range(3)])
    print("model_param_grads", got, "finite differences", fd)
    assert np.abs(fd).min() > 1e-3 * np.abs(fd).max()  # every parameter matters
    assert np.abs(got - fd).max() < 1e-6 * np.abs(fd).max()
    gs = np.asarray(r["grad_signals"]["ry90p"])
    assert gs.shape == (P, K, q["N"])
    for p, k, n in ((0, 0, 0), (1, 1, 7), (1, 0, 11)):
        vals = []
        for sgn in (+1, -1):
            s = {g: v.copy() for g, v in q["sigs"].items()}
            s["ry90p"][p, k, n] += sgn * eps
            vals.append(at(np.zeros(3), s))
        fdv = (vals[0] - vals[1]) / (2 * eps)
        print("grad_signals", (p, k, n), gs[p, k, n], fdv)
        assert abs(gs[p, k, n] - fdv) < 1e-6 * np.abs(gs).max()
