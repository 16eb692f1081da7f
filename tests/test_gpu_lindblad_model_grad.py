"""GPU checks of the model-operator cotangents of the Lindblad path (c3p_pwc_lindblad_model_vjp: c3p_grad.hip, the accumulating
general-generator sweep and the reduce kernel) against the numpy restatement of tests/lindblad_model_grad_ref.py (bar 1e-10
max|want| per output array, the bar of the Lindblad vjp tests in tests/test_gradient.py), and of open-system model learning
(model_learning.goal_run_batched[_with_grad] with col_ops) against finite differences of a numpy restatement on the oracle."""
import functools

import numpy as np
import pytest

import lindblad_model_grad_ref as ref
from c3_amd import _lib
from oracle import c3_oracle as o

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import _lib, propagation

    _lib.require_gpu()
    return propagation


def _inputs(D, N, B, C, per_sample, seed, col_scale=0.25, K=2):
    """the inputs of tests/test_gradient.py::test_lindblad_vjp_small_superoperators_general_sweep: Hermitian h0 / hks, complex
    non-Hermitian col_ops, random U_bar, row phases"""
    rng = np.random.default_rng(seed)
    herm = lambda s: (lambda a: s * (a + a.conj().T) / 2)(rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D)))
    nb = B if per_sample else 1
    h0 = np.stack([herm(0.8) for _ in range(nb)])
    hks = np.stack([np.stack([herm(0.5) for _ in range(K)]) for _ in range(nb)])
    if not per_sample:
        h0, hks = h0[0], hks[0]
    col = np.stack([col_scale * (rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))) for _ in range(C)])
    sig = rng.uniform(-1, 1, size=(B, K, N))
    Dm = D * D
    Ubar = rng.normal(size=(B, Dm, Dm)) + 1j * rng.normal(size=(B, Dm, Dm))
    ph = rng.uniform(0, 2 * np.pi, size=(B, Dm))
    return h0, hks, sig, col, Ubar, ph


def _want(h0, hks, sig, dt, col, Ubar, ph, per_sample, samples=None):
    """reference cotangents stacked over the samples (or the listed ones)"""
    bs = range(sig.shape[0]) if samples is None else samples
    r = [ref.lindblad_model_cotangents(h0[b] if per_sample else h0, hks[b] if per_sample else hks, col, sig[b], dt, Ubar[b], ph[b]) for b in bs]
    return tuple(np.stack([x[i] for x in r]) for i in range(3))


CASES = [(2, 7, 3, 1, False), (3, 17, 2, 2, True), (4, 40, 2, 1, False), (5, 17, 2, 2, False), (6, 9, 2, 1, True)]


@functools.lru_cache(maxsize=None)
def _case(D, N, B, C, per_sample):
    inp = _inputs(D, N, B, C, per_sample, 100 * D + N)
    h0, hks, sig, col, Ubar, ph = inp
    return inp, _want(h0, hks, sig, 0.3, col, Ubar, ph, per_sample)


def _close(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    print(f"{what}: max|got - want| = {err:.3e}, max|want| = {np.abs(want).max():.3e}")
    assert err < TOL * np.abs(want).max(), (what, err, np.abs(want).max())


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("D,N,B,C,per_sample", CASES)
def test_model_vjp_vs_reference(prop, D, N, B, C, per_sample):
    """One segment with fewer matrix elements than threads (D = 2), two uneven segments and odd D^2 (D = 3, per-sample
    operators), several segments in LDS (D = 4), the global-scratch variant (D = 5, 6): grad_h0, grad_hks, grad_col_ops against
    the exact directional derivatives of the reference; grad_signals bitwise equal to c3p_pwc_lindblad_vjp on the VALU sweep (the
    same arithmetic); a second call returns the same bits in every output."""
    (h0, hks, sig, col, Ubar, ph), want = _case(D, N, B, C, per_sample)
    dt = 0.3
    out = prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph, want_model_grads=True)
    assert _lib.last_kernel() == ("generic_lds" if D <= 4 else "generic_global")
    for got, w, what in zip(out[1:], want, ("grad_h0", "grad_hks", "grad_col_ops")):
        _close(got, w, what)
    _lib.set_option("valu_grad", "1")
    try:
        gv = prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph)
        assert _lib.last_kernel() == ("generic_lds" if D <= 4 else "generic_global")
    finally:
        _lib.set_option("valu_grad", None)
    assert _bits(out[0], gv)
    again = prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph, want_model_grads=True)
    for a, b in zip(out, again):
        assert _bits(a, b)


def test_model_vjp_device_tensors_match_host_arrays(prop):
    """device-resident inputs (no staging) return what the host-pointer call returns, bit for bit"""
    import torch

    (h0, hks, sig, col, Ubar, ph), _ = _case(*CASES[1])
    host = prop.propagate_batch_lindblad_vjp(h0, hks, sig, 0.3, col, Ubar, fr_phase=ph, want_model_grads=True)
    t = lambda a: torch.as_tensor(a, device="cuda:0")
    dev = prop.propagate_batch_lindblad_vjp(t(h0), t(hks), t(sig), 0.3, t(col), t(Ubar), fr_phase=t(ph), want_model_grads=True)
    for a, b in zip(host, dev):
        assert _bits(a, b.cpu().numpy())


def test_model_vjp_without_grad_signals(prop):
    """grad_signals = NULL is accepted (C ABI, host pointers); the operator cotangents are the same bits"""
    (h0, hks, sig, col, Ubar, ph), _ = _case(*CASES[0])
    D, N, B, C, _ps = CASES[0]
    K = sig.shape[1]
    full = prop.propagate_batch_lindblad_vjp(h0, hks, sig, 0.3, col, Ubar, fr_phase=ph, want_model_grads=True)
    c = lambda a: np.ascontiguousarray(a, dtype=np.complex128)
    h0c, hkc, colc, ubc = c(h0), c(hks), c(col), c(Ubar)
    g0, gk, gc = np.empty((B, D, D), complex), np.empty((B, K, D, D), complex), np.empty((B, C, D, D), complex)
    p = lambda a: a.ctypes.data
    rc = _lib.load().c3p_pwc_lindblad_model_vjp(p(h0c), 0, p(hkc), 0, p(sig), p(colc), C, 0.3, B, K, N, D, _lib.HOST_PTRS, p(ph), p(ubc),
                                                 None, p(g0), p(gk), p(gc), None)
    _lib.check(rc)
    for a, b in zip(full[1:], (g0, gk, gc)):
        assert _bits(a, b)


@pytest.mark.parametrize("D", [2, 4])
def test_model_vjp_sample_chunks(prop, D):
    """Five samples with per-sample operators in chunks of two (grad_chunk = 2): every output offset by the chunk, bitwise the
    one-chunk result; the last sample (a chunk of one) against the reference."""
    B, N = 5, 24
    h0, hks, sig, col, Ubar, ph = _inputs(D, N, B, 1, True, D)
    one = prop.propagate_batch_lindblad_vjp(h0, hks, sig, 0.3, col, Ubar, fr_phase=ph, want_model_grads=True)
    _lib.set_option("grad_chunk", "2")
    try:
        many = prop.propagate_batch_lindblad_vjp(h0, hks, sig, 0.3, col, Ubar, fr_phase=ph, want_model_grads=True)
    finally:
        _lib.set_option("grad_chunk", None)
    for a, b in zip(one, many):
        assert _bits(a, b)
    want = _want(h0, hks, sig, 0.3, col, Ubar, ph, True, samples=[4])
    for got, w, what in zip(many[1:], want, ("grad_h0", "grad_hks", "grad_col_ops")):
        _close(np.asarray(got)[4:], w, what)


def test_model_vjp_strong_dissipation(prop):
    """col_ops scaled to |clp|_1 dt = 3 (squarings in the pair evaluation, strongly contracting slices), D = 3, N = 12"""
    D, N, B, dt = 3, 12, 2, 0.3
    h0, hks, sig, col, Ubar, ph = _inputs(D, N, B, 1, False, 31)
    col = col * np.sqrt(3.0 / (np.linalg.norm(o.lindblad_dissipator(col), 1) * dt))
    assert abs(np.linalg.norm(o.lindblad_dissipator(col), 1) * dt - 3.0) < 1e-12
    out = prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph, want_model_grads=True)
    want = _want(h0, hks, sig, dt, col, Ubar, ph, False)
    for got, w, what in zip(out[1:], want, ("grad_h0", "grad_hks", "grad_col_ops")):
        _close(got, w, what)
    for b in range(B):
        ws = o.pwc_lindblad_signal_gradient(h0, hks, col, sig[b], dt, Ubar[b], ph[b])
        _close(out[0][b], ws, "grad_signals")


def test_model_vjp_refuses_d7(prop):
    from c3_amd._lib import C3PropError

    h0, hks, sig, col, Ubar, ph = _inputs(7, 2, 1, 1, False, 7)
    with pytest.raises(C3PropError, match=r"C3:Error.*D <= 6"):
        prop.propagate_batch_lindblad_vjp(h0, hks, sig, 0.3, col, Ubar, fr_phase=ph, want_model_grads=True)


# ---- open-system model learning ----


@functools.lru_cache(maxsize=None)
def _learning_problem():
    from c3_amd import model_learning as ml

    rng = np.random.default_rng(11)
    D, P, K, N, dt = 3, 2, 1, 20, 0.25
    herm = lambda s: (lambda a: s * (a + a.conj().T) / 2)(rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D)))
    h0 = herm(0.3) + np.diag([0.0, 1.0, 1.8])
    hks = np.stack([herm(0.5)])
    col = 0.2 * np.diag(np.sqrt(np.arange(1, D)), 1).astype(complex)[None] + 0.05 * (rng.normal(size=(1, D, D)) + 1j * rng.normal(size=(1, D, D)))
    sigs = {"rx90p": rng.uniform(-1, 1, size=(P, K, N)), "ry90p": rng.uniform(-1, 1, size=(P, K, N))}
    seqs = [[], ["rx90p"], ["ry90p", "rx90p", "rx90p"], ["rx90p", "ry90p", "ry90p", "rx90p", "ry90p"]]
    # kb T / hbar of the order of the level spacing given to the initial state: a visibly mixed rho0
    rho0 = ml.thermal_initial_state(2 * np.pi * np.array([0.0, 5.0e9, 9.8e9]), 0.15)
    return dict(D=D, P=P, K=K, N=N, dt=dt, h0=h0, hks=hks, col=col, sigs=sigs, seqs=seqs, rho0=rho0, labels=[0])


def _cpu_goal(q, h0, hks, col, sigs, data_sets=None):
    """numpy restatement on the oracle: (goal, goals [P], sim_vals [P,S])"""
    from c3_amd import model_learning as ml

    sim = np.zeros((q["P"], len(q["seqs"])))
    for p in range(q["P"]):
        Us = {g: o.propagate_batch(h0, hks, s[p : p + 1], q["dt"], col_ops=col, lindbladian=True)[0] for g, s in sigs.items()}
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
    off = np.array([[0.02, -0.015, 0.01, -0.02], [-0.01, 0.02, -0.02, 0.015]])
    return tuple({"seqs": q["seqs"], "results": sim[p] + off[p], "results_std": np.full(S, 0.01), "shots": np.full(S, 1000.0)} for p in range(q["P"]))


def test_open_system_goal_forward(prop):
    """goal, goals and sim_vals of both entry points (host arrays, and device tensors) equal the restatement on the oracle"""
    from c3_amd import model_learning as ml

    q, ds = _learning_problem(), list(_learning_data())
    goal, goals, sim = _cpu_goal(q, q["h0"], q["hks"], q["col"], q["sigs"], ds)
    assert 0.01 < sim.min() and sim.max() < 0.99
    for fn, dev in ((ml.goal_run_batched, None), (ml.goal_run_batched, "cuda:0"), (ml.goal_run_batched_with_grad, None)):
        r = fn(q["h0"], q["hks"], q["sigs"], q["dt"], ds, q["rho0"], q["labels"], col_ops=q["col"], device=dev)
        assert np.abs(r["sim_vals"] - sim).max() < 1e-10
        assert np.abs(r["goals"] - goals).max() < 1e-10 * max(1.0, np.abs(goals).max())
        assert abs(r["goal"] - goal) < 1e-10 * max(1.0, abs(goal))
    # a ket is taken as |psi><psi|
    ket = np.array([0.6, 0.8j, 0.0])
    r = ml.goal_run_batched(q["h0"], q["hks"], q["sigs"], q["dt"], ds, ket, q["labels"], col_ops=q["col"])
    rk = ml.goal_run_batched(q["h0"], q["hks"], q["sigs"], q["dt"], ds, np.outer(ket, ket.conj()).T.reshape(-1), q["labels"], col_ops=q["col"])
    assert np.array_equal(r["sim_vals"], rk["sim_vals"]) and abs(r["sim_vals"][0, 0] - 0.36) < 1e-14


def test_open_system_goal_gradient(prop):
    """model_param_grads for a scale on col_ops (a T1-like rate), a shift of h0[1,1] and a scale on hks[0], and three entries of
    one gate's grad_signals, against central differences of the numpy restatement: 1e-6 max|grad|"""
    from c3_amd import model_learning as ml

    q, ds = _learning_problem(), list(_learning_data())
    D, K = q["D"], q["K"]
    r = ml.goal_run_batched_with_grad(q["h0"], q["hks"], q["sigs"], q["dt"], ds, q["rho0"], q["labels"], col_ops=q["col"])
    assert np.asarray(r["grad_col_ops"]).shape == (q["P"], 1, D, D)
    assert np.asarray(r["grad_h0"]).shape == (q["P"], D, D) and np.asarray(r["grad_hks"]).shape == (q["P"], K, D, D)
    e11 = np.zeros((D, D), dtype=complex)
    e11[1, 1] = 1.0
    zero = lambda a: np.zeros_like(a)
    dh0 = np.stack([zero(q["h0"]), e11, zero(q["h0"])])
    dhks = np.stack([zero(q["hks"]), zero(q["hks"]), q["hks"]])
    dcol = np.stack([q["col"], zero(q["col"]), zero(q["col"])])
    got = ml.model_param_grads(r["grad_h0"], r["grad_hks"], dh0, dhks, r["grad_col_ops"], dcol)
    at = lambda th, sigs=q["sigs"]: _cpu_goal(q, q["h0"] + th[1] * e11, (1 + th[2]) * q["hks"], (1 + th[0]) * q["col"], sigs, ds)[0]
    eps = 1e-5
    fd = np.array([(at(eps * np.eye(3)[t]) - at(-eps * np.eye(3)[t])) / (2 * eps) for t in range(3)])
    print("model_param_grads", got, "finite differences", fd)
    assert np.abs(fd).min() > 1e-3 * np.abs(fd).max()  # every parameter matters
    assert np.abs(got - fd).max() < 1e-6 * np.abs(fd).max()
    gs = np.asarray(r["grad_signals"]["ry90p"])
    assert gs.shape == (q["P"], K, q["N"])
    for p, k, n in ((0, 0, 0), (1, 0, 7), (1, 0, 19)):
        vals = []
        for sgn in (+1, -1):
            s = {g: v.copy() for g, v in q["sigs"].items()}
            s["ry90p"][p, k, n] += sgn * eps
            vals.append(at(np.zeros(3), s))
        fdv = (vals[0] - vals[1]) / (2 * eps)
        print("grad_signals", (p, k, n), gs[p, k, n], fdv)
        assert abs(gs[p, k, n] - fdv) < 1e-6 * np.abs(gs).max()
