"""c3p_seq_chain_vjp, orbit_infid_with_grad and goal_run_batched_with_grad on the GPU.

References: the numpy reverse-mode loop of tests/test_seq_vjp_host.py (itself checked there against central differences),
and central differences of the existing FORWARD entry point c3p_seq_chain, which is independent of both VJPs.

Tolerance against the loop: Gbar is a sum over chains and positions of outer products xbar_{t+1} x_t^H.  Each factor is
the result of at most L matrix-vector products and carries at most ~L M eps relative rounding of the norms met along the
chain; the sums add ~(number of terms) eps more.  With |.| the largest norm of the states and cotangents met (bounded
here by scaling the random tables to norm ~1), the difference of two correct evaluations is below
~2 L M eps * (number of terms) * |out_bar| -- we use atol = 1e-13 * L * M * n_terms * max|out_bar| per entry with the loop's
own magnitude, loose by design at a factor ~4 above that bound, far below any indexing or orientation error (O(1)).
"""
import re

import numpy as np
import pytest

from tests.test_seq_vjp_host import random_table, vjp_loop

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"


@pytest.fixture(scope="module")
def sq(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from c3_amd import sequences

    return sequences


def ragged(rng, S, Lmax, n):
    lengths = rng.integers(0, Lmax + 1, size=S).astype(np.int32)
    lengths[:3] = [0, 1, Lmax]
    seqs = rng.integers(0, n, size=(S, Lmax)).astype(np.int32)
    return seqs, lengths


def cot(rng, mode, P, S, M):
    shape = {"product": (P, S, M, M), "state": (P, S, M), "population": (P, S)}[mode]
    if mode == "population":
        return rng.normal(size=shape)
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def close(got, want, L, M, terms, scale):
    tol = 1e-13 * max(L, 1) * M * max(terms, 1) * scale
    err = np.max(np.abs(got - want))
    assert err <= tol, (err, tol)
    # the check must be able to fail: the reference is far above the tolerance (an all-zero result would not pass)
    assert np.max(np.abs(want)) >= 1e3 * tol, (np.max(np.abs(want)), tol)


def haar(rng, M, n):
    Z = rng.normal(size=(n, M, M)) + 1j * rng.normal(size=(n, M, M))
    Q, R = np.linalg.qr(Z)
    return Q * (np.diagonal(R, axis1=1, axis2=2) / np.abs(np.diagonal(R, axis1=1, axis2=2)))[:, None, :]


def unit_table(rng, P, n, M, eps=0.02):
    """Haar unitaries times (I + eps R), R complex Gaussian / sqrt(M): NOT unitary (nor undone by the adjoint), yet every
    factor has norm 1 + O(eps), so products over a thousand steps neither vanish nor blow up (|log norm| ~ eps sqrt(L))"""
    U = haar(rng, M, P * n).reshape(P, n, M, M)
    R = (rng.normal(size=(P, n, M, M)) + 1j * rng.normal(size=(P, n, M, M))) / np.sqrt(2 * M)
    return U @ (np.eye(M) + eps * R)


@pytest.mark.parametrize("M", [2, 3, 4, 9, 16, 81])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("mode", ["product", "state", "population"])
def test_vjp_matches_reverse_loop(sq, M, shared, mode):
    rng = np.random.default_rng(M + 7 * shared + len(mode))
    P, n = 2, (3 if M <= 16 else 2)
    S, Lmax = (5, 9) if M < 81 else (3, 5)
    G = unit_table(rng, 1 if shared else P, n, M)
    seqs, lengths = ragged(rng, S, Lmax, n)
    psi0 = rng.normal(size=M) + 1j * rng.normal(size=M)
    psi0 /= np.linalg.norm(psi0)
    W = cot(rng, mode, P, S, M)
    Gfull = np.broadcast_to(G, (P,) + G.shape[1:]) if shared else G
    want = vjp_loop(Gfull, seqs, lengths, mode, W, psi0 if mode == "state" else None)
    got = sq.seq_chain_vjp(G[0] if shared else G, seqs, lengths, mode, W, psi0 if mode == "state" else None, P=P)
    if shared:
        want = want.sum(axis=0)
    close(got, want, Lmax, M, S * P * (M if mode == "product" else 1), np.max(np.abs(W)))


@pytest.mark.parametrize(
    "M,n,kernel",
    [
        (2, 16, "seq_vjp_lane_kernel<2>"),
        (4, 4, "seq_vjp_lane_kernel<4>"),
        (9, 4, "seq_vjp_wave_kernel<true, true>"),
        (3, 100, "seq_vjp_wave_kernel<true, true>"),  # 100 gates: too many for the lane kernel's per-lane copies
        (16, 12, "seq_vjp_wave_kernel<false, true>"),  # partial G_bar (48 KB) in LDS, the table beside it does not fit
        (81, 2, "seq_vjp_wave_kernel<false, false>"),  # partial (205 KB) and table from global memory
    ],
)
def test_kernel_variants_and_large_tables(sq, lib, M, n, kernel):
    """every kernel instantiation, identified from the launch log, against the reverse loop"""
    from c3_amd import _lib

    rng = np.random.default_rng(M * n)
    P, S, Lmax = 3, 40, 30
    G = unit_table(rng, P, n, M)
    seqs, lengths = ragged(rng, S, Lmax, n)
    W = cot(rng, "population", P, S, M)
    got = sq.seq_chain_vjp(torch.as_tensor(G, device=DEV), torch.as_tensor(seqs, device=DEV), torch.as_tensor(lengths, device=DEV), "population", torch.as_tensor(W, device=DEV))
    assert _lib.last_kernel() == "seq_vjp"
    detail = _lib.last_kernel_detail()
    assert kernel in detail, detail
    close(got.cpu().numpy(), vjp_loop(G, seqs, lengths, "population", W), Lmax, M, S * P, np.max(np.abs(W)))


@pytest.mark.parametrize("M", [3, 9, 16])
@pytest.mark.parametrize("mode,superop", [("product", False), ("state", False), ("population", False), ("population", True)])
def test_directional_derivative_against_forward_chain(sq, M, mode, superop):
    """Re <Gbar, E> against central differences of the existing forward entry point on non-unitary tables"""
    rng = np.random.default_rng(M + 3 * superop + len(mode))
    P, n, S, Lmax = 2, 3, 6, 12
    G = unit_table(rng, P, n, M) * 1.05
    seqs, lengths = ragged(rng, S, Lmax, n)
    psi0 = rng.normal(size=M) + 1j * rng.normal(size=M)
    psi = psi0 if mode == "state" else None
    out = sq.seq_chain(G, seqs, lengths, mode, psi, superop=superop)
    W = cot(rng, mode, P, S, M)
    Gbar = sq.seq_chain_vjp(G, seqs, lengths, mode, W, psi, superop=superop)

    def f(Gx):
        o = sq.seq_chain(Gx, seqs, lengths, mode, psi, superop=superop)
        return float(np.sum(np.conj(W) * o).real)

    for _ in range(2):
        E = rng.normal(size=G.shape) + 1j * rng.normal(size=G.shape)
        h = 1e-6
        fd = (f(G + h * E) - f(G - h * E)) / (2 * h)
        an = float(np.sum(np.conj(Gbar) * E).real)
        # truncation O(h^2) and rounding eps |f| / h ~ 1e-10 |f|
        assert an == pytest.approx(fd, rel=1e-6, abs=1e-8 * (1 + abs(f(G))))
    assert out.shape[:2] == (P, S)


def _interval(lib_detail):
    m = re.search(r"checkpoint interval C=(\d+)", lib_detail)
    assert m, lib_detail
    return int(m.group(1))


@pytest.mark.parametrize("M", [2, 9])
def test_checkpoint_segment_edges(sq, M):
    """lengths C - 1, C, C + 1, 2C, 2C + 1 and a chain of 1037 steps (not a multiple of C) around the reported interval,
    on the lane kernel (M = 2) and the workgroup kernel (M = 9 with two gates).  Every chain is checked on its own against
    the reverse loop with a RELATIVE tolerance: the tables stay near norm 1, so each chain's reference is O(1) and an
    error in any segment (or a zero result) fails.  Relative rounding of L steps: ~L M eps; the bound used is 1e-14 L M."""
    from c3_amd import _lib

    rng = np.random.default_rng(11 + M)
    n, P = 2, 2
    Lmax = 1037
    G = unit_table(rng, P, n, M)
    seqs = rng.integers(0, n, size=(1, Lmax)).astype(np.int32)
    sq.seq_chain_vjp(G, seqs, np.array([Lmax], dtype=np.int32), "population", np.ones((P, 1)))
    C = _interval(_lib.last_kernel_detail())
    assert C > 1 and Lmax % C != 0
    assert ("seq_vjp_lane_kernel" in _lib.last_kernel_detail()) == (M == 2)
    lengths = np.array([C - 1, C, C + 1, 2 * C, 2 * C + 1, Lmax], dtype=np.int32)
    seqs = rng.integers(0, n, size=(len(lengths), Lmax)).astype(np.int32)
    psi0 = np.eye(M)[1].astype(np.complex128)
    for mode in ("product", "state", "population"):
        psi = psi0 if mode == "state" else None
        W = cot(rng, mode, P, len(lengths), M)
        # all chains in one call (lanes / workgroups of different lengths side by side)
        got = sq.seq_chain_vjp(G, seqs, lengths, mode, W, psi)
        assert _interval(_lib.last_kernel_detail()) == C
        want = vjp_loop(G, seqs, lengths, mode, W, psi)
        ref = np.max(np.abs(want))
        assert ref > 0.05, ref
        assert np.max(np.abs(got - want)) <= 1e-14 * Lmax * M * ref
        # every chain alone
        for s, L in enumerate(lengths):
            Ws = W[:, s : s + 1]
            got = sq.seq_chain_vjp(G, seqs[s : s + 1], lengths[s : s + 1], mode, Ws, psi)
            want = vjp_loop(G, seqs[s : s + 1], lengths[s : s + 1], mode, Ws, psi)
            ref = np.max(np.abs(want))
            assert ref > 0.05, (L, mode, ref)
            assert np.max(np.abs(got - want)) <= 1e-14 * L * M * ref, (L, mode)


@pytest.mark.parametrize("M", [9, 16])
def test_empty_table_checks_and_writes_output(sq, M):
    """n_gates = 0, as c3p_seq_chain: sequences of length 0 are the identity (out written, empty gradient); a sequence
    with a gate is an error"""
    from c3_amd._lib import C3PropError

    P, S = 2, 3
    G = np.zeros((P, 0, M, M), dtype=np.complex128)
    seqs = np.zeros((S, 4), dtype=np.int32)
    psi0 = np.exp(1j * np.arange(M)) / np.sqrt(M)
    for dev in (False, True):
        cv = (lambda x: torch.as_tensor(x, device=DEV)) if dev else (lambda x: x)
        W = cot(np.random.default_rng(0), "state", P, S, M)
        g, out = sq.seq_chain_vjp(cv(G), cv(seqs), cv(np.zeros(S, dtype=np.int32)), "state", cv(W), cv(psi0), want_out=True)
        out = out.cpu().numpy() if dev else out
        assert g.numel() == 0 if dev else g.size == 0
        assert np.array_equal(out, np.broadcast_to(psi0, (P, S, M)))
        with pytest.raises(C3PropError, match="gate index|outside"):
            sq.seq_chain_vjp(cv(G), cv(seqs), cv(np.array([0, 2, 0], dtype=np.int32)), "state", cv(W), cv(psi0))


def test_superop_zero_population_gives_zero_cotangent(sq):
    G = np.zeros((1, 2, 4, 4), dtype=np.complex128)
    G[0, 0, 1, 0] = 1.0
    G[0, 1] = np.eye(4)
    seqs = np.array([[1, 0], [1, 1]], dtype=np.int32)
    Gbar = sq.seq_chain_vjp(G, seqs, np.array([2, 2], dtype=np.int32), "population", np.array([[1.0, 0.0]]), superop=True)
    assert np.all(np.isfinite(Gbar)) and not np.any(Gbar)


def test_deterministic_and_host_device_torch_agree(sq):
    from c3_amd import _lib

    rng = np.random.default_rng(5)
    P, n, M, S, Lmax = 64, 4, 3, 300, 200
    G = unit_table(rng, P, n, M)
    seqs, lengths = ragged(rng, S, Lmax, n)
    W = cot(rng, "population", P, S, M)
    Gt, st, lt, Wt = (torch.as_tensor(x, device=DEV) for x in (G, seqs, lengths, W))
    a, out = sq.seq_chain_vjp(Gt, st, lt, "population", Wt, want_out=True)
    b = sq.seq_chain_vjp(Gt, st, lt, "population", Wt)
    assert torch.equal(a, b)
    h = sq.seq_chain_vjp(G, seqs, lengths, "population", W)
    assert np.array_equal(h, a.cpu().numpy())
    fwd = sq.seq_chain(Gt, st, lt, "population")
    assert torch.allclose(out, fwd, rtol=0, atol=1e-13)
    # the workgroup kernel too
    G9 = unit_table(rng, 4, 4, 9)
    W9 = cot(rng, "product", 4, 20, 9)
    s9, l9 = ragged(rng, 20, 50, 4)
    x = sq.seq_chain_vjp(torch.as_tensor(G9, device=DEV), s9, l9, "product", torch.as_tensor(W9, device=DEV), want_out=True)
    y = sq.seq_chain_vjp(torch.as_tensor(G9, device=DEV), s9, l9, "product", torch.as_tensor(W9, device=DEV))
    assert torch.equal(x[0], y)
    assert torch.allclose(x[1], sq.seq_chain(torch.as_tensor(G9, device=DEV), s9, l9, "product"), rtol=0, atol=1e-13)
    assert _lib.last_kernel() == "seq"


def test_errors_then_next_call_works(sq):
    from c3_amd._lib import C3PropError

    rng = np.random.default_rng(6)
    G = unit_table(rng, 2, 3, 4)
    seqs, lengths = ragged(rng, 6, 8, 3)
    W = cot(rng, "state", 2, 6, 4)
    psi = np.eye(4)[0].astype(np.complex128)
    bad = seqs.copy()
    bad[2, 0] = 3
    for dev in (False, True):
        cv = (lambda x: torch.as_tensor(x, device=DEV)) if dev else (lambda x: x)
        with pytest.raises(C3PropError, match="gate index|outside"):
            sq.seq_chain_vjp(cv(G), cv(bad), cv(lengths), "state", cv(W), cv(psi))
        badlen = lengths.copy()
        badlen[1] = 9
        with pytest.raises(C3PropError, match="length"):
            sq.seq_chain_vjp(cv(G), cv(seqs), cv(badlen), "state", cv(W), cv(psi))
        with pytest.raises(C3PropError, match="out_bar"):
            sq.seq_chain_vjp(cv(G), cv(seqs), cv(lengths), "state", cv(W[:, :5]), cv(psi))
        got = sq.seq_chain_vjp(cv(G), cv(seqs), cv(lengths), "state", cv(W), cv(psi))
        got = got.cpu().numpy() if dev else got
        close(got, vjp_loop(G, seqs, lengths, "state", W, psi), 8, 4, 12, np.max(np.abs(W)))


# ---------------------------------------------------------------------------------------------------------------------------
# ORBIT
# ---------------------------------------------------------------------------------------------------------------------------
def _noisy_generators(rng, P, lindblad=False):
    from c3_amd.sequences import GENERATORS, _ideal_generators

    ideal = _ideal_generators()
    out = {}
    for g in GENERATORS:
        U = np.zeros((P, 3, 3), dtype=np.complex128)
        U[:, :2, :2] = ideal[g]
        U[:, 2, 2] = 1.0
        H = rng.normal(size=(P, 3, 3)) + 1j * rng.normal(size=(P, 3, 3))
        H = 0.03 * (H + np.conj(np.swapaxes(H, 1, 2)))
        w, V = np.linalg.eigh(H)
        E = V @ (np.exp(-1j * w)[..., None] * np.conj(np.swapaxes(V, 1, 2)))
        U = E @ U
        if lindblad:
            U = np.einsum("pij,pkl->pikjl", U, U.conj()).reshape(P, 9, 9) * 0.999
        out[f"{g}[0]"] = U
    return out


@pytest.mark.parametrize("lindblad", [False, True])
def test_orbit_infid_with_grad(sq, lindblad):
    from c3_amd._lib import C3PropError

    rng = np.random.default_rng(8 + lindblad)
    P = 3
    props = _noisy_generators(rng, P, lindblad)
    seqs = sq.single_length_RB(12, 6, rng=3)
    want = sq.orbit_infid(props, lindbladian=lindblad, seqs=seqs)
    infid, grads = sq.orbit_infid_with_grad(props, lindbladian=lindblad, seqs=seqs)
    assert np.allclose(infid, want, rtol=0, atol=1e-13)
    for k, U in props.items():
        E = rng.normal(size=U.shape) + 1j * rng.normal(size=U.shape)
        h = 1e-6
        fp = sq.orbit_infid({**props, k: U + h * E}, lindbladian=lindblad, seqs=seqs)
        fm = sq.orbit_infid({**props, k: U - h * E}, lindbladian=lindblad, seqs=seqs)
        fd = (fp - fm) / (2 * h)
        an = np.sum(np.conj(grads[k]) * E, axis=(-2, -1)).real
        assert np.allclose(an, fd, rtol=1e-6, atol=1e-9)
    with pytest.raises(C3PropError):
        sq.orbit_infid_with_grad(props, seqs=seqs, shots=100)
    with pytest.raises(C3PropError):
        sq.orbit_infid_with_grad(props, seqs=seqs, noise=0.01)


# ---------------------------------------------------------------------------------------------------------------------------
# model learning
# ---------------------------------------------------------------------------------------------------------------------------
def _ml_problem():
    from tests.test_model_learning import _problem

    return _problem()


@pytest.mark.parametrize("on_device", [False, True])
def test_goal_run_batched_with_grad_goal_and_model_gradient(lib, on_device):
    from c3_amd import model_learning as ml

    w, gate_signals, data_sets, psi0, labels = _ml_problem()
    dev = DEV if on_device else None
    base = ml.goal_run_batched(w.h0, w.hks, gate_signals, w.dt, data_sets, psi0, labels, device=dev)
    r = ml.goal_run_batched_with_grad(w.h0, w.hks, gate_signals, w.dt, data_sets, psi0, labels, device=dev)
    assert r["goal"] == pytest.approx(base["goal"], rel=1e-12)
    assert np.allclose(r["goals"], base["goals"], rtol=1e-12, atol=0)
    assert np.allclose(r["sim_vals"], base["sim_vals"], rtol=1e-12, atol=1e-14)
    # the frequency of subsystem 0: h0 + 2 pi v n0, with n0 the number operator of the first subsystem
    D = w.h0.shape[-1]
    d0 = int(w.dims[0])
    n0 = np.kron(np.diag(np.arange(d0)), np.eye(D // d0)).astype(np.complex128)
    dh0 = (2 * np.pi * n0)[None]
    g = ml.model_param_grads(r["grad_h0"], r["grad_hks"], dh0)[0]
    h = 1e5  # Hz: truncation (2 pi h N dt)^2 ~ 1e-8 relative, rounding eps |goal| / (h |goal'|) ~ 1e-12
    fp = ml.goal_run_batched(w.h0 + h * dh0[0], w.hks, gate_signals, w.dt, data_sets, psi0, labels)["goal"]
    fm = ml.goal_run_batched(w.h0 - h * dh0[0], w.hks, gate_signals, w.dt, data_sets, psi0, labels)["goal"]
    assert g == pytest.approx((fp - fm) / (2 * h), rel=1e-5)
    # a control-signal direction
    rng = np.random.default_rng(4)
    gate = "cr[0,1]"
    E = rng.normal(size=gate_signals[gate].shape) * 1e6
    an = float(np.sum(torch.as_tensor(r["grad_signals"][gate]).cpu().numpy() * E))
    hs = 1.0
    sp = {**gate_signals, gate: gate_signals[gate] + hs * E}
    sm = {**gate_signals, gate: gate_signals[gate] - hs * E}
    fd = (ml.goal_run_batched(w.h0, w.hks, sp, w.dt, data_sets, psi0, labels)["goal"] - ml.goal_run_batched(w.h0, w.hks, sm, w.dt, data_sets, psi0, labels)["goal"]) / (2 * hs)
    assert an == pytest.approx(fd, rel=1e-5)


def test_goal_run_batched_with_grad_frame_phases_and_all_populations(lib):
    """grad_fr_phase against central differences of goal_run_batched along a random direction of every gate's phases;
    then label_indices = None (every population is a simulated value, results [S, D]): goal as goal_run_batched and the
    frequency gradient against central differences"""
    from c3_amd import model_learning as ml

    w, gate_signals, data_sets, psi0, labels = _ml_problem()
    P, D = len(data_sets), int(w.h0.shape[-1])
    rng = np.random.default_rng(12)
    ph = {g: rng.uniform(-1, 1, size=(P, D)) for g in gate_signals}
    r = ml.goal_run_batched_with_grad(w.h0, w.hks, gate_signals, w.dt, data_sets, psi0, labels, fr_phase=ph, device=DEV)
    base = ml.goal_run_batched(w.h0, w.hks, gate_signals, w.dt, data_sets, psi0, labels, fr_phase=ph)
    assert r["goal"] == pytest.approx(base["goal"], rel=1e-12)
    E = {g: rng.normal(size=(P, D)) for g in gate_signals}
    an = sum(float(np.sum(r["grad_fr_phase"][g].cpu().numpy() * E[g])) for g in gate_signals)
    h = 1e-5  # rad: truncation (h |E|)^2 ~ 1e-9 relative, rounding eps |goal| / h ~ 1e-10 |goal|
    f = lambda sgn: ml.goal_run_batched(w.h0, w.hks, gate_signals, w.dt, data_sets, psi0, labels, fr_phase={g: ph[g] + sgn * h * E[g] for g in ph})["goal"]
    assert an == pytest.approx((f(1) - f(-1)) / (2 * h), rel=1e-5)

    # every population: results [S, D] near the simulated values (so the likelihood stays smooth where populations are small)
    S = len(data_sets[0]["seqs"])
    cols = [{**d, "results": np.full((S, D), 0.5), "shots": np.asarray(d["shots"], dtype=np.float64)[:, None]} for d in data_sets]
    sim = ml.goal_run_batched(w.h0, w.hks, gate_signals, w.dt, cols, psi0, None)["sim_vals"]  # [P,S,D]
    sets = [{**d, "results": sim[p] * (1 + 0.05 * rng.normal(size=sim[p].shape))} for p, d in enumerate(cols)]
    r = ml.goal_run_batched_with_grad(w.h0, w.hks, gate_signals, w.dt, sets, psi0, None, device=DEV)
    base = ml.goal_run_batched(w.h0, w.hks, gate_signals, w.dt, sets, psi0, None)
    assert r["goal"] == pytest.approx(base["goal"], rel=1e-12)
    assert r["sim_vals"].shape == (P, len(sets[0]["seqs"]), D)
    d0 = int(w.dims[0])
    dh0 = (2 * np.pi * np.kron(np.diag(np.arange(d0)), np.eye(D // d0)).astype(np.complex128))[None]
    g = ml.model_param_grads(r["grad_h0"], r["grad_hks"], dh0)[0]
    hv = 1e5
    fd = (ml.goal_run_batched(w.h0 + hv * dh0[0], w.hks, gate_signals, w.dt, sets, psi0, None)["goal"]
          - ml.goal_run_batched(w.h0 - hv * dh0[0], w.hks, gate_signals, w.dt, sets, psi0, None)["goal"]) / (2 * hv)
    assert g == pytest.approx(fd, rel=1e-5)


def _qutrit(freq, anh):
    """a driven qutrit in the frame of the drive: detuning freq and anharmonicity anh (Hz), two quadrature controls"""
    a = np.diag(np.sqrt([1.0, 2.0]), 1).astype(np.complex128)
    n = a.conj().T @ a
    h0 = 2 * np.pi * (freq * n + 0.5 * anh * n @ (n - np.eye(3)))
    hks = np.stack([(a + a.conj().T) / 2, 1j * (a.conj().T - a) / 2])
    return h0, hks, n


def test_learning_with_lbfgs_recovers_qutrit_parameters(lib):
    """synthetic ORBIT data at known frequency (a frame detuning) and anharmonicity; L-BFGS-B with the analytic gradient
    from a start 1e5 Hz off cuts each parameter's error 100-fold within 50 evaluations"""
    from scipy.optimize import minimize

    from c3_amd import model_learning as ml
    from c3_amd import sequences as sq

    true = np.array([2.0e5, -2.8e8])
    N, T = 80, 8e-9  # a short pulse: its bandwidth reaches the second level, so the anharmonicity is seen
    dt = T / N
    t = (np.arange(N) + 0.5) * dt
    env = np.exp(-((t - T / 2) ** 2) / (2 * (T / 5) ** 2))
    amp = (np.pi / 2) / (np.sum(env) * dt)  # a pi/2 rotation on the 0-1 transition (the control is sigma_x / 2 there)
    z = np.zeros(N)
    pulses = {"rx90p[0]": (env, z), "rx90m[0]": (-env, z), "ry90p[0]": (z, env), "ry90m[0]": (z, -env)}
    P = 2  # two parameter sets: the pulses at two drive scales
    scales = [1.0, 0.8]
    sig = {g: np.stack([np.stack([amp * s * i, amp * s * q]) for s in scales]) for g, (i, q) in pulses.items()}
    rng = np.random.default_rng(0)
    seqs = [[g for c in row for g in c] for row in [[sq.CLIFFORD_WORDS[k] for k in rng.integers(0, 24, size=5)] for _ in range(20)]]
    seqs = [[f"{g}[0]" for g in s] for s in seqs]
    psi0 = np.array([1, 0, 0], dtype=np.complex128)
    labels = [1]
    h0, hks, n = _qutrit(*true)
    sim = ml.goal_run_batched(h0, hks, sig, dt, [{"seqs": seqs, "results": [0.5] * len(seqs), "results_std": [0.01] * len(seqs), "shots": [1000] * len(seqs)}] * P, psi0, labels)["sim_vals"]
    data = [{"seqs": seqs, "results": list(sim[p]), "results_std": [0.01] * len(seqs), "shots": [1000] * len(seqs)} for p in range(P)]
    nn = n @ (n - np.eye(3))
    dh0 = np.stack([2 * np.pi * n, np.pi * nn])
    scale = 1e5  # optimizer coordinates: offsets in units of 100 kHz

    def fun(x):
        th = start + x * scale
        h0x, _, _ = _qutrit(*th)
        r = ml.goal_run_batched_with_grad(h0x, hks, sig, dt, data, psi0, labels, device=DEV)
        g = ml.model_param_grads(r["grad_h0"], r["grad_hks"], dh0) * scale
        return r["goal"], g

    start = true + np.array([1e5, -1e5])
    res = minimize(fun, np.zeros(2), jac=True, method="L-BFGS-B", options={"maxfun": 50, "ftol": 1e-15, "gtol": 1e-12})
    err0 = np.abs(start - true)
    err = np.abs(start + res.x * scale - true)
    assert res.nfev <= 50
    assert np.all(err * 100 <= err0), (err, res)
