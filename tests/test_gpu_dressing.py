"""c3p_dress / c3p_dress_vjp on the GPU (c3_amd/dressing.py) against tests/dressing_ref.py.

Bounds from first-order perturbation theory, with kappa = ||H||_2 / min gap of the input's spectrum and eps = 2^-52:
  max|e - e_ref| <= D eps ||H||_2,   ||T^+ T - I||_F <= D eps sqrt(D),   ||T - T_ref||_F <= D eps kappa sqrt(D),
  dressed operators within 2 D eps kappa ||A||_F;
the VJP against the numpy closed form fed THE SAME T and e, within 8 D eps || |T| (|W'| o |F| + |diag ebar|) |T^+| ||_F for the
gradient on H and 8 D eps || |T| |Gbar| |T^+| ||_F for the bare operators (shared operators: the sum of the sets' bounds, their
errors add).  Every check prints the ratio to its bound before asserting it."""
import functools
import os
import warnings

import numpy as np
import pytest

import dressing_ref as dr
from c3_amd import _lib, workloads

pytestmark = pytest.mark.gpu

EPS = 2.0**-52
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dressing(lib):
    from c3_amd import dressing as d

    _lib.require_gpu()
    return d


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _quiet(fn, *a, **k):
    """the call without the reference's 'overly dressed' warning"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


@functools.lru_cache(maxsize=None)
def _random_model(D, complex_drift=False, seed=0):
    """well separated bare levels in rad/s with couplings a hundredth of the spacing: the ordered branch"""
    rng = np.random.default_rng(100 * D + seed)
    X = rng.normal(size=(D, D)) + (1j * rng.normal(size=(D, D)) if complex_drift else 0)
    H = np.diag(2 * np.pi * (5e9 + 3e8 * rng.permutation(D))) + 2 * np.pi * 3e6 * (X + X.conj().T)
    return H.astype(np.complex128)


def _ops(D, M, seed=1, P=None):
    rng = np.random.default_rng(seed + D)
    shape = (M, D, D) if P is None else (P, M, D, D)
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)  # not Hermitian


def _check_forward(H, ops, r, what, status=0):
    """H [P,D,D], ops None / [M,D,D] / [P,M,D,D] against the host reference, set by set; returns the worst ratios"""
    H = np.asarray(H)
    P, D = H.shape[0], H.shape[-1]
    e, T, h0, st = _np(r["eigenframe"]), _np(r["transform"]), _np(r["h0"]), _np(r["status"])
    G = None if r["ops"] is None else _np(r["ops"])
    worst = np.zeros(4)
    for p in range(P):
        A = None if ops is None else (ops if ops.ndim == 3 else ops[p])
        ref = dr.dress_ref(H[p], A)
        nH = np.linalg.norm(H[p], 2)
        kap = nH / np.min(np.diff(np.sort(ref["eigenframe"])))
        ratios = [np.abs(e[p] - ref["eigenframe"]).max() / (D * EPS * nH), np.linalg.norm(T[p].conj().T @ T[p] - np.eye(D)) / (D * EPS * np.sqrt(D)),
                  np.linalg.norm(T[p] - ref["transform"]) / (D * EPS * kap * np.sqrt(D)), 0.0]
        if A is not None:
            ratios[3] = max(np.linalg.norm(G[p, m] - ref["ops"][m]) / (2 * D * EPS * kap * np.linalg.norm(A[m])) for m in range(len(A)))
        worst = np.maximum(worst, ratios)
        assert st[p] == status == ref["status"], (what, p, st[p], ref["status"])
        assert np.array_equal(h0[p], np.diag(e[p])), (what, p)
        assert np.abs(np.diagonal(T[p]).imag).max() == 0 and (np.diagonal(T[p]).real > 0).all(), (what, p)
    print(f"{what}: D={D} P={P} ratios to the bounds: e {worst[0]:.3f}, T^+T {worst[1]:.3f}, T {worst[2]:.3f}, ops {worst[3]:.3f}")
    assert (worst <= 1.0).all(), (what, worst)
    return worst


def _check_vjp(dressing, H, ops, what, seed=0, with_transform=True, on_device=False):
    """forward on the device, random cotangents, the device VJP against the closed form on the device's own T and e"""
    import torch

    H = np.asarray(H)
    P, D = H.shape[0], H.shape[-1]
    rng = np.random.default_rng(seed)
    M = 0 if ops is None else ops.shape[-3]
    to = (lambda x: None if x is None else torch.as_tensor(x, device=DEV)) if on_device else (lambda x: x)
    f = _quiet(dressing.dress_batch, to(H), to(ops))
    T, e = _np(f["transform"]), _np(f["eigenframe"])
    eb = rng.normal(size=(P, D))
    hb = rng.normal(size=(P, D, D)) + 1j * rng.normal(size=(P, D, D))
    Gb = None if M == 0 else rng.normal(size=(P, M, D, D)) + 1j * rng.normal(size=(P, M, D, D))
    # (the cotangent of T on the scale of the level spacings, so that W' o F weighs as much as diag(ebar) in the result)
    scale = np.array([np.linalg.norm(h, 2) / D for h in H])[:, None, None]
    Tb = scale * (rng.normal(size=(P, D, D)) + 1j * rng.normal(size=(P, D, D))) if with_transform else None
    v = dressing.dress_batch_vjp(f["transform"], f["eigenframe"], to(ops), grad_h0=to(hb), grad_ops=to(Gb), grad_eigenframe=to(eb), grad_transform=to(Tb))
    gH, st = _np(v["grad_H"]), _np(v["status"])
    gA = None if M == 0 else _np(v["grad_ops"])
    shared = ops is not None and ops.ndim == 3
    worst_H = worst_A = 0.0
    sum_ref = None if not shared else np.zeros((M, D, D), dtype=np.complex128)
    sum_bound = None if not shared else np.zeros(M)
    for p in range(P):
        A = None if ops is None else (ops if shared else ops[p])
        kw = dict(grad_ops=None if M == 0 else Gb[p], grad_eigenframe=eb[p], grad_h0=hb[p], grad_transform=None if Tb is None else Tb[p])
        ref = dr.dress_vjp_ref(T[p], e[p], A, **kw)
        bound = 8 * D * EPS * dr.vjp_bound(T[p], e[p], A, **kw)
        worst_H = max(worst_H, np.linalg.norm(gH[p] - ref["grad_H"]) / bound)
        assert st[p] == ref["status"] == 0, (what, p)
        assert np.array_equal(gH[p], gH[p].conj().T), (what, p)
        if M and shared:
            sum_ref += ref["grad_ops"]
            sum_bound += 8 * D * EPS * dr.vjp_bound_ops(T[p], Gb[p])
        elif M:
            b = 8 * D * EPS * dr.vjp_bound_ops(T[p], Gb[p])
            worst_A = max(worst_A, max(np.linalg.norm(gA[p, m] - ref["grad_ops"][m]) / b[m] for m in range(M)))
    if M and shared:
        assert gA.shape == (M, D, D)
        worst_A = max(np.linalg.norm(gA[m] - sum_ref[m]) / sum_bound[m] for m in range(M))
    print(f"{what}: D={D} P={P} M={M} VJP ratios to the bounds: grad_H {worst_H:.2e}, grad_ops {worst_A:.2e}")
    assert worst_H <= 1.0 and worst_A <= 1.0, (what, worst_H, worst_A)
    return f, v


# ---- dimensions -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("D", [2, 3, 12, 13, 16, 17, 40])
def test_random_real_models(dressing, D):
    """a single pair, the bye of an odd dimension, both sides of the one-wave / four-wave boundary (16 | 17) and of the chain
    kernels' (12 | 13), the largest dimension"""
    H = np.stack([_random_model(D), _random_model(D, seed=1)])
    ops = _ops(D, 2)
    _check_forward(H, ops, dressing.dress_batch(H, ops), f"random real D={D}")
    _check_vjp(dressing, H, ops, f"random real D={D}", seed=D)


def test_golden_two_qubit_arrays(dressing, golden_dir):
    g = np.load(os.path.join(golden_dir, "two_qubit.npz"))
    m = workloads.ChipModel((2, 2), (5e9, 5.6e9), (0, 0), {(0, 1): 20e6}, {"d1": 0, "d2": 1}, dressed=False)
    ops = np.stack([m.control_hams["d1"], m.control_hams["d2"]])
    r = dressing.dress_batch(m.drift_ham, ops)
    assert r["h0"].shape == (4, 4) and r["ops"].shape == (2, 4, 4) and r["eigenframe"].shape == (4,) and r["status"].shape == ()
    kap = dr.kappa_of(m.drift_ham)
    assert np.abs(r["h0"] - g["hdrift"]).max() <= 4 * EPS * np.linalg.norm(m.drift_ham, 2)
    for got, key, A in ((r["ops"][0], "hk_d1", ops[0]), (r["ops"][1], "hk_d2", ops[1])):
        assert np.linalg.norm(got - g[key]) <= 2 * 4 * EPS * kap * np.linalg.norm(A)
    _check_forward(m.drift_ham[None], ops, dressing.dress_batch(m.drift_ham[None], ops), "two qubits D=4")


@pytest.mark.parametrize("dims", [(3, 3), (3, 3, 3), (3, 3, 4)])
def test_cfg_models(dressing, dims):
    H, hks = dr.cfg_model(dims)
    r = dressing.dress_batch(H[None], hks)
    _check_forward(H[None], hks, r, f"cfg model {dims}")
    T = workloads.dressing_transform(H)
    assert np.linalg.norm(r["transform"][0] - T) <= len(H) * EPS * dr.kappa_of(H) * np.sqrt(len(H))
    _check_vjp(dressing, H[None], hks, f"cfg model {dims}", seed=len(dims))


def test_complex_hermitian_perturbation_of_cfg2(dressing):
    H, hks = dr.cfg_model((3, 3))
    rng = np.random.default_rng(2)
    X = rng.normal(size=(3, 9, 9)) + 1j * rng.normal(size=(3, 9, 9))
    Hc = H[None] + 2 * np.pi * 5e6 * (X + X.conj().transpose(0, 2, 1))
    _check_forward(Hc, hks, dressing.dress_batch(Hc, hks), "complex cfg2")
    _check_vjp(dressing, Hc, hks, "complex cfg2", seed=7)
    Hc40 = _random_model(40, True)[None]
    _check_forward(Hc40, None, dressing.dress_batch(Hc40), "complex D=40")
    Hc17 = _random_model(17, True)[None]
    _check_vjp(dressing, Hc17, _ops(17, 1), "complex D=17", seed=8)


def test_dimension_41_is_refused(dressing):
    with pytest.raises(_lib.C3PropError, match="2 <= D <= 40"):
        dressing.dress_batch(np.eye(41))
    with pytest.raises(_lib.C3PropError, match="2 <= D <= 40"):
        dressing.dress_batch_vjp(np.eye(41), np.arange(41.0))
    with pytest.raises(_lib.C3PropError, match="Hermitian"):
        dressing.dress_batch(np.triu(np.ones((4, 4))))
    bad = _random_model(5).copy()
    bad[1, 1] = np.nan
    with pytest.raises(_lib.C3PropError, match="did not converge"):
        dressing.dress_batch(bad)


# ---- batch and operator layout ----------------------------------------------------------------------------------------------


def _cfg2_batch(P):
    """P two-qutrit models, the first frequency and the coupling differ from set to set"""
    Hs = [workloads.bare_drift((3, 3), (5.0e9 + 2e6 * p, 5.6e9), dr.ANHARS[:2], {(0, 1): 20e6 + 1e5 * p}) for p in range(P)]
    return np.stack(Hs)


def _cfg2_ops(M):
    """x-type and y-type drives (Hermitian), then collapse operators (not Hermitian)"""
    a = workloads.annihilators((3, 3))
    ops = [a[0] + a[0].conj().T, 1j * (a[1] - a[1].conj().T), workloads.qubit_collapse_op(a[0], 27e-6, 39e-6), workloads.qubit_collapse_op(a[1], 23e-6, None), a[0] @ a[1]]
    return np.stack(ops[:M])


@pytest.mark.parametrize("P", [1, 3, 67])
@pytest.mark.parametrize("M, per_set", [(0, False), (1, False), (5, False), (5, True)])
def test_batch_and_operator_layouts(dressing, P, M, per_set):
    H = _cfg2_batch(P)
    ops = None if M == 0 else _cfg2_ops(M)
    if per_set:
        ops = ops[None] * (1.0 + 0.1 * np.arange(P))[:, None, None, None]
    r = dressing.dress_batch(H, ops)
    assert (r["ops"] is None) == (M == 0)
    _check_forward(H, ops, r, f"layout P={P} M={M} per_set={per_set}")
    if P != 67 or M == 5:
        _check_vjp(dressing, H, ops, f"layout P={P} M={M} per_set={per_set}", seed=P + M, with_transform=M != 1)


def test_both_pointer_routes_and_a_side_stream(dressing):
    import torch

    H, ops = _cfg2_batch(5), _cfg2_ops(3)
    host = dressing.dress_batch(H, ops)
    Hd, od = torch.as_tensor(H, device=DEV), torch.as_tensor(ops, device=DEV)
    dev = dressing.dress_batch(Hd, od)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = dressing.dress_batch(Hd, od)
        vs = dressing.dress_batch_vjp(on_side["transform"], on_side["eigenframe"], od, grad_ops=on_side["ops"], grad_h0=on_side["h0"])
    side.synchronize()
    for k in ("h0", "ops", "eigenframe", "transform", "status"):
        assert torch.is_tensor(dev[k]) and dev[k].is_cuda and isinstance(host[k], np.ndarray)
        assert np.array_equal(_np(dev[k]), host[k]) and np.array_equal(_np(on_side[k]), host[k]), k
    vh = dressing.dress_batch_vjp(host["transform"], host["eigenframe"], ops, grad_ops=host["ops"], grad_h0=host["h0"])
    for k in ("grad_H", "grad_ops", "status"):
        assert np.array_equal(_np(vs[k]), vh[k]), k
    _check_vjp(dressing, H, ops, "device pointers", seed=3, on_device=True)


# ---- the greedy branch -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 3, 3)])
def test_greedy_branch(dressing, dims):
    H, hks = dr.greedy_model(dims)
    with pytest.warns(UserWarning, match="C3 Warning: Some states are overly dressed, trying to recover..."):
        r = dressing.dress_batch(H[None], hks)
    _check_forward(H[None], hks, r, f"greedy {dims}", status=1)
    # next to an ordered set: one status per set
    H2 = np.stack([H, dr.cfg_model(dims)[0]])
    st = _quiet(dressing.dress_batch, H2)["status"]
    assert list(st) == [1, 0]
    _check_vjp(dressing, H[None], hks, f"greedy {dims}", seed=11)


# ---- exact properties -------------------------------------------------------------------------------------------------------


def test_already_diagonal_input(dressing):
    d = 2 * np.pi * np.array([5.1e9, 4.9e9, 5.3e9, 4.9e9, 0.0])
    H = np.diag(d).astype(np.complex128)
    r = dressing.dress_batch(H, np.stack([H, H.T]))
    assert np.array_equal(r["transform"], np.eye(5)) and np.array_equal(r["eigenframe"], d) and r["status"] == 0
    assert np.array_equal(r["ops"][0], H)
    rng = np.random.default_rng(0)
    Tb = rng.normal(size=(5, 5)) + 1j * rng.normal(size=(5, 5))
    v = dressing.dress_batch_vjp(r["transform"], r["eigenframe"], grad_transform=Tb)
    assert v["status"] == 2
    ref = dr.dress_vjp_ref(np.eye(5, dtype=complex), d, grad_transform=Tb)
    assert v["grad_H"][1, 3] == 0 and v["grad_H"][3, 1] == 0  # the skipped pair, exactly
    assert np.abs(v["grad_H"] - ref["grad_H"]).max() <= 8 * 5 * EPS * np.abs(ref["grad_H"]).max()
    assert np.abs(v["grad_H"][0, 1]) > 0


@pytest.mark.parametrize("which", ["cfg2", "complex", "greedy"])
def test_scaling_by_a_power_of_two(dressing, which):
    """no absolute threshold anywhere: 2^-30 H has the same T bit for bit, and the eigenvalues scaled exactly"""
    H = {"cfg2": lambda: dr.cfg_model((3, 3))[0], "complex": lambda: _random_model(17, True), "greedy": lambda: dr.greedy_model((2, 2, 2))[0]}[which]()
    a = _quiet(dressing.dress_batch, H)
    b = _quiet(dressing.dress_batch, H * 2.0**-30)
    assert np.array_equal(a["transform"], b["transform"])
    assert np.array_equal(a["eigenframe"] * 2.0**-30, b["eigenframe"])
    assert a["status"] == b["status"]


def test_reproducible_bit_for_bit(dressing):
    for H, ops in ((_cfg2_batch(67), _cfg2_ops(5)), (np.stack([dr.cfg_model((3, 3, 4))[0]] * 3), dr.cfg_model((3, 3, 4))[1])):
        a, b = dressing.dress_batch(H, ops), dressing.dress_batch(H, ops)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        rng = np.random.default_rng(5)
        Gb = rng.normal(size=a["ops"].shape) + 1j * rng.normal(size=a["ops"].shape)
        va = dressing.dress_batch_vjp(a["transform"], a["eigenframe"], ops, grad_ops=Gb, grad_h0=a["h0"])
        vb = dressing.dress_batch_vjp(a["transform"], a["eigenframe"], ops, grad_ops=Gb, grad_h0=a["h0"])
        for k in va:
            assert np.array_equal(va[k], vb[k]), k


def test_launch_log_names_the_kernels(dressing):
    H, hks = dr.cfg_model((3, 3))
    r = dressing.dress_batch(H, hks)
    assert _lib.last_kernel() == "dress"
    assert "c3p_dress.hip: dress_jacobi_kernel<64>" in _lib.last_kernel_detail()
    dressing.dress_batch_vjp(r["transform"], r["eigenframe"], hks, grad_ops=r["ops"])
    assert _lib.last_kernel() == "dress_vjp"
    log = _lib.last_kernel_detail()
    assert "dress_vjp_kernel<64, 4>" in log and "dress_vjp_opsum_kernel" in log
    H27 = dr.cfg_model((3, 3, 3))[0]
    dressing.dress_batch(H27)
    assert "dress_jacobi_kernel<256>" in _lib.last_kernel_detail()


# ---- end to end -------------------------------------------------------------------------------------------------------------

SEQS = [["rx90p[0]"], ["rx90p[0]", "ry90p[1]"], ["ry90p[1]", "rx90p[0]", "ry90p[1]"], ["rx90p[0]", "rx90p[0]", "ry90p[1]"]]
P_E2E, N_E2E, DT_E2E = 3, 40, 1e-11


def _e2e_problem(dims, with_col):
    """P sets of a two-transmon model (the first frequency differs), two gates, four short sequences; theta = (f_0 shift, g)"""
    nq, D = len(dims), int(np.prod(dims))
    a = workloads.annihilators(dims)
    rng = np.random.default_rng(31 + D)
    ts = (np.arange(N_E2E) + 0.5) * DT_E2E
    sig = np.empty((P_E2E, nq, N_E2E))
    for p in range(P_E2E):
        for k in range(nq):
            sig[p, k] = 2 * np.pi * 1e9 * rng.uniform(0.2, 0.6) * np.cos(2 * np.pi * (dr.FREQS[k] + 50e6) * ts + rng.uniform(0, 2 * np.pi))
    gate_signals = {"rx90p[0]": sig, "ry90p[1]": sig[::-1].copy() * 0.7}
    psi0 = np.zeros(D, dtype=np.complex128)
    psi0[0] = 1.0
    data_sets = [{"seqs": SEQS, "results": list(rng.uniform(0.2, 0.8, size=len(SEQS))), "results_std": [0.02] * len(SEQS), "shots": [1000 + 10 * p] * len(SEQS)}
                 for p in range(P_E2E)]
    anh = dr.ANHARS[:nq]
    G = np.stack([2 * np.pi * a[0].conj().T @ a[0], 2 * np.pi * (a[0].conj().T + a[0]) @ (a[1].conj().T + a[1])])  # dH / d f_0, dH / d g

    def H_of(theta):
        return np.stack([workloads.bare_drift(dims, (5.0e9 + 2e6 * p, 5.6e9), anh, {(0, 1): 20e6}) + theta[0] * G[0] + (theta[1] - 20e6) * G[1] for p in range(P_E2E)])

    hks_bare = np.stack([x + x.conj().T for x in a])
    # decoherence on the scale of the gates (0.4 ns), so that the collapse operators carry gradient
    col_bare = np.stack([workloads.qubit_collapse_op(x, 3e-9, 5e-9) for x in a]) if with_col else None
    return dict(H_of=H_of, G=G, hks=hks_bare, col=col_bare, sig=gate_signals, psi0=psi0, data=data_sets, labels=[1], D=D)


def _host_dressed_goal(ml, q, theta):
    H = q["H_of"](theta)
    Ts = [workloads.dressing_transform(h) for h in H]
    h0 = np.stack([workloads.dress(h, T) for h, T in zip(H, Ts)])
    hks = np.stack([np.stack([workloads.dress(A, T) for A in q["hks"]]) for T in Ts])
    col = None if q["col"] is None else np.stack([np.stack([workloads.dress(A, T) for A in q["col"]]) for T in Ts])
    return ml.goal_run_batched(h0, hks, q["sig"], DT_E2E, q["data"], q["psi0"], q["labels"], col_ops=col)


@pytest.mark.parametrize("dims, with_col, on_device", [((3, 3), False, False), ((3, 3), False, True), ((2, 2), True, False)])
def test_goal_run_dressed_with_grad(dressing, dims, with_col, on_device):
    from c3_amd import model_learning as ml

    q = _e2e_problem(dims, with_col)
    D = q["D"]
    theta0 = np.array([0.0, 20e6])
    H = q["H_of"](theta0)
    r = ml.goal_run_dressed_with_grad(H, q["hks"], q["sig"], DT_E2E, q["data"], q["psi0"], q["labels"], col_ops_bare=q["col"], device=DEV if on_device else None)
    base = _host_dressed_goal(ml, q, theta0)
    assert np.abs(r["sim_vals"] - base["sim_vals"]).max() < 1e-11
    assert r["goal"] == pytest.approx(base["goal"], rel=1e-7)
    assert list(r["status"]) == [0] * P_E2E and np.asarray(_np(r["grad_H_bare"])).shape == (P_E2E, D, D)
    assert _np(r["grad_hks_bare"]).shape == q["hks"].shape and (r["grad_col_ops_bare"] is None) == (not with_col)
    # 1. the same upstream cotangents through the host VJP, on the device's own T and e
    ops = q["hks"] if not with_col else np.concatenate([q["hks"], q["col"]])
    f = dressing.dress_batch(H, ops)
    assert np.array_equal(f["eigenframe"], _np(r["eigenframe"]))
    g_ops = _np(r["grad_hks"]) if not with_col else np.concatenate([_np(r["grad_hks"]), _np(r["grad_col_ops"])], 1)
    gH = _np(r["grad_H_bare"])
    gA = _np(r["grad_hks_bare"]) if not with_col else np.concatenate([_np(r["grad_hks_bare"]), _np(r["grad_col_ops_bare"])])
    worst, sum_ref, sum_bound = 0.0, 0.0, 0.0
    for p in range(P_E2E):
        kw = dict(grad_ops=g_ops[p], grad_h0=_np(r["grad_h0"])[p])
        ref = dr.dress_vjp_ref(f["transform"][p], f["eigenframe"][p], ops, **kw)
        worst = max(worst, np.linalg.norm(gH[p] - ref["grad_H"]) / (8 * D * EPS * dr.vjp_bound(f["transform"][p], f["eigenframe"][p], ops, **kw)))
        sum_ref = sum_ref + ref["grad_ops"]
        sum_bound = sum_bound + 8 * D * EPS * dr.vjp_bound_ops(f["transform"][p], g_ops[p])
    worst_A = max(np.linalg.norm(gA[m] - sum_ref[m]) / sum_bound[m] for m in range(len(ops)))
    print(f"end to end {dims} col={with_col} device={on_device}: ratios to the VJP bounds: grad_H_bare {worst:.2e}, bare operators {worst_A:.2e}")
    assert worst <= 1.0 and worst_A <= 1.0
    # 2. exact parameter gradients with constant derivative matrices, against central differences on host-dressed operators
    got = ml.model_param_grads(r["grad_H_bare"], r["grad_hks_bare"], dh0=q["G"])
    fd = np.zeros(2)
    for t, h in enumerate((1e5, 1e5)):  # Hz: truncation (2 pi h N dt)^2 ~ 1e-8 relative, (h / detuning)^2 ~ 3e-8 for the coupling
        e = np.eye(2)[t] * h
        fd[t] = (_host_dressed_goal(ml, q, theta0 + e)["goal"] - _host_dressed_goal(ml, q, theta0 - e)["goal"]) / (2 * h)
    print(f"end to end {dims} col={with_col}: d goal / d (f_0, g) = {got}, central differences {fd}, max diff {np.abs(got - fd).max():.3e} (bar {1e-6 * np.abs(fd).max():.3e})")
    assert np.abs(got - fd).max() <= 1e-6 * np.abs(fd).max()
    assert np.abs(fd).min() > 1e-4 * np.abs(fd).max()  # both parameters move the goal well above the bar


def test_sensitivity_sweep_dressed_equals_the_host_route(dressing):
    from c3_amd import model_learning as ml

    q = _e2e_problem((3, 3), False)
    one = {g: s[0] for g, s in q["sig"].items()}
    vals = np.linspace(-3e6, 3e6, 7)
    H_of = lambda v: q["H_of"](np.array([v, 20e6]))[0]
    Tr = lambda v: workloads.dressing_transform(H_of(v))
    want = ml.sensitivity_sweep(lambda v: workloads.dress(H_of(v), Tr(v)), lambda v: np.stack([workloads.dress(A, Tr(v)) for A in q["hks"]]), vals, one, DT_E2E, q["data"][0],
                                q["psi0"], q["labels"])
    for dev in (None, DEV):
        got = ml.sensitivity_sweep_dressed(H_of, q["hks"], vals, one, DT_E2E, q["data"][0], q["psi0"], q["labels"], device=dev)
        assert np.array_equal(got["values"], vals)
        assert np.abs(got["sim_vals"] - want["sim_vals"]).max() < 1e-11
        assert np.abs(got["goals"] - want["goals"]).max() < 1e-7 * max(1.0, np.abs(want["goals"]).max())
    assert np.ptp(want["goals"]) > 0
