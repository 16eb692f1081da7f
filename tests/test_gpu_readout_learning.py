"""The read-out model through model learning, end to end on the GPU: a closed qutrit (D = 3, K = 1, N = 40, P = 2, four short
sequences over two gates), the same qutrit with one collapse operator (density vectors, M = 9), and two coupled qutrits from the
bare model (`goal_run_dressed_with_grad`, D = 9, P = 2, N = 20).  For each: the empty read-out against today's epilogue, the
simulated values against a serial numpy loop over tests/readout_ref.py, every gradient against central differences of
`goal_run_batched(..., readout=...)`, per-set read-out parameters, and the sensitivity sweep against its serial loop."""
import functools

import numpy as np
import pytest

from tests import readout_ref as rr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
SYSTEMS = ("closed", "open", "dressed")


@pytest.fixture(scope="module")
def ml(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from c3_amd import model_learning

    return model_learning


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@functools.lru_cache(maxsize=None)
def _system(kind):
    """The model, pulses, sequences and read-out parameters of one of the three systems (no device work)."""
    from c3_amd import workloads

    rng = np.random.default_rng({"closed": 41, "open": 42, "dressed": 43}[kind])
    P = 2
    if kind == "dressed":
        dims, N, dt = (3, 3), 20, 1e-11
        a = workloads.annihilators(dims)
        H_bare = np.stack([workloads.bare_drift(dims, (5.0e9 + 2e6 * p, 5.6e9), (-210e6, -240e6), {(0, 1): 20e6}) for p in range(P)])
        hks = np.stack([x + x.conj().T for x in a])
        ts = (np.arange(N) + 0.5) * dt
        sig = np.stack([[2 * np.pi * 1e9 * rng.uniform(0.5, 0.8) * np.cos(2 * np.pi * (f + 50e6) * ts + rng.uniform(0, 2 * np.pi)) for f in (5.0e9, 5.6e9)] for _ in range(P)])
        sigs = {"rx90p[0]": sig, "ry90p[1]": sig[::-1].copy() * 0.7}
        seqs = [["rx90p[0]"], ["rx90p[0]", "ry90p[1]"], ["ry90p[1]", "rx90p[0]", "ry90p[1]"], ["rx90p[0]", "rx90p[0]", "ry90p[1]"]]
        col, step_hz, unit_hz = None, 1e4, 1e9  # truncation (2 pi h 3 N dt)^2 ~ 1.4e-9 of the largest term, rounding eps |goal| / h ~ 1e-10
        h0 = None
    else:
        dims, N, dt = (3,), 40, 0.5e-9
        a = workloads.annihilators(dims)
        # a qutrit in the frame of its drive: 2 MHz detuning, -200 MHz anharmonicity; 20 ns gates of about a quarter turn
        h0 = 2 * np.pi * np.diag([0.0, 2e6, 2 * 2e6 - 200e6]).astype(np.complex128)
        H_bare = None
        hks = np.stack([a[0] + a[0].conj().T])
        sigs = {g: amp * rng.uniform(0.7, 1.3, size=(P, 1, N)) for g, amp in (("rx90p", 2.0e7), ("ry90p", 1.5e7))}
        seqs = [["rx90p"], ["ry90p", "rx90p"], ["rx90p", "rx90p", "ry90p"], ["ry90p"]]
        col = np.stack([np.sqrt(1 / 50e-9) * a[0]]) if kind == "open" else None
        unit_hz = 1e6
        step_hz = 60.0  # truncation (2 pi h 3 N dt)^2 ~ 5e-10 of the largest term of the derivative (terms cancel), rounding eps |goal| / h ~ 1e-10
    D = int(np.prod(dims))
    psi0 = np.zeros(D, dtype=np.complex128)
    psi0[0] = 1.0
    rows = [np.stack([[0.97, 0.04, 0.06], [0.95, 0.07, 0.03]])[:, :d] + 0.01 * q for q, d in enumerate(dims)]  # [P,d_q], inside the bounds
    scale, offset = np.array([1.03, 0.98]), np.array([-0.01, 0.015])
    return dict(kind=kind, dims=dims, D=D, P=P, N=N, dt=dt, h0=h0, H_bare=H_bare, hks=hks, sigs=sigs, seqs=seqs, col=col, psi0=psi0, rows=rows, scale=scale,
                offset=offset, step_hz=step_hz, unit_hz=unit_hz,
                # the first subsystem excited, the second not: a state index without a confusion matrix, a row of comp_state_labels with one
                labels_plain=[3] if kind == "dressed" else [1], labels_comp=[2] if kind == "dressed" else [1])


def _operators(q):
    """(h0, hks, col) that `goal_run_batched` takes: the dressed ones for the bare model (dressed on the device, once)."""
    if q["kind"] != "dressed":
        return q["h0"], q["hks"], q["col"]
    if "dressed_ops" not in _memo:
        from c3_amd import dressing

        d = dressing.dress_batch(q["H_bare"], q["hks"])
        _memo["dressed_ops"] = (np.asarray(d["h0"]), np.asarray(d["ops"]), None)
    return _memo["dressed_ops"]


_memo = {}


def _labels(q, readout):
    return q["labels_comp"] if (readout is not None and readout.conf_rows is not None) else q["labels_plain"]


def _forward(ml, q, readout, estimator, data, *, labels="default", h0=None, hks=None, device=DEV):
    o = _operators(q)
    return ml.goal_run_batched(o[0] if h0 is None else h0, o[1] if hks is None else hks, q["sigs"], q["dt"], data, q["psi0"], _labels(q, readout) if labels == "default" else labels,
                               device=device, col_ops=o[2], readout=readout, estimator=estimator)


def _with_grad(ml, q, readout, estimator, data, device=DEV):
    if q["kind"] == "dressed":
        return ml.goal_run_dressed_with_grad(q["H_bare"], q["hks"], q["sigs"], q["dt"], data, q["psi0"], _labels(q, readout), device=device, readout=readout, estimator=estimator)
    return ml.goal_run_batched_with_grad(q["h0"], q["hks"], q["sigs"], q["dt"], data, q["psi0"], _labels(q, readout), device=device, col_ops=q["col"], readout=readout,
                                         estimator=estimator)


def _readout(q, per_set=True):
    from c3_amd import readout as ro

    if per_set:
        return ro.Readout(conf_rows=q["rows"], meas_scale=q["scale"], meas_offset=q["offset"], dims=q["dims"])
    return ro.Readout(conf_rows=[r[0] for r in q["rows"]], meas_scale=float(q["scale"][0]), meas_offset=float(q["offset"][0]), dims=q["dims"])


def _data(ml, q, readout, key):
    """Data sets whose results lie 0.01 - 0.02 off the simulated values of this read-out (so that |m - s| is neither zero nor large)."""
    if key not in _memo:
        S = len(q["seqs"])
        dummy = [{"seqs": q["seqs"], "results": np.full(S, 0.5), "results_std": np.full(S, 0.02), "shots": np.full(S, 1000.0)} for _ in range(q["P"])]
        sim = _forward(ml, q, readout, "rms_dist", dummy)["sim_vals"]
        assert sim.min() > 0.05 and sim.max() < 0.95, sim
        off = np.array([[0.02, -0.015, 0.01, -0.02], [-0.01, 0.02, -0.02, 0.015]])
        _memo[key] = [{"seqs": q["seqs"], "results": sim[p] + off[p], "results_std": np.full(S, 0.02), "shots": np.full(S, 1000.0 + 10 * p)} for p in range(q["P"])]
    return _memo[key]


@pytest.mark.parametrize("kind", SYSTEMS)
def test_empty_readout_is_todays_epilogue(ml, kind):
    from c3_amd import readout as ro

    q = _system(kind)
    data = _data(ml, q, None, (kind, "plain"))
    for dev in (None, DEV):
        base = _forward(ml, q, None, "g_LL_prime", data, device=dev)
        got = _forward(ml, q, ro.Readout(), "g_LL_prime", data, device=dev)
        assert set(base) == {"goal", "goals", "sim_vals"} and got["sim_vals_no_rescale"] is None
        assert np.allclose(got["goals"], base["goals"], rtol=1e-12, atol=0)
        assert np.allclose(got["sim_vals"], base["sim_vals"], rtol=1e-12, atol=1e-14)
        assert got["goal"] == pytest.approx(base["goal"], rel=1e-12)
    # and with the gradient: the same goal, the same operator cotangents (two routes to the same values)
    r0 = _with_grad(ml, q, None, "g_LL_prime", data)
    r1 = _with_grad(ml, q, ro.Readout(), "g_LL_prime", data)
    assert "grad_conf_rows" not in r0 and r1["grad_conf_rows"] is None and r1["grad_meas_scale"] is None
    assert np.allclose(r1["goals"], r0["goals"], rtol=1e-12, atol=0)
    key = "grad_H_bare" if kind == "dressed" else "grad_h0"
    g0, g1 = _np(r0[key]), _np(r1[key])
    assert np.allclose(g1, g0, rtol=0, atol=1e-10 * np.max(np.abs(g0)))


@pytest.mark.parametrize("kind", SYSTEMS)
def test_sim_vals_against_serial_loop(ml, kind):
    """The populations of the existing path (no labels: every population is a value), then per set confusion, selection and
    rescale by tests/readout_ref.py."""
    q = _system(kind)
    rd = _readout(q)
    data = _data(ml, q, rd, (kind, "perset"))
    S, D, P = len(q["seqs"]), q["D"], q["P"]
    all_pops = [{"seqs": q["seqs"], "results": np.full((S, D), 0.5), "results_std": np.full((S, D), 0.02), "shots": np.full((S, D), 1000.0)} for _ in range(P)]
    pops = _forward(ml, q, None, "g_LL_prime", all_pops, labels=None)["sim_vals"]
    assert pops.shape == (P, S, D)
    R = 2 ** len(q["dims"])
    w = np.zeros(R)
    np.add.at(w, q["labels_comp"], 1.0)
    want = np.empty((P, S))
    for p in range(P):
        cm = rr.confusion_matrix([r[p] for r in q["rows"]], np.float64)
        want[p] = (cm @ pops[p].T).T @ w * q["scale"][p] + q["offset"][p]
    for dev in (None, DEV):
        got = _forward(ml, q, rd, "g_LL_prime", data, device=dev)
        assert np.allclose(got["sim_vals"], want, rtol=1e-12, atol=1e-14)
        assert np.allclose(got["sim_vals_no_rescale"] * q["scale"][:, None] + q["offset"][:, None], want, rtol=1e-12, atol=1e-14)
        goals = [rr.estimator("g_LL_prime", data[p]["results"], want[p], data[p]["results_std"], data[p]["shots"], np.float64) for p in range(P)]
        # |m - s| >= 0.01 and shots / (s (1 - s)) <= 2.2e4: a relative 1e-12 of s moves the goal by at most ~1e-9 of it
        assert np.allclose(got["goals"], goals, rtol=1e-9, atol=0)


@pytest.mark.parametrize("estimator", ["g_LL_prime", "rms_dist"])
@pytest.mark.parametrize("kind", SYSTEMS)
def test_gradients_against_central_differences(ml, kind, estimator):
    from c3_amd import readout as ro

    q = _system(kind)
    rd = _readout(q)
    data = _data(ml, q, rd, (kind, "perset"))
    r = _with_grad(ml, q, rd, estimator, data)
    assert torch.is_tensor(r["grad_meas_scale"]) and r["grad_meas_scale"].is_cuda  # nothing came back but goals and sim_vals
    rng = np.random.default_rng(7)
    P = q["P"]
    goal = lambda rd_=rd, **kw: _forward(ml, q, rd_, estimator, data, **kw)["goal"]
    assert goal() == pytest.approx(r["goal"], rel=1e-12)
    h = 1e-6
    checks = []
    for k, row in enumerate(q["rows"]):
        E = rng.uniform(-1, 1, size=row.shape)  # |h E| <= 1e-6: every row stays inside its bounds
        mk = lambda s: ro.Readout(conf_rows=[a + s * h * E if j == k else a for j, a in enumerate(q["rows"])], meas_scale=q["scale"], meas_offset=q["offset"])
        checks.append((f"conf_row[{k}]", float(np.sum(_np(r["grad_conf_rows"][k]) * E)), (goal(mk(+1)) - goal(mk(-1))) / (2 * h)))
    for name, key in (("meas_scale", "grad_meas_scale"), ("meas_offset", "grad_meas_offset")):
        E = rng.uniform(-1, 1, size=P)
        mk = lambda s: ro.Readout(conf_rows=q["rows"], meas_scale=q["scale"] + (s * h * E if name == "meas_scale" else 0),
                                  meas_offset=q["offset"] + (s * h * E if name == "meas_offset" else 0))
        checks.append((name, float(np.sum(_np(r[key]) * E)), (goal(mk(+1)) - goal(mk(-1))) / (2 * h)))
    # the (dressed) drift Hamiltonian along a random Hermitian direction, step in Hz; the control Hamiltonians, step 1e-6
    h0, hks, _ = _operators(q)
    D = q["D"]
    herm = lambda: (lambda a: (a + a.conj().T) / 2)(rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D)))
    # The step is sized in Hz (q["step_hz"]); the derivative is quoted per q["unit_hz"] (MHz, GHz for the 0.6 ns sequences) so that
    # it is O(1) and atol = 1e-9 stays the allowance for a vanishing entry, not a loosened rtol.
    E0 = herm()
    unit = q["unit_hz"]
    dh0 = 2 * np.pi * unit * E0
    hu = q["step_hz"] / unit
    an = float(np.sum(np.conj(_np(r["grad_h0"])) * dh0).real)
    checks.append(("h0", an, (goal(h0=h0 + hu * dh0) - goal(h0=h0 - hu * dh0)) / (2 * hu)))
    Ek = np.stack([herm() for _ in range(hks.shape[-3])])
    an = float(np.sum(np.conj(_np(r["grad_hks"])) * Ek).real)
    checks.append(("hks", an, (goal(hks=hks + h * Ek) - goal(hks=hks - h * Ek)) / (2 * h)))
    for what, an, fd in checks:
        print(f"{kind} {estimator} d goal / d {what}: {an:.9e}  central differences {fd:.9e}")
    for what, an, fd in checks:
        assert np.allclose(an, fd, rtol=1e-6, atol=1e-9), (what, an, fd)
        assert abs(fd) > 1e-6, (what, fd)  # the check can fail: a thousand times atol


@pytest.mark.parametrize("kind", SYSTEMS)
def test_per_set_readout_leaves_the_other_set_alone(ml, kind):
    from c3_amd import readout as ro

    q = _system(kind)
    rd = _readout(q)
    data = _data(ml, q, rd, (kind, "perset"))
    rows2 = [r.copy() for r in q["rows"]]
    for r in rows2:
        r[1] = r[1] + np.array([-0.05, 0.03, 0.02])[: r.shape[1]]
    rd2 = ro.Readout(conf_rows=rows2, meas_scale=q["scale"], meas_offset=q["offset"])
    a, b = _with_grad(ml, q, rd, "g_LL_prime", data), _with_grad(ml, q, rd2, "g_LL_prime", data)
    assert np.array_equal(a["goals"][0], b["goals"][0]) and np.array_equal(a["sim_vals"][0], b["sim_vals"][0])
    assert a["goals"][1] != b["goals"][1]
    for k in range(len(rows2)):
        assert np.array_equal(_np(a["grad_conf_rows"][k])[0], _np(b["grad_conf_rows"][k])[0])
    assert np.array_equal(_np(a["grad_meas_scale"])[0], _np(b["grad_meas_scale"])[0])
    assert np.array_equal(_np(a["grad_h0"])[0], _np(b["grad_h0"])[0])
    assert not np.array_equal(_np(a["grad_h0"])[1], _np(b["grad_h0"])[1])


@pytest.mark.parametrize("kind", SYSTEMS)
def test_sensitivity_sweep_with_readout(ml, kind):
    """The sweep (one batch) against the serial loop over `goal_run_batched`, one point at a time, with a shared read-out."""
    from c3_amd import workloads

    q = _system(kind)
    rd = _readout(q, per_set=False)
    data = _data(ml, q, _readout(q), (kind, "perset"))[0]
    one = {g: s[0] for g, s in q["sigs"].items()}
    vals = np.array([-2e5, 0.0, 1e5, 3e5])
    if kind == "dressed":
        n0 = 2 * np.pi * np.kron(np.diag(np.arange(3.0)), np.eye(3))
        H_of = lambda v: q["H_bare"][0] + v * n0
        got = ml.sensitivity_sweep_dressed(H_of, q["hks"], vals, one, q["dt"], data, q["psi0"], q["labels_comp"], device=DEV, readout=rd, estimator="rms_dist")
        from c3_amd import dressing

        def point(v):
            d = dressing.dress_batch(H_of(v)[None], q["hks"])
            return ml.goal_run_batched(d["h0"], d["ops"], {g: s[None] for g, s in one.items()}, q["dt"], [data], q["psi0"], q["labels_comp"], device=DEV, readout=rd, estimator="rms_dist")
    else:
        n0 = 2 * np.pi * np.diag(np.arange(3.0))
        h0_of, hks_of = (lambda v: q["h0"] + v * n0), (lambda v: q["hks"])
        col_of = None if q["col"] is None else (lambda v: q["col"])
        got = ml.sensitivity_sweep(h0_of, hks_of, vals, one, q["dt"], data, q["psi0"], q["labels_comp"], device=DEV, col_ops_of=col_of, readout=rd, estimator="rms_dist")

        def point(v):
            return ml.goal_run_batched(h0_of(v)[None], hks_of(v)[None], {g: s[None] for g, s in one.items()}, q["dt"], [data], q["psi0"], q["labels_comp"], device=DEV,
                                       col_ops=None if q["col"] is None else q["col"][None], readout=rd, estimator="rms_dist")
    want = [point(v) for v in vals]
    assert np.array_equal(got["values"], vals)
    assert np.allclose(got["sim_vals"], np.concatenate([w["sim_vals"] for w in want]), rtol=1e-12, atol=1e-14)
    # rms_dist: |m - s| ~ 0.01 - 0.02 against s <= 1, a relative 1e-12 of s is at most 1e-10 of the goal
    assert np.allclose(got["goals"], np.concatenate([w["goals"] for w in want]), rtol=1e-9, atol=0)
    assert np.ptp(got["goals"]) > 0
