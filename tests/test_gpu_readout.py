"""c3p_readout_goal / c3p_readout_goal_vjp through the C ABI against the long-double restatement of tests/readout_ref.py.

Shapes: D = 2, 3, 6 (dims (3,2)), 9 with kets (M = D) and density vectors (M = D^2, 81 at D = 9); S = 1 and one below, at and one
above the boundaries of the kernels' sequence split -- a workgroup of the element-wise kernels serves SEQ_BLOCK sequences, the
per-set sums stride over the S V values with REDUCE_THREADS; both numbers are read from c3_amd/readout.py -- P = 1, 3, 5; confusion
and rescale shared, per set and absent; one label, a repeated label, none (V = R); every estimator; host and device pointers.

The bar: every output's error, relative to its largest magnitude in the case, is at most 8 e_cpu, where e_cpu is the error of
the float64 run of the same restatement against the long-double one, the worst over the cases of that estimator, never below one
unit roundoff.  8 is the project's margin for a route whose operation order differs from the CPU's (tests/test_gpu_pwc_extended.py).
The measured ratios are printed before they are asserted.
"""
import ctypes as C

import numpy as np
import pytest

from tests import readout_ref as rr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
LD = np.longdouble
FACTOR = 8.0
UNIT = float(np.finfo(np.float64).eps) / 2
QUANTITIES = ("sim", "raw", "goals", "x_bar", "conf_bar", "rescale_bar")


@pytest.fixture(scope="module")
def ro(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from c3_amd import readout

    return readout


def shapes(ro):
    """(D, density, P, S, conf, rescale, labels): every S boundary, D, P and mode at least once."""
    B, T = ro.SEQ_BLOCK, ro.REDUCE_THREADS
    return [
        (2, 0, 1, 1, "none", "none", "one"),
        (2, 1, 3, B - 1, "shared", "shared", "none"),
        (3, 0, 3, B, "perset", "perset", "one"),
        (3, 1, 5, B + 1, "shared", "perset", "repeated"),
        (6, 0, 3, 2 * B - 1, "perset", "shared", "none"),
        (6, 1, 1, 2 * B, "none", "shared", "one"),
        (6, 0, 5, 2 * B + 1, "shared", "none", "repeated"),
        (9, 0, 3, T - 1, "shared", "shared", "one"),
        (9, 1, 3, B + 1, "perset", "perset", "none"),
        (3, 0, 1, T, "none", "perset", "one"),
        (2, 0, 3, T + 1, "perset", "shared", "repeated"),
        (9, 1, 5, 1, "none", "none", "none"),
        (2, 1, 1, T // 2, "shared", "none", "none"),  # V = 2: S V = REDUCE_THREADS
        (3, 0, 3, T // 3, "none", "none", "none"),  # V = 3: S V = REDUCE_THREADS - 1
        (3, 1, 3, T // 3 + 1, "none", "shared", "none"),  # S V = REDUCE_THREADS + 2
    ]


_cache = {}


def case(ro, i):
    if ("case", i) not in _cache:
        _cache[("case", i)] = rr.make_case(100 + i, *shapes(ro)[i])
    return _cache[("case", i)]


def references(ro, name):
    """Long-double results of every case of this estimator and e_cpu per output; computed once."""
    if name not in _cache:
        refs, e_cpu = [], {q: UNIT for q in QUANTITIES}
        for i in range(len(shapes(ro))):
            c = case(ro, i)
            # the inputs keep s (1 - s) away from its poles
            assert c["sim64"].min() >= 0.05 and c["sim64"].max() <= 0.95, (i, c["sim64"].min(), c["sim64"].max())
            hi, lo = rr.run_case(c, name, LD), rr.run_case(c, name, np.float64)
            refs.append(hi)
            for q in QUANTITIES:
                e_cpu[q] = max(e_cpu[q], float(np.max(np.abs(lo[q] - hi[q])) / np.max(np.abs(hi[q]))))
        _cache[name] = (refs, e_cpu)
    return _cache[name]


def run(ro, c, name, vjp=True, device=False, sets=None, want_pop_bar=False):
    """One call through the C ABI.  `sets`: a slice of the parameter sets to compute alone."""
    from c3_amd import _lib

    lib = _lib.load()
    P0 = c["x"].shape[0]
    sl = slice(0, P0) if sets is None else sets
    x = c["x"][sl]
    P, S, M = x.shape
    D, R, V = c["D"], c["R"], c["V"]
    conf, cstride = c["conf"], 0
    if conf is not None and conf.ndim == 3:
        conf, cstride = conf[sl], R * D
    rescale, rstride = None, 0
    if c["scale"] is not None:
        if np.ndim(c["scale"]):
            rescale, rstride = np.stack([c["scale"][sl], c["offset"][sl]], -1), 2
        else:
            rescale = np.array([c["scale"], c["offset"]])
    ins = {"x": x, "conf": conf, "lw": c["label_w"], "rescale": rescale, "meas": c["meas"][sl], "stds": c["stds"][sl], "shots": c["shots"][sl],
           "gw": c["weights"][sl]}
    outs = {"sim": (P, S, V), "raw": (P, S, V), "goals": (P,)}
    if vjp:
        outs.update({"x_bar": (P, S, M), "conf_bar": (P, R, D), "rescale_bar": (P, 2)})
        if want_pop_bar:
            outs["pop_bar"] = (P, S, D)
    if device:
        ins = {k: None if v is None else torch.as_tensor(np.ascontiguousarray(v), device=DEV) for k, v in ins.items()}
        bufs = {k: torch.full(s, float("nan"), dtype=torch.complex128 if k == "x_bar" else torch.float64, device=DEV) for k, s in outs.items()}
        ptr = lambda a: None if a is None else a.data_ptr()
        stream = torch.cuda.current_stream().cuda_stream
    else:
        ins = {k: None if v is None else np.ascontiguousarray(v) for k, v in ins.items()}
        bufs = {k: np.full(s, np.nan, dtype=np.complex128 if k == "x_bar" else np.float64) for k, s in outs.items()}
        ptr = lambda a: None if a is None else a.ctypes.data
        stream = None
    flags = 0 if device else _lib.HOST_PTRS
    head = (ptr(ins["x"]), P, S, M, D, ptr(ins["conf"]), cstride, R, ptr(ins["lw"]), ptr(ins["rescale"]), rstride, ptr(ins["meas"]), ptr(ins["stds"]),
            ptr(ins["shots"]), ro.ESTIMATORS[name])
    if vjp:
        rc = lib.c3p_readout_goal_vjp(*head, ptr(ins["gw"]), flags, ptr(bufs["sim"]), ptr(bufs["raw"]), ptr(bufs["goals"]), ptr(bufs["x_bar"]),
                                      ptr(bufs["conf_bar"]), ptr(bufs["rescale_bar"]), ptr(bufs.get("pop_bar")), stream)
    else:
        rc = lib.c3p_readout_goal(*head, flags, ptr(bufs["sim"]), ptr(bufs["raw"]), ptr(bufs["goals"]), stream)
    _lib.check(rc)
    if device:
        torch.cuda.synchronize()
        bufs = {k: v.cpu().numpy() for k, v in bufs.items()}
    return bufs


def case_ids(n=15):
    return list(range(n))


@pytest.mark.parametrize("name", rr.ESTIMATORS)
@pytest.mark.parametrize("i", case_ids())
def test_readout_against_long_double(ro, name, i):
    from c3_amd import _lib

    assert len(shapes(ro)) == len(case_ids())
    c = case(ro, i)
    refs, e_cpu = references(ro, name)
    ref = refs[i]
    got = run(ro, c, name, device=True)
    assert _lib.last_kernel() == "readout_vjp"
    detail = _lib.last_kernel_detail()
    assert "c3p_readout.hip" in detail and "readout_vjp_kernel" in detail and "readout_goal_kernel" in detail, detail
    worst = {}
    for q in QUANTITIES:
        err = float(np.max(np.abs(got[q] - ref[q])) / np.max(np.abs(ref[q])))
        worst[q] = err / e_cpu[q]
    print(f"\nREADOUT {name} case={i} {shapes(ro)[i]} " + " ".join(f"{q}: e_device/e_cpu={worst[q]:.3g} (e_cpu={e_cpu[q]:.2e})" for q in QUANTITIES))
    for q in QUANTITIES:
        assert np.all(np.isfinite(got[q])), q
        assert worst[q] <= FACTOR, (q, worst[q], e_cpu[q])
    # density vectors: the cotangent is exactly zero off the entries n (D + 1), and real on them
    if c["x"].shape[-1] != c["D"]:
        mask = np.ones(c["x"].shape[-1], dtype=bool)
        mask[:: c["D"] + 1] = False
        assert np.all(got["x_bar"][..., mask] == 0)
        assert np.all(got["x_bar"].imag == 0)
    # the same call again: the same bits; host pointers: the same bits as device pointers
    again = run(ro, c, name, device=True)
    host = run(ro, c, name, device=False)
    for q in QUANTITIES:
        assert np.array_equal(got[q], again[q]), q
        assert np.array_equal(got[q], host[q]), q
    # the forward entry: the same bits as the forward outputs of the reverse entry
    fwd = run(ro, c, name, vjp=False, device=True)
    assert _lib.last_kernel() == "readout"
    for q in ("sim", "raw", "goals"):
        assert np.array_equal(fwd[q], got[q]), q
    # the last set alone: the same bits as inside the batch
    P = c["x"].shape[0]
    alone = run(ro, c, name, device=True, sets=slice(P - 1, P))
    for q in QUANTITIES:
        assert np.array_equal(alone[q][0], got[q][P - 1]), q


def test_pop_bar_output_and_python_layer(ro):
    """pop_bar_out against the restatement, and `readout_goal_vjp` (numpy and tensors) against the raw calls, row cotangents included."""
    i, name = 4, "neg_loglkh_gauss"
    c = case(ro, i)
    refs, e_cpu = references(ro, name)
    got = run(ro, c, name, device=True, want_pop_bar=True)
    err = float(np.max(np.abs(got["pop_bar"] - refs[i]["pop_bar"])) / np.max(np.abs(refs[i]["pop_bar"])))
    assert err <= FACTOR * e_cpu["x_bar"], (err, e_cpu["x_bar"])  # x_bar = 2 pop_bar x: the same error class
    data = {"results": c["meas"], "results_std": c["stds"], "shots": c["shots"]}
    rd = ro.Readout(conf_rows=c["rows"], meas_scale=c["scale"], meas_offset=c["offset"], dims=c["dims"])
    rows_want = rr.confusion_rows_bar(c["rows"], refs[i]["conf_bar"], LD)
    for dev in (False, True):
        x = torch.as_tensor(c["x"], device=DEV) if dev else c["x"]
        r = ro.readout_goal_vjp(x, rd, data, None, name, c["weights"], dim=c["D"])
        h = lambda a: a.cpu().numpy() if dev else a
        assert (not dev) or r["x_bar"].is_cuda
        assert np.array_equal(h(r["sim"]), got["sim"]) and np.array_equal(h(r["goals"]), got["goals"]) and np.array_equal(h(r["x_bar"]), got["x_bar"])
        assert np.array_equal(h(r["grad_meas_scale"]), got["rescale_bar"][:, 0]) and np.array_equal(h(r["grad_meas_offset"]), got["rescale_bar"][:, 1])
        for g, w in zip(r["grad_conf_rows"], rows_want):
            assert np.allclose(h(g), w.astype(np.float64), rtol=0, atol=FACTOR * e_cpu["conf_bar"] * c["D"] * float(np.max(np.abs(refs[i]["conf_bar"]))))
        f = ro.readout_goal(x, rd, data, None, name, dim=c["D"])
        assert np.array_equal(h(f["goals"]), got["goals"]) and np.array_equal(h(f["sim_raw"]), got["raw"])
    # label tuples resolve to the same weights as indices
    c1 = case(ro, 2)
    d1 = {"results": c1["meas"][..., 0], "results_std": c1["stds"][..., 0], "shots": c1["shots"][..., 0]}
    rd1 = ro.Readout(conf_rows=c1["rows"], meas_scale=c1["scale"], meas_offset=c1["offset"], dims=c1["dims"])
    a = ro.readout_goal(c1["x"], rd1, d1, [1], "rms_dist")
    b = ro.readout_goal(c1["x"], rd1, d1, [(1,)], "rms_dist")
    assert a["sim"].shape == c1["meas"].shape[:2] and np.array_equal(a["sim"], b["sim"]) and np.array_equal(a["goals"], b["goals"])


def test_refusals_launch_nothing(ro):
    from c3_amd import _lib
    from c3_amd._lib import C3PropError

    lib = _lib.load()
    c = case(ro, 2)  # D = 3 kets, per-set confusion (R = 2) and rescale, one label
    run(ro, c, "g_LL_prime", device=False)
    before = _lib.last_kernel_detail()
    P, S, M = c["x"].shape
    D, R = c["D"], c["R"]
    rescale = np.ascontiguousarray(np.stack([c["scale"], c["offset"]], -1))
    keep = [np.ascontiguousarray(a) for a in (c["x"], c["conf"], c["label_w"], c["meas"], c["stds"], c["shots"], c["weights"])]
    x, conf, lw, meas, stds, shots, gw = keep
    sim, raw, goals, xb = np.empty((P, S)), np.empty((P, S)), np.empty(P), np.empty((P, S, M), dtype=np.complex128)
    p = lambda a: a.ctypes.data

    def fwd(M=M, D=D, R=R, est=0, sim_p=p(sim), goals_p=p(goals), conf_p=p(conf)):
        return lib.c3p_readout_goal(p(x), P, S, M, D, conf_p, R * D, R, p(lw), p(rescale), 2, p(meas), p(stds), p(shots), est, _lib.HOST_PTRS, sim_p, p(raw), goals_p, None)

    def bwd(M=M, D=D, R=R, est=0, sim_p=p(sim), goals_p=p(goals), xb_p=p(xb)):
        return lib.c3p_readout_goal_vjp(p(x), P, S, M, D, p(conf), R * D, R, p(lw), p(rescale), 2, p(meas), p(stds), p(shots), est, p(gw), _lib.HOST_PTRS, sim_p, p(raw),
                                        goals_p, xb_p, None, None, None, None)

    for call in (fwd, bwd):
        for kw, msg in (({"M": D + 1}, "neither D=3 .* nor D\\^2=9"), ({"R": 0}, "R=0"), ({"D": 1, "M": 1}, "2 <= D"), ({"sim_p": None}, "NULL sim_out"),
                        ({"goals_p": None}, "NULL sim_out / goals_out"), ({"est": 7}, "unknown estimator id 7"), ({"est": -1}, "unknown estimator id -1")):
            with pytest.raises(C3PropError, match=msg):
                _lib.check(call(**kw))
            assert _lib.last_kernel_detail() == before
    with pytest.raises(C3PropError, match="NULL x_bar_out"):
        _lib.check(bwd(xb_p=None))
    with pytest.raises(C3PropError, match="without a confusion matrix R must be D"):
        _lib.check(fwd(conf_p=None))
    assert _lib.last_kernel_detail() == before
    _lib.check(fwd())
    assert _lib.last_kernel_detail() != before
