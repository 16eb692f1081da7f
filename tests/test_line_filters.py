"""Line filters, DC offset and crosstalk on the host: the numpy restatement (tests/line_filter_ref.py) against the reference's
stored ResponseFFT signal, its three convolution routes against each other, its vjp against differences of its long-double
forward, and the Python tables and packers of c3_amd.signals.  No GPU."""
import os
import re

import numpy as np
import pytest

import line_filter_ref as ref
from c3_amd import signals as sg
from c3_amd._lib import C3PropError
from oracle import c3_oracle as o

TWO_PI = 2 * np.pi


# ------------------------------------------------------------------------------------------------ golden ResponseFFT
def flattop_cut(t, t_up, t_down, risefall):
    """envelopes.py:282-302"""
    from math import erf

    shape = np.array([erf((x - t_up) / risefall) * erf((-x + t_down) / risefall) for x in t])
    shape = np.clip(shape, 0, 1)
    return shape / shape.max()


def transmon_flux_iq():
    """AWG samples of test/test_transmon_expanded.py:127-155: flattop_cut, amp 0.3, on 5 AWG samples of 1 ns"""
    T, awg_res = 1e-9, 5e9
    ts_awg = o.create_ts(0.0, T, awg_res)
    env = o.envelope_mask(ts_awg, T, T) * flattop_cut(ts_awg, 0.2e-9, 0.96e-9, 0.2e-9)
    return 0.3 * env, np.zeros_like(env)


@pytest.mark.parametrize("q", ["q1", "q2"])
def test_response_fft_reproduces_the_stored_transmon_signal(golden_dir, q):
    """sim_res 20e9, awg_res 5e9, T = 1 ns: N = 20, Na = 5, M = floor(0.3e-9 * 20e9) = 6 taps; LO frequency 0, no V->Hz.
    Bound 1e-14 (the literal route lands at 1.6e-15); with the legacy sign of 1/sim_res in the centre it misses by 0.05."""
    g = np.load(golden_dir + "/transmon_expanded.npz")
    sim_res = 20e9
    ts = o.create_ts(0.0, 1e-9, sim_res)
    assert ts.shape == (20,) and np.abs(ts - g["ts_" + q]).max() == 0.0
    inph, quad = transmon_flux_iq()
    h = ref.response_fft_taps(0.3e-9, sim_res)
    assert h.shape == (6,)
    I = ref.tf_convolve(o.dac_nearest(inph, 20), h).real
    Q = ref.tf_convolve(o.dac_nearest(quad, 20), h).real
    sig = np.cos(0.0 * ts) * I + np.sin(0.0 * ts) * Q
    err = np.abs(sig - g["sig_" + q]).max()
    print(f"ResponseFFT vs sig_{q}: {err:.3e}")
    assert err < 1e-14
    # the same through the whole-line restatement, direct sum
    sig2, _ = ref.line_from_iq(inph, quad, 0.0, ts, sim_res, stages=[{"kind": "response_fft", "rise_time": 0.3e-9}])
    assert np.abs(sig2 - g["sig_" + q]).max() < 1e-14
    # the legacy centre is another filter
    legacy = ref.chain.response_taps(0.3e-9, sim_res)
    assert np.abs(ref.conv_direct(o.dac_nearest(inph, 20), legacy) - g["sig_" + q]).max() > 0.01


# ------------------------------------------------------------------------------------------------ the three routes
def _test_signal(N, seed):
    """a flux-pulse-like row: a flattop with a little noise, max about 0.3"""
    rng = np.random.default_rng(seed)
    t = (np.arange(N) + 0.5) / N
    from math import erf

    x = 0.3 * np.array([(1 + erf((u - 0.1) / 0.03)) * (1 + erf((0.85 - u) / 0.03)) / 4 for u in t])
    return x + 1e-3 * rng.normal(size=N)


STAGES = {
    "exp_iir": {"kind": "exp_iir", "time_iir": 7e-9, "amp": -0.12},
    "highpass_exp": {"kind": "highpass_exp", "time_hp": 40e-9},
    "skin_effect": {"kind": "skin_effect", "alpha": 2.5e-4},
    "response_fft": {"kind": "response_fft", "rise_time": 0.305e-9},
}


@pytest.mark.parametrize("N", [300, 2000, 10000])
@pytest.mark.parametrize("kind", list(STAGES))
def test_literal_and_direct_routes_against_long_double(kind, N):
    """tf_convolve and the direct sum, taps formed in double, against the long-double sum over taps formed in long double:
    1e-13 max|y| (measured 1-3e-16 absolute at max|y| about 0.3; the rest is room for the step response's own rounding, about
    sqrt(N) eps)."""
    sim_res = 100e9
    ts = o.create_ts(0.0, (N + 0.5) / sim_res, sim_res)
    assert ts.shape == (N,)
    x = _test_signal(N, N)
    st = STAGES[kind]
    want = ref.apply_stage(x, st, ts, sim_res, ref.conv_ld)
    assert want.dtype == ref.LD
    top = float(np.abs(want).max())
    for name, conv in (("fft", ref.conv_fft), ("direct", ref.conv_direct)):
        err = float(np.abs(ref.apply_stage(x, st, ts, sim_res, conv) - want).max())
        print(f"{kind} N={N} {name}: {err:.3e} absolute, max|y| = {top:.3f}")
        assert err <= 1e-13 * top, (name, err, top)


def test_erfc_ld_against_mpmath():
    """The long-double erfc behind the skin-effect reference.  A step response lies in [0, 2] and the taps are its differences,
    so what the reference needs is the absolute error: 4 eps_ld (1 - erf below 2 rounds at the size of 1, not of erfc).  From
    2 on, where the continued fraction runs, also the relative error: (8 + 2 x^2) eps_ld, x^2 eps_ld being what rounding x^2
    costs exp(-x^2)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    xs = np.concatenate([np.linspace(0.0, 2.0, 41), np.linspace(2.0, 12.0, 41), [1e-8, 1e-3, 25.0], -np.linspace(0.1, 5.0, 9)])
    got = ref.erfc_ld(xs)
    eps = float(np.finfo(ref.LD).eps)
    worst_abs = worst_rel = 0.0
    for x, gv in zip(xs, got):
        want = mp.erfc(mp.mpf(float(x)))
        err = abs(mp.mpf(float(gv)) + mp.mpf(float(gv - ref.LD(float(gv)))) - want)
        worst_abs = max(worst_abs, float(err) / eps)
        assert err <= 4 * eps, (x, float(err) / eps)
        if x >= 2:
            worst_rel = max(worst_rel, float(err / want) / ((8 + 2 * x * x) * eps))
            assert err / want <= (8 + 2 * x * x) * eps, (x, float(err / want) / eps)
    print(f"erfc_ld vs mpmath: worst absolute error {worst_abs:.2f} eps_ld; from 2 on, worst relative error / bar {worst_rel:.2f}")


# ------------------------------------------------------------------------------------------------ vjp of the restatement
def test_restated_vjp_against_differences_of_the_long_double_forward():
    """Every stage parameter, the offset and one envelope amplitude of a two-stage flux line: the analytic vjp against central
    differences of sum(g * values) with the stages convolved in long double.  Steps of 1e-4 relative: the truncation error is
    about h^2 = 1e-8 and the rounding eps_ld / h = 1e-15; bar 1e-6."""
    N, Na, sim_res = 400, 9, 100e9
    t1 = (N + 0.5) / sim_res
    awg_res = (Na + 0.5) / t1
    rng = np.random.default_rng(5)
    comp = dict(shape=o.ENV_FLATTOP, amp=0.7, t_final=t1, t_up=0.4e-9, t_down=3.2e-9, risefall=0.3e-9, xy_angle=0.3, freq_offset=2e7 * TWO_PI)
    line = dict(ref.chain.TC_LINE)
    stages = [dict(STAGES["exp_iir"], time_iir=1.5e-9), {"kind": "skin_effect", "alpha": 1.2e-4}, {"kind": "highpass_exp", "time_hp": 9e-9}]
    kw = dict(kind=ref.chain.KIND_FLUX, rise_time=0.3e-9, line=line)
    lo, dc = 0.8e9 * TWO_PI, 0.05
    g = rng.normal(size=N)
    gcomp, gcar, gline, gst, gdc = ref.generate_vjp([comp], lo, 0.0, t1, awg_res, sim_res, g, stages=stages, dc=dc, **kw)

    def loss(comp=comp, stages=stages, dc=dc):
        v = ref.generate([comp], lo, 0.0, t1, awg_res, sim_res, stages=stages, dc=dc, conv=ref.conv_ld, **kw)
        return np.sum(np.asarray(g, dtype=ref.LD) * v)

    def fd(f, x0):
        h = 1e-4 * abs(x0)
        return (f(x0 + h) - f(x0 - h)) / (2 * h)

    checks = [("amp", gcomp[0]["amp"], fd(lambda v: loss(comp=dict(comp, amp=v)), comp["amp"])), ("dc", gdc, fd(lambda v: loss(dc=v), dc))]
    for f, st in enumerate(stages):
        for key in ref.STAGE_PARAMS[st["kind"]]:
            with_v = lambda v, f=f, key=key: loss(stages=[dict(s, **{key: v}) if i == f else s for i, s in enumerate(stages)])
            checks.append((f"stage{f}.{key}", gst[f][key], fd(with_v, st[key])))
    for name, got, want in checks:
        print(f"{name}: {got:.9e} (differences {want:.9e})")
        assert abs(got - want) < 1e-6 * abs(want), name


def test_crosstalk_and_offset_restatement():
    """Crosstalk.process on the reference's own test matrix (test/test_crosstalk.py): [[1,0],[1,0]] makes both lines equal"""
    s = np.arange(12.0).reshape(2, 6)
    out = ref.crosstalk([[1, 0], [1, 0]], s)
    assert np.array_equal(out[0], s[0]) and np.array_equal(out[1], s[0])
    assert np.array_equal(ref.dc_offset(s[0], 0.5), s[0] + 0.5)


# ------------------------------------------------------------------------------------------------ Python tables and packers
def test_filter_tables_match_header():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "c3prop.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+C3P_FILT_(\w+)\s+(\d+)", hdr)}
    for name, idx in sg.FILT_KINDS.items():
        assert defs[name.upper()] == idx, name
    assert defs["NKINDS"] == len(sg.FILT_KINDS)
    for name, idx in sg.FILT_SLOTS.items():
        assert defs[name.upper()] == idx, name
    assert defs["NPAR"] == sg.FILT_NPAR == len(sg.FILT_SLOTS)
    from c3_amd import _lib

    for entry in ("c3p_synth_filt", "c3p_synth_filt_vjp"):
        assert entry in _lib.SIGNATURES and re.search(r"\bint " + entry + r"\(", hdr)
    # the new entries take the arguments of the table entries plus the five (and three) new ones
    assert len(_lib.SIGNATURES["c3p_synth_filt"][1]) == len(_lib.SIGNATURES["c3p_synth_tab"][1]) + 5
    assert len(_lib.SIGNATURES["c3p_synth_filt_vjp"][1]) == len(_lib.SIGNATURES["c3p_synth_tab_vjp"][1]) + 8


def test_pack_line_filters_layout():
    lines = [[{"kind": "response_fft", "rise_time": 0.3e-9}, {"kind": "exp_iir", "time_iir": [5e-9, 6e-9, 7e-9], "amp": -0.1}],
             [{"kind": "skin_effect", "alpha": 2e-4}]]
    kinds, par = sg.pack_line_filters(lines, B=3, sim_res=100e9)
    assert kinds.dtype == np.int32 and kinds.tolist() == [[0, 1], [3, -1]]
    assert par.shape == (3, 2, 2, sg.FILT_NPAR) and par.dtype == np.float64
    assert np.all(par[:, 0, 0] == [0.3e-9, 0.0])
    assert par[:, 0, 1, 0].tolist() == [5e-9, 6e-9, 7e-9] and np.all(par[:, 0, 1, 1] == -0.1)
    assert np.all(par[:, 1, 0] == [2e-4, 0.0]) and np.all(par[:, 1, 1] == 0.0)
    k2, p2 = sg.pack_line_filters([[{"kind": "highpass_exp", "time_hp": 3e-8}], []])
    assert k2.tolist() == [[2], [-1]] and p2[0, 0, 0, 0] == 3e-8
    k0, p0 = sg.pack_line_filters([[], []], B=2)
    assert k0.shape == (2, 0) and p0.shape == (2, 2, 0, sg.FILT_NPAR)


@pytest.mark.parametrize("lines, text", [
    ([[{"kind": "lowpass", "tau": 1e-9}]], "filter kind"),
    ([[{"kind": "exp_iir", "time_iir": 1e-9}]], "needs 'amp'"),
    ([[{"kind": "exp_iir", "time_iir": 1e-9, "amp": 0.1, "alpha": 1.0}]], "takes no parameter"),
    ([[{"kind": "highpass_exp", "time_hp": 0.0}]], "positive"),
    ([[{"kind": "exp_iir", "time_iir": -1e-9, "amp": 0.1}]], "positive"),
    ([[{"kind": "exp_iir", "time_iir": 1e-9, "amp": np.inf}]], "finite"),
    ([[{"kind": "skin_effect", "alpha": np.nan}]], "finite"),
    ([[{"kind": "response_fft", "rise_time": 0.001e-9}]], "no tap"),
    ([[{"kind": "highpass_exp", "time_hp": [1e-9, 2e-9]}]], "scalar or"),
])
def test_pack_line_filters_refusals(lines, text):
    with pytest.raises(C3PropError, match="C3:Error.*" + re.escape(text)):
        sg.pack_line_filters(lines, B=1, sim_res=100e9)


def test_pack_crosstalk_layout_and_refusals():
    m = sg.pack_crosstalk(["d1", "TC", "d2"], ["d2", "d1"], [[1.0, 0.2], [0.3, 0.9]])
    assert m.tolist() == [[0.9, 0.0, 0.3], [0.0, 1.0, 0.0], [0.2, 0.0, 1.0]]
    assert np.array_equal(sg.pack_crosstalk(["a", "b"], [], np.zeros((0, 0))), np.eye(2))
    # Crosstalk.process on the lines it names, the others untouched
    s = np.arange(15.0).reshape(3, 5)
    want = s.copy()
    want[[2, 0]] = np.array([[1.0, 0.2], [0.3, 0.9]]) @ s[[2, 0]]
    assert np.allclose(ref.crosstalk(m, s), want, rtol=0, atol=1e-15)
    for args, text in ((( ["a", "b"], ["a", "c"], np.eye(2)), "is not a line"), ((["a", "b"], ["a"], np.eye(2)), "must be"),
                       ((["a", "b"], ["a", "a"], np.eye(2)), "twice")):
        with pytest.raises(C3PropError, match="C3:Error.*" + text):
            sg.pack_crosstalk(*args)
