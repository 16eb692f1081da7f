"""The device chain of a flux line on the CPU: the numpy restatement (tests/signal_chain_ref.py) pinned to the reference's
stored tunable-coupler signal, its two convolution forms against each other, its vector-Jacobian product against central
differences, and the host side of `c3p_synth_chain` (slot tables, packing, host-pointer checks)."""
import ctypes
import os
import re

import numpy as np
import pytest

import signal_chain_ref as ref
from c3_amd import _lib
from c3_amd import signals as sg
from oracle import c3_oracle as o
from test_signals import tunable_coupler_flux_component

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_PI = 2 * np.pi


@pytest.fixture(scope="module")
def tc(golden_dir):
    z = np.load(golden_dir + "/tunable_coupler.npz")
    return {k: z[k] for k in ("tc_signal", "tc_ts", "tc_awg_I", "tc_awg_Q")}


def _tc_values(I, Q, ts, **kw):
    return ref.chain_from_iq(I, Q, ref.TC_LO_FREQ, ts, ref.KIND_FLUX, 1.0, ref.TC_RISE_TIME, ref.TC_GRID[3], ref.TC_LINE, **kw)[0]


def test_restatement_reproduces_tunable_coupler_signal(tc):
    """test/test_tunable_coupler.py:430-446 compares the TC line's signal with the pickle; here from the stored AWG I/Q.
    Measured 1.04e-13 max|tc_signal|; without the Response stage the same input is 7.2e-2 away."""
    want = tc["tc_signal"]
    assert ref.response_tap_count(ref.TC_RISE_TIME, ref.TC_GRID[3]) == 30 and ref.response_tap_count(0.01e-9, 100e9) == 0
    got = _tc_values(tc["tc_awg_I"], tc["tc_awg_Q"], tc["tc_ts"])
    assert got.shape == (10000,) and got[0] == 0.0
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max()
    plain = ref.chain_from_iq(tc["tc_awg_I"], tc["tc_awg_Q"], ref.TC_LO_FREQ, tc["tc_ts"], ref.KIND_FLUX, line=ref.TC_LINE)[0]
    assert np.abs(plain - want).max() > 1e-2 * np.abs(want).max()


def test_restatement_from_envelope_row(tc):
    t0, t1, awg_res, sim_res = ref.TC_GRID
    r = ref.generate_chain_signal([tunable_coupler_flux_component()], ref.TC_LO_FREQ, t0, t1, awg_res, sim_res, ref.KIND_FLUX, 1.0, ref.TC_RISE_TIME, ref.TC_LINE)
    assert np.abs(r["ts"] - tc["tc_ts"]).max() == 0.0
    assert np.abs(r["values"] - tc["tc_signal"]).max() < 1e-12 * np.abs(tc["tc_signal"]).max()


def test_fft_form_equals_direct_form(tc):
    """The literal zero-padded FFT product (tf_utils.py:476-518) is the causal FIR with one sample of delay."""
    h = ref.response_taps(ref.TC_RISE_TIME, 100e9)
    assert h.shape == (30,) and abs(h.sum() - 1.0) < 1e-15
    for x in (o.dac_nearest(tc["tc_awg_I"], 10000), o.dac_nearest(tc["tc_awg_Q"], 10000)):
        a, b = ref.fir_fft(x, h), ref.fir_direct(x, h)
        assert b[0] == 0.0 and np.abs(a - b).max() < 1e-14 * max(np.abs(x).max(), 1.0)
    assert np.abs(_tc_values(tc["tc_awg_I"], tc["tc_awg_Q"], tc["tc_ts"], conv=ref.fir_fft) - _tc_values(tc["tc_awg_I"], tc["tc_awg_Q"], tc["tc_ts"])).max() < 1e-14 * np.abs(tc["tc_signal"]).max()
    # more taps than samples
    rng = np.random.default_rng(3)
    x, h = rng.normal(size=64), ref.response_taps(1e-9, 100e9)
    assert h.shape == (100,) and np.abs(ref.fir_fft(x, h) - ref.fir_direct(x, h)).max() < 1e-14


def _rel(fd, an):
    return abs(fd - an) / abs(fd)


@pytest.mark.parametrize("N,Na,M", [(700, 16, 30), (64, 3, 100)])
@pytest.mark.parametrize("kind", [ref.KIND_FLUX, ref.KIND_DRIVE])
def test_restatement_vjp_matches_finite_differences(N, Na, M, kind):
    """Transposed FIR, F' and the line parameters against central differences at step 1e-6 (bar 1e-7 relative, as
    tests/test_signals.py:190; measured 1.2e-9 for I/Q, 4.8e-9 for phi)."""
    rng = np.random.default_rng(11)
    sim_res = 100e9
    ts = o.create_ts(0.0, (N + 0.5) / sim_res, sim_res)  # the sample count is a truncation (devices.py:72-84)
    assert ts.shape[0] == N
    rise = (M + 0.5) / sim_res
    assert ref.response_tap_count(rise, sim_res) == M
    I, Q, gs = rng.normal(size=Na), rng.normal(size=Na), rng.normal(size=N)
    lo, v = 0.8e9 * TWO_PI, 1e9 * TWO_PI
    line = dict(ref.TC_LINE)
    f = lambda I_=I, Q_=Q, lo_=lo, v_=v, line_=line: float(np.sum(gs * ref.chain_from_iq(I_, Q_, lo_, ts, kind, v_, rise, sim_res, line_)[0]))
    gI, gQ, gcar, gline = ref.chain_from_iq_vjp(I, Q, lo, ts, gs, kind, v, rise, sim_res, line)
    h = 1e-6
    # Directional differences along sign(gradient) * weights: F is ~5e10 rad/s, so f carries rounding of ~1e-16 * 5e10 * sqrt(N)
    # and a difference over 2h resolves ~1e2 rad/s -- 1e-8 of a typical entry (1e10), but not 1e-7 of an entry that happens
    # to cancel to 1e-3 of it.  Along these directions every entry adds up with the same sign.
    for wts in (np.ones(Na), rng.uniform(0.5, 1.5, size=Na)):
        vI, vQ = np.sign(gI) * wts, np.sign(gQ) * wts
        assert _rel((f(I_=I + h * vI) - f(I_=I - h * vI)) / (2 * h), gI @ vI) < 1e-7
        assert _rel((f(Q_=Q + h * vQ) - f(Q_=Q - h * vQ)) / (2 * h), gQ @ vQ) < 1e-7
    # LO frequency: a step that turns the last sample's phase by 1e-4 rad (these grids are 0.64 and 7 ns long: the 1e2 rad/s
    # of tests/test_signals.py:191 would move f by less than its rounding); truncation ~1e-8 / 6
    hw = 1e-4 / ts[-1]
    assert _rel((f(lo_=lo + hw) - f(lo_=lo - hw)) / (2 * hw), gcar["lo_freq"]) < 1e-7
    if kind == ref.KIND_DRIVE:
        assert _rel((f(v_=v * (1 + h)) - f(v_=v * (1 - h))) / (2 * h * v), gcar["v_to_hz"]) < 1e-7
        assert all(gline[key] == 0.0 for key in ref.LINE_KEYS)
    else:
        assert gcar["v_to_hz"] == 0.0
        for key in ref.LINE_KEYS:
            # omega_0 and anhar are ~1e10 rad/s: the step scales with them
            step = h * max(1.0, abs(line[key]))
            fd = (f(line_=dict(line, **{key: line[key] + step})) - f(line_=dict(line, **{key: line[key] - step}))) / (2 * step)
            assert _rel(fd, gline[key]) < 1e-7, (key, fd, gline[key])


def test_restatement_envelope_vjp_is_the_oracles():
    """Without Response and FluxTuning the chain vjp is oracle.generate_signal_vjp."""
    T = 12e-9
    comps = [dict(shape=o.ENV_GAUSSIAN_NONORM, amp=0.4, xy_angle=0.3, freq_offset=-50e6 * TWO_PI, delta=0.7, t_final=T, sigma=T / 4, use_t_before=True, drag=True)]
    gs = np.random.default_rng(5).normal(size=1200)
    want, wcar = o.generate_signal_vjp(comps, 5e9 * TWO_PI, 1e9 * TWO_PI, 0.0, T, 2.4e9, 100e9, gs)
    got, gcar, _ = ref.generate_chain_signal_vjp(comps, 5e9 * TWO_PI, 0.0, T, 2.4e9, 100e9, gs, ref.KIND_DRIVE, 1e9 * TWO_PI)
    for key in want[0]:
        assert abs(got[0][key] - want[0][key]) <= 1e-14 * abs(want[0][key])
    for key in wcar:
        assert abs(gcar[key] - wcar[key]) <= 1e-14 * abs(wcar[key])


def test_line_tables_match_header():
    text = open(os.path.join(ROOT, "include", "c3prop.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (C3P_LINE_[A-Z_0-9]+) (\d+)", text)}
    want = {"C3P_LINE_KIND_" + n.upper(): i for n, i in sg.LINE_KINDS.items()}
    want.update({"C3P_LINE_" + n.upper(): i for n, i in sg.LINE_SLOTS.items()})
    want.update({"C3P_LINE_NKINDS": len(sg.LINE_KINDS), "C3P_LINE_NPAR": sg.LINE_NPAR})
    assert defs == want
    assert sorted(sg.LINE_SLOTS.values()) == list(range(sg.LINE_NPAR))
    assert (sg.LINE_KINDS["drive"], sg.LINE_KINDS["flux"]) == (ref.KIND_DRIVE, ref.KIND_FLUX)
    assert set(ref.LINE_KEYS) | {"rise_time"} == set(sg.LINE_SLOTS)


def test_pack_lines():
    kinds, par = sg.pack_lines([{"kind": "drive"}, dict(ref.TC_LINE, kind="flux", rise_time=np.array([0.3e-9, 0.5e-9]))], B=2, sim_res=100e9)
    assert kinds.dtype == np.int32 and kinds.tolist() == [0, 1] and par.shape == (2, 2, sg.LINE_NPAR)
    assert np.all(par[:, 0] == 0.0) and par[1, 1, sg.LINE_SLOTS["rise_time"]] == 0.5e-9 and par[0, 1, sg.LINE_SLOTS["d"]] == 0.36
    assert sg.response_tap_count(0.3e-9, 100e9) == 30 and sg.response_tap_count(0.01e-9, 100e9) == 0
    with pytest.raises(_lib.C3PropError, match="C3:Error.*kind"):
        sg.pack_lines([{"kind": "coupling"}])
    with pytest.raises(_lib.C3PropError, match="C3:Error.*rise_time"):
        sg.pack_lines([{"kind": "drive", "rise_time": 0.01e-9}], sim_res=100e9)
    with pytest.raises(_lib.C3PropError, match="C3:Error.*wobble"):
        sg.pack_lines([{"kind": "drive", "wobble": 1.0}])
    with pytest.raises(_lib.C3PropError, match="C3:Error.*phi_0"):
        sg.pack_lines([{"kind": "flux", "phi": 1.0, "omega_0": 1.0, "anhar": 1.0}])


def _host_call(lib, vjp, kinds, par):
    """c3p_synth_chain[_vjp] on host pointers, K = 1, one rect component, 1 ns at 100 GS/s; -> (return code, message)."""
    env, shapes = sg.pack_components([[dict(shape="rect", amp=1.0, t_final=1e-9)]])
    car = np.array([[[5e9 * TWO_PI, 1.0]]])
    kinds = np.asarray(kinds, dtype=np.int32)
    p = lambda a: a.ctypes.data
    sig, genv, gcar, gline = np.zeros((1, 1, 100)), np.zeros_like(env), np.zeros_like(car), np.zeros((1, 1, sg.LINE_NPAR))
    head = (p(env), p(shapes), p(car), p(kinds), p(par), 0.0, 1e-9, 2.4e9 * 5, 100e9, 1, 1, 1, _lib.HOST_PTRS)
    rc = lib.c3p_synth_chain_vjp(*head, p(sig), p(genv), p(gcar), p(gline), None) if vjp else lib.c3p_synth_chain(*head, None, p(sig), None)
    return rc, lib.c3p_last_error().decode()


@pytest.mark.parametrize("vjp", [False, True])
def test_host_pointer_checks(lib, vjp):
    """An unknown kind and a rise_time too short for one tap are refused before any device work (no GPU needed)."""
    par = np.zeros((1, 1, sg.LINE_NPAR))
    rc, msg = _host_call(lib, vjp, [2], par)
    assert rc != 0 and "line_kind[0]=2" in msg
    with pytest.raises(_lib.C3PropError, match="C3:Error"):
        _lib.check(rc)
    par[0, 0, sg.LINE_SLOTS["rise_time"]] = 0.01e-9
    rc, msg = _host_call(lib, vjp, [0], par)
    assert rc != 0 and "rise_time" in msg and "no Response tap" in msg
    par[0, 0, sg.LINE_SLOTS["rise_time"]] = 0.0
    rc, msg = _host_call(lib, vjp, [1], par)
    assert rc != 0 and "phi_0" in msg


@pytest.mark.parametrize("vjp", [False, True])
def test_drive_entries_check_shape_ids_before_any_device_work(lib, vjp):
    """c3p_synth_signals[_vjp] on host pointers refuse an unknown shape id by its own message, with no GPU present: the look
    at env_shapes comes before the workspace lock, as in the chain and table entries."""
    env, shapes = sg.pack_components([[dict(shape="rect", amp=1.0, t_final=1e-9)]])
    shapes[0, 0] = 12
    car = np.array([[[5e9 * TWO_PI, 1.0]]])
    p = lambda a: a.ctypes.data
    sig, genv, gcar = np.zeros((1, 1, 100)), np.zeros_like(env), np.zeros_like(car)
    head = (p(env), p(shapes), p(car), 0.0, 1e-9, 2.4e9 * 5, 100e9, 1, 1, 1, _lib.HOST_PTRS)
    rc = lib.c3p_synth_signals_vjp(*head, p(sig), p(genv), p(gcar), None) if vjp else lib.c3p_synth_signals(*head, None, p(sig), None)
    msg = lib.c3p_last_error().decode()
    assert rc != 0 and "env_shapes[0]=12 is not a C3P_ENV_* id" in msg
