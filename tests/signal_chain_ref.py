"""The device chain behind a flux line, in numpy (float64): AWG -> DigitalToAnalog -> Response -> Mixer -> VoltsToHertz
or FluxTuning, and its vector-Jacobian product.

Restated from the reference (c3/generator/devices.py:585-642 Response, c3/utils/tf_utils.py:476-518 tf_convolve_legacy,
devices.py:457-525 FluxTuning; DAC, Mixer, LO and VoltsToHertz as in oracle.c3_oracle.generate_signal).  The Response
convolution is held twice: `fir_fft`, the literal zero-padded FFT product with the window [M-1 : N+M-1], and `fir_direct`,
the causal FIR with one sample of delay that this product is, y[n] = sum_{m < min(M, n)} h[m] x[n-1-m] with m ascending --
the form the device kernels are written to.
"""
import numpy as np

from oracle import c3_oracle as o

KIND_DRIVE, KIND_FLUX = 0, 1
LINE_KEYS = ("phi_0", "phi", "omega_0", "anhar", "d")


def response_tap_count(rise_time: float, sim_res: float) -> int:
    """devices.py:614: floor(rise_time * resolution) of the one double product (0.3e-9 * 100e9 floors to 30)."""
    return int(np.floor(rise_time * sim_res))


def response_taps(rise_time: float, sim_res: float) -> np.ndarray:
    """devices.py:614-630: the normalised rise function, M = floor(rise_time * sim_res) samples of a Gaussian centred at
    (rise_time + dt) / 2 with sigma = rise_time / 4, minus its (underflowing) value at t = -1."""
    M = response_tap_count(rise_time, sim_res)
    ts = np.linspace(0.0, rise_time, M)
    cen = (rise_time + 1.0 / sim_res) / 2
    sigma = rise_time / 4
    r = np.exp(-((ts - cen) ** 2) / (2 * sigma * sigma)) - np.exp(-((-1 - cen) ** 2) / (2 * sigma * sigma))
    return r / np.sum(r)


def fir_fft(x: np.ndarray, h: np.ndarray) -> np.ndarray:
    """tf_utils.py:476-518: [0_M, x, 0_M] and [h, 0_{N+M}] multiplied in the Fourier domain, window [M-1 : N+M-1]."""
    N, M = x.shape[0], h.shape[0]
    sig = np.concatenate([np.zeros(M), x, np.zeros(M)]).astype(np.complex128)
    resp = np.concatenate([h, np.zeros(N + M)]).astype(np.complex128)
    conv = np.fft.ifft(np.fft.fft(sig) * np.fft.fft(resp))
    return conv[M - 1 : N + M - 1].real  # devices.py:635-636


def fir_direct(x: np.ndarray, h: np.ndarray) -> np.ndarray:
    """y[n] = sum_{m=0}^{min(M,n)-1} h[m] x[n-1-m], accumulated with m ascending; y[0] = 0."""
    N = x.shape[0]
    y = np.zeros(N)
    for m in range(min(h.shape[0], N - 1)):
        y[m + 1 :] += h[m] * x[: N - 1 - m]
    return y


def fir_direct_T(g: np.ndarray, h: np.ndarray) -> np.ndarray:
    """Transpose of `fir_direct`: gx[i] = sum_m h[m] g[i+1+m]."""
    N = g.shape[0]
    gx = np.zeros(N)
    for m in range(min(h.shape[0], N - 1)):
        gx[: N - 1 - m] += h[m] * g[m + 1 :]
    return gx


def _flux_parts(x, p):
    """(f, df/du, df/dd, u) of f = (cos^2 u + d^2 sin^2 u)^(1/4), u = pi x / phi_0 (devices.py:481-495; d = 0 is the
    branch without d, sqrt|cos u|)."""
    u = np.pi * x / p["phi_0"]
    c, s, d = np.cos(u), np.sin(u), p.get("d", 0.0)
    q = c**2 + d**2 * s**2
    f = np.sqrt(np.sqrt(q))
    with np.errstate(divide="ignore", invalid="ignore"):
        q34 = 0.5 / (f * f * f)  # q^(-3/4) / 2
        return f, q34 * s * c * (d * d - 1.0), q34 * d * s * s, u


def flux_freq(x, p):
    """FluxTuning.get_freq (devices.py:497-502)."""
    return (p["omega_0"] - p["anhar"]) * _flux_parts(x, p)[0] + p["anhar"]


def _grid(N, Na):
    return np.minimum(np.floor((np.arange(N) + 0.5) * (Na / N)).astype(np.int64), Na - 1)  # oracle.dac_nearest


def chain_from_iq(inph, quad, lo_freq, ts, kind=KIND_DRIVE, v_to_hz=1.0, rise_time=0.0, sim_res=None, line=None, conv=fir_direct):
    """DAC -> Response (rise_time > 0) -> Mixer -> V->Hz (kind 0) or FluxTuning (kind 1, devices.py:520-524).
    Returns (values [N], I [N], Q [N]) with I, Q what the mixer reads."""
    N = ts.shape[0]
    I, Q = o.dac_nearest(inph, N), o.dac_nearest(quad, N)
    if rise_time > 0:
        h = response_taps(rise_time, sim_res)
        I, Q = conv(I, h), conv(Q, h)
    mixed = np.cos(lo_freq * ts) * I + np.sin(lo_freq * ts) * Q
    if kind == KIND_DRIVE:
        return mixed * v_to_hz, I, Q
    return flux_freq(line["phi"] + mixed, line) - flux_freq(line["phi"], line), I, Q


def generate_chain_signal(components, lo_freq, t_start, t_end, awg_res, sim_res, kind=KIND_DRIVE, v_to_hz=1.0, rise_time=0.0, line=None):
    """One line from its envelope components (oracle.awg_iq) through the whole chain."""
    ts_awg, ts = o.create_ts(t_start, t_end, awg_res), o.create_ts(t_start, t_end, sim_res)
    inph, quad = o.awg_iq(components, ts_awg, t_start)
    values, _, _ = chain_from_iq(inph, quad, lo_freq, ts, kind, v_to_hz, rise_time, sim_res, line)
    return {"values": values, "ts": ts, "inphase": inph, "quadrature": quad}


def chain_from_iq_vjp(inph, quad, lo_freq, ts, gsig, kind=KIND_DRIVE, v_to_hz=1.0, rise_time=0.0, sim_res=None, line=None):
    """d loss/d values [N] -> (gI [Na], gQ [Na], {"lo_freq", "v_to_hz"}, {phi_0, phi, omega_0, anhar, d}).
    rise_time is not differentiated (the tap count is a floor)."""
    N, Na = ts.shape[0], inph.shape[0]
    idx = _grid(N, Na)
    _, I, Q = chain_from_iq(inph, quad, lo_freq, ts, kind, v_to_hz, rise_time, sim_res, line)
    cs, sn = np.cos(lo_freq * ts), np.sin(lo_freq * ts)
    mixed = cs * I + sn * Q
    gline = dict.fromkeys(LINE_KEYS, 0.0)
    if kind == KIND_DRIVE:
        gm = gsig * v_to_hz
        gv = float(np.sum(gsig * mixed))
    else:
        A = line["omega_0"] - line["anhar"]
        f1, du1, dd1, u1 = _flux_parts(line["phi"] + mixed, line)
        f0, du0, dd0, u0 = _flux_parts(line["phi"], line)
        k = np.pi / line["phi_0"]
        gm = gsig * A * du1 * k
        gv = 0.0
        gline["phi"] = float(np.sum(gsig * A * k * (du1 - du0)))
        gline["phi_0"] = float(np.sum(gsig * A * (du0 * u0 - du1 * u1))) / line["phi_0"]
        gline["omega_0"] = float(np.sum(gsig * (f1 - f0)))
        gline["anhar"] = float(np.sum(gsig * (f0 - f1)))
        gline["d"] = float(np.sum(gsig * A * (dd1 - dd0)))
    gcar = {"lo_freq": float(np.sum(gm * ts * (cs * Q - sn * I))), "v_to_hz": gv}
    gc, gs = gm * cs, gm * sn
    if rise_time > 0:
        h = response_taps(rise_time, sim_res)
        gc, gs = fir_direct_T(gc, h), fir_direct_T(gs, h)
    gI, gQ = np.zeros(Na), np.zeros(Na)
    np.add.at(gI, idx, gc)
    np.add.at(gQ, idx, gs)
    return gI, gQ, gcar, gline


def awg_iq_vjp(components, ts_awg, t_start, gI, gQ):
    """(gI, gQ) at AWG resolution -> d loss/d {amp, xy_angle, freq_offset, delta} per component: the envelope half of
    oracle.generate_signal_vjp (gates.py:341-370 under the tape of optimizer.py:206-216)."""
    out = []
    for comp in components:
        ts_off = ts_awg - (t_start + comp.get("delay", 0.0))
        ph = np.exp(1j * (comp.get("xy_angle", 0.0) - comp.get("freq_offset", 0.0) * ts_off))
        env = o.envelope_values(comp, ts_off, comp["t_final"])
        z = comp["amp"] * env * ph
        g = {"amp": float(np.sum(gI * (env * ph).real + gQ * (env * ph).imag)), "xy_angle": float(np.sum(-gI * z.imag + gQ * z.real)),
             "freq_offset": float(np.sum(ts_off * (gI * z.imag - gQ * z.real))), "delta": 0.0}
        if comp.get("drag", False):
            dz = comp["amp"] * (o.envelope_values(dict(comp, delta=1.0), ts_off, comp["t_final"]) - o.envelope_values(dict(comp, delta=0.0), ts_off, comp["t_final"])) * ph
            g["delta"] = float(np.sum(gI * dz.real + gQ * dz.imag))
        out.append(g)
    return out


def generate_chain_signal_vjp(components, lo_freq, t_start, t_end, awg_res, sim_res, gsig, kind=KIND_DRIVE, v_to_hz=1.0, rise_time=0.0, line=None):
    """(per-component dicts, carrier dict, line dict) for one line."""
    ts_awg, ts = o.create_ts(t_start, t_end, awg_res), o.create_ts(t_start, t_end, sim_res)
    inph, quad = o.awg_iq(components, ts_awg, t_start)
    gI, gQ, gcar, gline = chain_from_iq_vjp(inph, quad, lo_freq, ts, gsig, kind, v_to_hz, rise_time, sim_res, line)
    return awg_iq_vjp(components, ts_awg, t_start, gI, gQ), gcar, gline


# the reference's tunable-coupler flux line (test/test_tunable_coupler.py:36-63,163-182; "Hz 2pi" quantities in rad/s)
TC_LINE = {"phi_0": 10.0, "phi": 10.0 * 0.23, "omega_0": 8.1e9 * 2 * np.pi, "anhar": -286e6 * 2 * np.pi, "d": 0.36}
TC_RISE_TIME = 0.3e-9
TC_LO_FREQ = 829e6 * 2 * np.pi
TC_GRID = (0.0, 100e-9, 2.4e9, 100e9)  # t_start, t_end, awg_res, sim_res
