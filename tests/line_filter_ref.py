"""Line filters, DC offset and crosstalk in numpy, and their vector-Jacobian product.

Restated from the reference: c3/utils/tf_utils.py:439-473 tf_convolve, c3/generator/devices.py:705-731 StepFuncFilter.process,
:735-751 ExponentialIIR, :755-769 HighpassExponential, :773-787 SkinEffectResponse, :646-701 ResponseFFT, :1039-1059 DC_Offset,
:225-292 Crosstalk.  What stands round them (AWG, DAC, the legacy Response, Mixer, VoltsToHertz | FluxTuning) is
tests/signal_chain_ref.py and tests/sampled_envelope_ref.py.

The convolution is held three times: `tf_convolve`, the literal zero-padded FFT product; `conv_direct`, the causal sum
y[n] = sum_{m <= n} h[m] x[n-m] that this product is (the form the device kernel is written to); and `conv_ld`, the same sum in
long double, which with the step responses evaluated in long double (`stage_taps(..., ld=True)`) is what the other two are
measured against.

A stage is a dict: {"kind": "exp_iir", "time_iir", "amp"}, {"kind": "highpass_exp", "time_hp"}, {"kind": "skin_effect", "alpha"},
{"kind": "response_fft", "rise_time"}.
"""
import numpy as np

import sampled_envelope_ref as senv
import signal_chain_ref as chain
from oracle import c3_oracle as o

LD = np.longdouble
STEP_KINDS = ("exp_iir", "highpass_exp", "skin_effect")
# the differentiated parameters of each kind (response_fft: none, its tap count is a floor)
STAGE_PARAMS = {"exp_iir": ("time_iir", "amp"), "highpass_exp": ("time_hp",), "skin_effect": ("alpha",), "response_fft": ()}


# ------------------------------------------------------------------------------------------------ convolution
def tf_convolve(sig: np.ndarray, resp: np.ndarray) -> np.ndarray:
    """tf_utils.py:456-473: [sig, 0_M] and [resp, 0_N] multiplied in the Fourier domain, the first N samples.  Complex, as
    there; the callers take the real part (devices.py:694-695, :728)."""
    sig, resp = np.asarray(sig, dtype=np.complex128), np.asarray(resp, dtype=np.complex128)
    n, m = sig.shape[0], resp.shape[0]
    sig_pad = np.concatenate([sig, np.zeros(m, dtype=np.complex128)])
    resp_pad = np.concatenate([resp, np.zeros(n, dtype=np.complex128)])
    return np.fft.ifft(np.fft.fft(sig_pad) * np.fft.fft(resp_pad))[:n]


def conv_fft(x, h):
    return tf_convolve(x, h).real


def conv_direct(x, h):
    """y[n] = sum_{m=0..n} h[m] x[n-m]"""
    return np.convolve(x, h)[: x.shape[0]]


def conv_ld(x, h):
    """`conv_direct` accumulated in long double, m ascending"""
    x, h = np.asarray(x, dtype=LD), np.asarray(h, dtype=LD)
    N = x.shape[0]
    y = np.zeros(N, dtype=LD)
    for m in range(min(h.shape[0], N)):
        if h[m] != 0:
            y[m:] += h[m] * x[: N - m]
    return y


# ------------------------------------------------------------------------------------------------ long-double erfc
def erfc_ld(x):
    """erfc in long double, a few eps_ld relative (pinned to mpmath by tests/test_line_filters.py).  |x| < 2: 1 - erf with the
    all-positive series erf x = 2/sqrt(pi) e^{-x^2} sum_n 2^n x^(2n+1) / (1 3 .. (2n+1)); |x| >= 2: the continued fraction
    sqrt(pi) e^{x^2} erfc x = 1 / (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...)))), evaluated from a fixed depth upwards;
    erfc(-x) = 2 - erfc(x)."""
    x = np.atleast_1d(np.asarray(x, dtype=LD))
    a = np.abs(x)
    out = np.zeros(a.shape, dtype=LD)
    sqrt_pi = np.sqrt(4 * np.arctan(LD(1)))
    small = a < 2
    if small.any():
        z = a[small]
        term = z.copy()
        s = z.copy()
        for n in range(1, 200):
            term = term * 2 * z * z / (2 * n + 1)
            s = s + term
        out[small] = 1 - 2 / sqrt_pi * np.exp(-z * z) * s
    big = ~small & np.isfinite(a)
    if big.any():
        z = a[big]
        f = z.copy()
        for k in range(400, 0, -1):
            f = z + (LD(k) / 2) / f
        out[big] = np.exp(-z * z) / sqrt_pi / f
    return np.where(x < 0, 2 - out, out)


def _erfc(x, ld):
    if ld:
        return erfc_ld(x)
    from math import erfc

    return np.array([erfc(float(v)) for v in np.atleast_1d(x)])


# ------------------------------------------------------------------------------------------------ impulse responses
def step_response(stage, ts, ld=False):
    """step_response_function of the three kinds; ts in the precision asked for"""
    t = np.asarray(ts, dtype=LD if ld else np.float64)
    c = (lambda v: LD(v)) if ld else float
    kind = stage["kind"]
    if kind == "exp_iir":
        return 1 + c(stage["amp"]) * np.exp(-t / c(stage["time_iir"]))  # devices.py:750
    if kind == "highpass_exp":
        return np.exp(-t / c(stage["time_hp"]))  # devices.py:769
    if kind == "skin_effect":
        with np.errstate(divide="ignore"):
            return _erfc(c(stage["alpha"]) / 21 / np.sqrt(np.abs(t)), ld)  # devices.py:787
    raise ValueError(kind)


def step_response_der(stage, ts):
    """{parameter: d s / d parameter at ts}"""
    t = np.asarray(ts, dtype=np.float64)
    kind = stage["kind"]
    if kind == "exp_iir":
        e = np.exp(-t / stage["time_iir"])
        return {"time_iir": stage["amp"] * e * t / stage["time_iir"] ** 2, "amp": e}
    if kind == "highpass_exp":
        return {"time_hp": np.exp(-t / stage["time_hp"]) * t / stage["time_hp"] ** 2}
    q = 21 * np.sqrt(np.abs(t))
    return {"alpha": -2 / np.sqrt(np.pi) * np.exp(-((stage["alpha"] / q) ** 2)) / q}


def response_fft_taps(rise_time: float, sim_res: float) -> np.ndarray:
    """devices.py:675-689: as the legacy Response but centred at (rise_time - dt) / 2"""
    M = int(np.floor(rise_time * sim_res))
    ts = np.linspace(0.0, rise_time, M)
    cen = (rise_time - 1 / sim_res) / 2
    sigma = rise_time / 4
    r = np.exp(-((ts - cen) ** 2) / (2 * sigma * sigma)) - np.exp(-((-1 - cen) ** 2) / (2 * sigma * sigma))
    return r / np.sum(r)


def stage_taps(stage, ts, sim_res, ld=False):
    """impulse response of a stage on the signal's own time grid (StepFuncFilter.process, devices.py:720-723: the step
    response at ts, a zero in front, first differences); response_fft: its M taps, formed in double"""
    if stage["kind"] == "response_fft":
        h = response_fft_taps(stage["rise_time"], sim_res)
        return np.asarray(h, dtype=LD) if ld else h
    s = step_response(stage, ts, ld)
    s = np.concatenate([np.zeros(1, dtype=s.dtype), s])
    return s[1:] - s[:-1]


def apply_stage(x, stage, ts, sim_res, conv=conv_direct):
    return conv(x, stage_taps(stage, ts, sim_res, ld=conv is conv_ld))


def dc_offset(values, offset_amp):
    return values + offset_amp  # devices.py:1057


def crosstalk(matrix, signals):
    """devices.py:287-291 over all lines: signals [K,N] -> matrix [K,K] @ signals"""
    return np.asarray(matrix) @ np.asarray(signals)


# ------------------------------------------------------------------------------------------------ one line, and its vjp
def line_from_iq(inph, quad, lo_freq, ts, sim_res, stages=(), dc=0.0, kind=chain.KIND_DRIVE, v_to_hz=1.0, rise_time=0.0, line=None, conv=conv_direct):
    """DAC -> legacy Response (rise_time > 0) -> stages -> Mixer -> + dc -> V->Hz | FluxTuning.
    -> (values [N], [(I, Q) read by stage 0, .., by stage F-1, by the mixer])"""
    N = ts.shape[0]
    I, Q = o.dac_nearest(inph, N), o.dac_nearest(quad, N)
    if rise_time > 0:
        h = chain.response_taps(rise_time, sim_res)
        I, Q = chain.fir_direct(I, h), chain.fir_direct(Q, h)
    bufs = [(I, Q)]
    for st in stages:
        I, Q = apply_stage(I, st, ts, sim_res, conv), apply_stage(Q, st, ts, sim_res, conv)
        bufs.append((I, Q))
    t = ts.astype(I.dtype)
    mixed = np.cos(lo_freq * t) * I + np.sin(lo_freq * t) * Q + dc
    if kind == chain.KIND_DRIVE:
        return mixed * v_to_hz, bufs
    return chain.flux_freq(line["phi"] + mixed, line) - chain.flux_freq(line["phi"], line), bufs


def generate(components, lo_freq, t_start, t_end, awg_res, sim_res, **kw):
    """One line from its components (closed-form or table shapes): values [N]"""
    ts_awg, ts = o.create_ts(t_start, t_end, awg_res), o.create_ts(t_start, t_end, sim_res)
    inph, quad = senv.awg_iq(components, ts_awg, t_start)
    return line_from_iq(inph, quad, lo_freq, ts, sim_res, **kw)[0]


def generate_vjp(components, lo_freq, t_start, t_end, awg_res, sim_res, gsig, stages=(), dc=0.0, kind=chain.KIND_DRIVE, v_to_hz=1.0, rise_time=0.0, line=None):
    """d loss / d values [N] (before the crosstalk) -> (per-component dicts, carrier dict, line dict, per-stage dicts, d/d dc)"""
    ts_awg, ts = o.create_ts(t_start, t_end, awg_res), o.create_ts(t_start, t_end, sim_res)
    N, Na = ts.shape[0], ts_awg.shape[0]
    inph, quad = senv.awg_iq(components, ts_awg, t_start)
    _, bufs = line_from_iq(inph, quad, lo_freq, ts, sim_res, stages, dc, kind, v_to_hz, rise_time, line)
    I, Q = bufs[-1]
    cs, sn = np.cos(lo_freq * ts), np.sin(lo_freq * ts)
    mixed = cs * I + sn * Q + dc
    gline = dict.fromkeys(chain.LINE_KEYS, 0.0)
    if kind == chain.KIND_DRIVE:
        gm = gsig * v_to_hz
        gv = float(np.sum(gsig * mixed))
    else:
        A = line["omega_0"] - line["anhar"]
        f1, du1, dd1, u1 = chain._flux_parts(line["phi"] + mixed, line)
        f0, du0, dd0, u0 = chain._flux_parts(line["phi"], line)
        k = np.pi / line["phi_0"]
        gm = gsig * A * du1 * k
        gv = 0.0
        gline["phi"] = float(np.sum(gsig * A * k * (du1 - du0)))
        gline["phi_0"] = float(np.sum(gsig * A * (du0 * u0 - du1 * u1))) / line["phi_0"]
        gline["omega_0"] = float(np.sum(gsig * (f1 - f0)))
        gline["anhar"] = float(np.sum(gsig * (f0 - f1)))
        gline["d"] = float(np.sum(gsig * A * (dd1 - dd0)))
    gcar = {"lo_freq": float(np.sum(gm * ts * (cs * Q - sn * I))), "v_to_hz": gv}
    gdc = float(np.sum(gm))
    gc, gs = gm * cs, gm * sn
    gstages = [None] * len(stages)
    for f in range(len(stages) - 1, -1, -1):
        st = stages[f]
        xI, xQ = bufs[f]
        # gh[m] = sum_{n >= m} gy[n] x[n-m]
        gh = (np.convolve(gc[::-1], xI)[:N] + np.convolve(gs[::-1], xQ)[:N])[::-1]
        g = {}
        if st["kind"] in STEP_KINDS:
            for key, ds in step_response_der(st, ts).items():
                ds = np.concatenate([[0.0], ds])
                g[key] = float(np.sum(gh * (ds[1:] - ds[:-1])))
        gstages[f] = g
        h = stage_taps(st, ts, sim_res)
        # gx[j] = sum_{n >= j} h[n-j] gy[n]
        gc, gs = np.convolve(gc[::-1], h)[:N][::-1], np.convolve(gs[::-1], h)[:N][::-1]
    if rise_time > 0:
        h = chain.response_taps(rise_time, sim_res)
        gc, gs = chain.fir_direct_T(gc, h), chain.fir_direct_T(gs, h)
    gI, gQ = np.zeros(Na), np.zeros(Na)
    idx = chain._grid(N, Na)
    np.add.at(gI, idx, gc)
    np.add.at(gQ, idx, gs)
    gcomp = []
    for comp in components:
        if comp["shape"] in senv.TAB_NAMES:
            gcomp.append(senv.component_vjp(comp, ts_awg - (t_start + comp.get("delay", 0.0)), gI, gQ))
        else:
            gcomp.append(chain.awg_iq_vjp([comp], ts_awg, t_start, gI, gQ)[0])
    return gcomp, gcar, gline, gstages, gdc
