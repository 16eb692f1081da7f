"""Sampled and Fourier pulse envelopes in numpy (float64), and their vector-Jacobian product.

Restated from the reference: c3/libraries/envelopes.py:31-34 pwc, :37-68 pwc_shape, :104-125 pwc_symmetric, :142-168
fourier_sin, :171-191 fourier_cos; tfp.math.interp_regular_1d_grid with fill_value_below = fill_value_above = 0; the mask and
the t_before offset of c3/signal/pulse.py:98-141; the sum over components of c3/signal/gates.py:341-370.  What follows the AWG
(DAC, Response, Mixer, VoltsToHertz | FluxTuning) is tests/signal_chain_ref.py.

A component is a dict keyed like the reference's `Envelope.params`.  `shape` is one of TAB_NAMES here, or an oracle ENV_* id
for a closed-form component, which goes to oracle.envelope_values.
"""
import numpy as np

import signal_chain_ref as chain
from oracle import c3_oracle as o

TAB_NAMES = ("pwc", "pwc_shape", "pwc_symmetric", "fourier_sin", "fourier_cos")
# the differentiated arrays of each shape
TAB_ARRAYS = {"pwc": ("inphase", "quadrature"), "pwc_shape": ("inphase",), "pwc_symmetric": ("inphase",),
              "fourier_sin": ("amps", "freqs", "phases"), "fourier_cos": ("amps", "freqs")}


def hat_weights(x, x_min, x_max, M):
    """[len(x), M] weights of the M knots of the regular grid x_min .. x_max (both included) in the linear interpolation at x;
    rows of zeros outside [x_min, x_max] (interp_regular_1d_grid with both fill values 0)."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    xi = np.clip((x - x_min) / (x_max - x_min) * (M - 1), 0.0, M - 1.0)
    lo = np.minimum(np.floor(xi).astype(np.int64), M - 2)
    w = xi - lo
    inside = (x >= x_min) & (x <= x_max)
    W = np.zeros((x.shape[0], M))
    rows = np.arange(x.shape[0])
    W[rows, lo] = np.where(inside, 1.0 - w, 0.0)
    W[rows, lo + 1] += np.where(inside, w, 0.0)
    return W


def _mirror(t, t_final):
    return np.where(t > t_final / 2, t_final - t, t)  # envelopes.py:113


def pwc_shape(t, p):
    y = np.asarray(p["inphase"], dtype=np.float64)
    return hat_weights(t, p["t_bin_start"], p["t_bin_end"], y.shape[0]) @ y


def pwc_symmetric(t, p):
    return pwc_shape(_mirror(np.atleast_1d(np.asarray(t, dtype=np.float64)), p["t_final"]), p)


def fourier_sin(t, p):
    a, f, ph = (np.asarray(p[k], dtype=np.float64)[:, None] for k in ("amps", "freqs", "phases"))
    return np.sum(a * np.sin(f * np.atleast_1d(t)[None, :] + ph), axis=0)


def fourier_cos(t, p):
    a, f = (np.asarray(p[k], dtype=np.float64)[:, None] for k in ("amps", "freqs"))
    return np.sum(a * np.cos(f * np.atleast_1d(t)[None, :]), axis=0)


REAL_SHAPES = {"pwc_shape": pwc_shape, "pwc_symmetric": pwc_symmetric, "fourier_sin": fourier_sin, "fourier_cos": fourier_cos}


def _before(ts_off):
    return 2 * ts_off[0] - ts_off[1]  # pulse.py:127


def envelope_values(comp, ts_off):
    """mask * (s(ts) - [use_t_before] s(t_before)), complex (pulse.py:118-141); pwc multiplies the stored pairs with the mask."""
    name = comp["shape"]
    if name not in TAB_NAMES:
        return o.envelope_values(comp, ts_off, comp["t_final"])
    mask = o.envelope_mask(ts_off, comp["t_final"], comp["t_final"])
    if name == "pwc":
        assert not comp.get("use_t_before", False) and len(comp["inphase"]) == ts_off.shape[0]
        return mask * (np.asarray(comp["inphase"], dtype=np.float64) + 1j * np.asarray(comp["quadrature"], dtype=np.float64))
    f = REAL_SHAPES[name]
    offset = f(_before(ts_off), comp)[0] if comp.get("use_t_before", False) else 0.0
    return (mask * (f(ts_off, comp) - offset)).astype(np.complex128)


def _phase(comp, ts_off):
    return np.exp(1j * (comp.get("xy_angle", 0.0) - comp.get("freq_offset", 0.0) * ts_off))


def awg_iq(components, ts_awg, t_start):
    """gates.py:341-370: sum_e amp_e env_e exp(i (xy_e - freq_offset_e tau)), tau = t - (t_start + delay_e)."""
    sig = np.zeros(ts_awg.shape, dtype=np.complex128)
    for comp in components:
        ts_off = ts_awg - (t_start + comp.get("delay", 0.0))
        sig = sig + comp["amp"] * envelope_values(comp, ts_off) * _phase(comp, ts_off)
    return sig.real, sig.imag


def generate(components, lo_freq, t_start, t_end, awg_res, sim_res, kind=chain.KIND_DRIVE, v_to_hz=1.0, rise_time=0.0, line=None):
    """One line from its components through the whole chain: {"values" [N], "inphase" / "quadrature" [Na]}."""
    ts_awg, ts = o.create_ts(t_start, t_end, awg_res), o.create_ts(t_start, t_end, sim_res)
    inph, quad = awg_iq(components, ts_awg, t_start)
    values, _, _ = chain.chain_from_iq(inph, quad, lo_freq, ts, kind, v_to_hz, rise_time, sim_res, line)
    return {"values": values, "inphase": inph, "quadrature": quad}


def component_vjp(comp, ts_off, gI, gQ):
    """Cotangents of one component from those of the AWG I/Q: {"amp", "xy_angle", "freq_offset"} and one array per entry of
    TAB_ARRAYS.  With c_j = amp g_j exp(-i phase_j):  d L / d theta = sum_j mask_j (Re c_j Re ds_j + Im c_j Im ds_j),
    ds_j = d(s_j - s_before) / d theta."""
    name = comp["shape"]
    ph = _phase(comp, ts_off)
    env = envelope_values(comp, ts_off)
    z = comp["amp"] * env * ph
    g = {"amp": float(np.sum(gI * (env * ph).real + gQ * (env * ph).imag)), "xy_angle": float(np.sum(-gI * z.imag + gQ * z.real)),
         "freq_offset": float(np.sum(ts_off * (gI * z.imag - gQ * z.real)))}
    mask = o.envelope_mask(ts_off, comp["t_final"], comp["t_final"])
    c = comp["amp"] * (gI + 1j * gQ) * np.conj(ph) * mask
    before = comp.get("use_t_before", False)
    tb = _before(ts_off)
    if name == "pwc":
        g["inphase"], g["quadrature"] = c.real, c.imag
    elif name in ("pwc_shape", "pwc_symmetric"):
        M = len(comp["inphase"])
        mir = (lambda t: _mirror(np.atleast_1d(t), comp["t_final"])) if name == "pwc_symmetric" else (lambda t: t)
        W = hat_weights(mir(ts_off), comp["t_bin_start"], comp["t_bin_end"], M)
        if before:
            W = W - hat_weights(mir(tb), comp["t_bin_start"], comp["t_bin_end"], M)
        g["inphase"] = c.real @ W
    else:
        a, f = (np.asarray(comp[k], dtype=np.float64)[:, None] for k in ("amps", "freqs"))
        p = np.asarray(comp["phases"], dtype=np.float64)[:, None] if name == "fourier_sin" else np.zeros_like(a)
        times = [(ts_off[None, :], 1.0)] + ([(np.array([[tb]]), -1.0)] if before else [])
        d_a, d_f, d_p = (np.zeros((a.shape[0], ts_off.shape[0])) for _ in range(3))
        for t, sgn in times:
            arg = f * t + p
            if name == "fourier_sin":
                d_a, d_f, d_p = d_a + sgn * np.sin(arg), d_f + sgn * a * t * np.cos(arg), d_p + sgn * a * np.cos(arg)
            else:
                d_a, d_f = d_a + sgn * np.cos(arg), d_f - sgn * a * t * np.sin(arg)
        g["amps"], g["freqs"] = d_a @ c.real, d_f @ c.real
        if name == "fourier_sin":
            g["phases"] = d_p @ c.real
    return g


def generate_vjp(components, lo_freq, t_start, t_end, awg_res, sim_res, gsig, kind=chain.KIND_DRIVE, v_to_hz=1.0, rise_time=0.0, line=None):
    """d loss / d values [N] -> (per-component dicts, carrier dict, line dict).  Closed-form components get the four scalar
    cotangents of signal_chain_ref.awg_iq_vjp."""
    ts_awg, ts = o.create_ts(t_start, t_end, awg_res), o.create_ts(t_start, t_end, sim_res)
    inph, quad = awg_iq(components, ts_awg, t_start)
    gI, gQ, gcar, gline = chain.chain_from_iq_vjp(inph, quad, lo_freq, ts, gsig, kind, v_to_hz, rise_time, sim_res, line)
    out = []
    for comp in components:
        if comp["shape"] in TAB_NAMES:
            out.append(component_vjp(comp, ts_awg - (t_start + comp.get("delay", 0.0)), gI, gQ))
        else:
            out.append(chain.awg_iq_vjp([comp], ts_awg, t_start, gI, gQ)[0])
    return out, gcar, gline
