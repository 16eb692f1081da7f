"""On-device control-signal synthesis -- host side of `c3p_synth_signals`.

The reference builds each drive-line signal through the generator chain LO + AWG ->
DigitalToAnalog -> Mixer -> VoltsToHertz (c3/generator/generator.py:172-229 `generate_signals`,
devices.py:72-122,203-221,306-351,914-939,1073-1195; envelopes via Instruction.get_awg_signal
c3/signal/gates.py:341-370 and Envelope / EnvelopeDrag c3/signal/pulse.py:88-180).  Here a batch
is described by B x K x E envelope-parameter rows and the B x K x N samples are produced in HBM,
where `propagate_batch` consumes them without a host round trip.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from ._cache import TensorMemo
from ._lib import C3PropError
from .propagation import _Call, _is_torch, _ptr

# shape ids / parameter slots: include/c3prop.h (a test checks these against the header)
ENV_SHAPES = {
    "no_drive": 0,
    "rect": 1,
    "gaussian_nonorm": 2,
    "flattop": 3,
    "flattop_risefall": 4,
    "cosine": 5,
    "gaussian_sigma": 6,
    "gaussian": 7,
    "trapezoid": 8,
}
ENV_SLOTS = {
    "amp": 0,
    "xy_angle": 1,
    "freq_offset": 2,
    "delta": 3,
    "t_final": 4,
    "sigma": 5,
    "t_up": 6,
    "t_down": 7,
    "risefall": 8,
    "delay": 9,
    "flags": 10,
}
ENV_NPAR = 12
# shapes whose parameters are an array of coefficients: they read a block of the coefficient table that travels with the
# rows (C3P_ENVT_* of include/c3prop.h; `pack_table_components`, `synthesize_signals(env_tables=, table_index=)`)
TAB_SHAPES = {"pwc": 16, "pwc_shape": 17, "pwc_symmetric": 18, "fourier_sin": 19, "fourier_cos": 20}
# the block of each: scalars first, then arrays of M doubles each, in this order
TAB_LAYOUT = {
    "pwc": ((), ("inphase", "quadrature")),
    "pwc_shape": (("t_bin_start", "t_bin_end"), ("inphase",)),
    "pwc_symmetric": (("t_bin_start", "t_bin_end"), ("inphase",)),
    "fourier_sin": ((), ("amps", "freqs", "phases")),
    "fourier_cos": ((), ("amps", "freqs")),
}
_TAB_NAMES = {v: k for k, v in TAB_SHAPES.items()}
_TAB_KEYS = frozenset(k for sc, ar in TAB_LAYOUT.values() for k in sc + ar)
ENVF_T_BEFORE = 1
ENVF_DRAG = 2
# what follows the mixer on a line, and the per-line parameter row of `c3p_synth_chain` (C3P_LINE_* of include/c3prop.h)
LINE_KINDS = {"drive": 0, "flux": 1}
LINE_SLOTS = {"rise_time": 0, "phi_0": 1, "phi": 2, "omega_0": 3, "anhar": 4, "d": 5}
LINE_NPAR = 6
# distortion stages between DAC and Mixer and their parameter slots (C3P_FILT_* of include/c3prop.h; `pack_line_filters`)
FILT_KINDS = {"response_fft": 0, "exp_iir": 1, "highpass_exp": 2, "skin_effect": 3}
FILT_SLOTS = {"tau": 0, "amp": 1}
FILT_NPAR = 2
# the reference's parameter names per kind -> slot (devices.py:651, :741-743, :761, :786)
_FILT_KEYS = {
    "response_fft": {"rise_time": "tau"},
    "exp_iir": {"time_iir": "tau", "amp": "amp"},
    "highpass_exp": {"time_hp": "tau"},
    "skin_effect": {"alpha": "tau"},
}


def slice_num(t_start: float, t_end: float, resolution: float) -> int:
    """Device.calc_slice_num (devices.py:72-84)."""
    return int(abs(t_start - t_end) * resolution)


def pack_components(channels: Sequence[Sequence[Dict]], B: int = 1):
    """Envelope components per drive line -> (env_params [B,K,E,NPAR], env_shapes [K,E]).

    `channels[k]` lists the envelope components of line k as dicts keyed like the reference's
    `Envelope.params` (amp, xy_angle, freq_offset, delta, t_final, sigma, t_up, t_down, risefall)
    plus `shape` (a name from the envelope library), `use_t_before`, `drag`, `delay`.  A value may be
    a scalar (shared by the batch) or an array of B per-sample values.
    """
    K = len(channels)
    E = max(1, max(len(c) for c in channels))
    env = np.zeros((B, K, E, ENV_NPAR), dtype=np.float64)
    shapes = np.full((K, E), -1, dtype=np.int32)
    for k, comps in enumerate(channels):
        for e, comp in enumerate(comps):
            name = comp["shape"]
            if name not in ENV_SHAPES:
                raise C3PropError(f"C3:Error: envelope shape {name!r} is not available on the device (have {sorted(ENV_SHAPES)})")
            shapes[k, e] = ENV_SHAPES[name]
            for key, val in comp.items():
                if key in ("shape", "use_t_before", "drag"):
                    continue
                if key not in ENV_SLOTS:
                    raise C3PropError(f"C3:Error: unknown envelope parameter {key!r}")
                env[:, k, e, ENV_SLOTS[key]] = np.asarray(val, dtype=np.float64)
            fl = (ENVF_T_BEFORE if comp.get("use_t_before", False) else 0) | (ENVF_DRAG if comp.get("drag", False) else 0)
            env[:, k, e, ENV_SLOTS["flags"]] = float(fl)
            if name != "no_drive" and "t_final" not in comp:
                raise C3PropError("C3:Error: envelope component needs t_final")
    return env, shapes


def table_block_len(shape: str, M: int) -> int:
    """Doubles in the block of a table component with M coefficients per array."""
    scalars, arrays = TAB_LAYOUT[shape]
    return len(scalars) + len(arrays) * M


def pack_table_components(channels: Sequence[Sequence[Dict]], B: int = 1, awg_samples: Optional[int] = None):
    """`pack_components` for lines that also carry sampled or Fourier envelopes ->
    (env_params [B,K,E,NPAR], env_shapes [K,E], env_tables [B,T], table_index [K,E,2]).

    A component whose `shape` is one of TAB_SHAPES carries the reference's array parameters (envelopes.py:31-68,104-125,
    142-191): `inphase` / `quadrature` (pwc: one pair per AWG sample), `t_bin_start`, `t_bin_end`, `inphase` (pwc_shape,
    pwc_symmetric: M >= 2 knots), `amps`, `freqs`, `phases` (fourier_sin), `amps`, `freqs` (fourier_cos).  An array is [M]
    (shared by the batch) or [B,M]; the scalars are shared or [B].  Its block lies at `table_index[k,e] = (offset, M)` in every
    sample's row of `env_tables`, laid out as TAB_LAYOUT says; components without a table have (-1, 0).  The blocks follow
    each other in the order of the components.  `awg_samples` (Na) lets the pwc length be checked here.
    """
    K = len(channels)
    E = max(1, max(len(c) for c in channels))
    for comps in channels:
        for comp in comps:
            stray = sorted(set(comp) & _TAB_KEYS) if comp["shape"] in ENV_SHAPES else []
            if stray:
                raise C3PropError(f"C3:Error: envelope shape {comp['shape']!r} takes no array parameter {stray[0]!r}")
    plain = [[{k: v for k, v in comp.items() if k not in _TAB_KEYS} if comp["shape"] in TAB_SHAPES else comp for comp in comps] for comps in channels]
    for comps in plain:
        for comp in comps:
            if comp["shape"] in TAB_SHAPES:
                comp["shape"] = "rect"  # placeholder: the row's slots are packed as for any shape, the id is set below
    env, shapes = pack_components(plain, B=B)
    index = np.zeros((K, E, 2), dtype=np.int32)
    index[..., 0] = -1
    blocks, T = [], 0
    for k, comps in enumerate(channels):
        for e, comp in enumerate(comps):
            name = comp["shape"]
            if name not in TAB_SHAPES:
                continue
            if comp.get("drag", False):
                raise C3PropError(f"C3:Error: DRAG on the table shape {name!r} is not available on the device")
            if name == "pwc" and comp.get("use_t_before", False):
                raise C3PropError("C3:Error: use_t_before on 'pwc' is refused (the reference's offset would be the array itself)")
            scalars, arrays = TAB_LAYOUT[name]
            for key in scalars + arrays:
                if key not in comp:
                    raise C3PropError(f"C3:Error: envelope shape {name!r} needs '{key}'")
            cols = []
            for key in scalars:
                v = np.asarray(comp[key], dtype=np.float64)
                if v.shape not in ((), (B,)):
                    raise C3PropError(f"C3:Error: '{key}' must be a scalar or [{B}], got {v.shape}")
                cols.append(np.broadcast_to(v.reshape(-1, 1), (B, 1)))
            M = None
            for key in arrays:
                v = np.asarray(comp[key], dtype=np.float64)
                if v.ndim not in (1, 2) or (v.ndim == 2 and v.shape[0] != B):
                    raise C3PropError(f"C3:Error: '{key}' must be [M] or [{B},M], got {v.shape}")
                if M is None:
                    M = int(v.shape[-1])
                    if M < 1:
                        raise C3PropError(f"C3:Error: '{key}' of {name!r} is empty")
                elif v.shape[-1] != M:
                    raise C3PropError(f"C3:Error: '{key}' of {name!r} holds {v.shape[-1]} values, '{arrays[0]}' holds {M}")
                cols.append(np.broadcast_to(v.reshape(-1, M), (B, M)))
            if name in ("pwc_shape", "pwc_symmetric"):
                if M < 2:
                    raise C3PropError(f"C3:Error: {name!r} needs at least two knots, got {M}")
                if not np.all(cols[1] > cols[0]):
                    raise C3PropError(f"C3:Error: {name!r} needs t_bin_end > t_bin_start")
            if name == "pwc" and awg_samples is not None and M != awg_samples:
                raise C3PropError(f"C3:Error: 'pwc' holds one pair per AWG sample: {M} values for {awg_samples} samples")
            shapes[k, e] = TAB_SHAPES[name]
            index[k, e] = (T, M)
            blocks += cols
            T += table_block_len(name, M)
    tables = np.ascontiguousarray(np.concatenate(blocks, axis=1)) if blocks else np.zeros((B, 0), dtype=np.float64)
    return env, shapes, tables, index


def response_tap_count(rise_time: float, sim_res: float) -> int:
    """Response (devices.py:614): floor(rise_time * resolution) taps, of that one double product."""
    return int(np.floor(float(rise_time) * float(sim_res)))


def _check_lines(kinds: np.ndarray, params: Optional[np.ndarray], sim_res: Optional[float]) -> None:
    if kinds.size and (kinds.min() < 0 or kinds.max() >= len(LINE_KINDS)):
        raise C3PropError(f"C3:Error: line_kinds holds an unknown kind id (have {LINE_KINDS})")
    if sim_res is not None:
        rt = params[..., LINE_SLOTS["rise_time"]]
        bad = (rt > 0) & (np.floor(rt * float(sim_res)) < 1)
        if bad.any():
            b, k = (int(x) for x in np.argwhere(bad)[0])
            raise C3PropError(f"C3:Error: rise_time={rt[b, k]:g} of line [{b},{k}] gives no Response tap at sim_res={sim_res:g}")


def pack_lines(lines: Sequence[Dict], B: int = 1, sim_res: Optional[float] = None):
    """What follows the AWG on each line -> (line_kinds int32 [K], line_params [B,K,LINE_NPAR]).

    `lines[k]` is a dict: `kind` "drive" (Mixer -> VoltsToHertz, the default) or "flux" (Mixer -> FluxTuning,
    devices.py:457-525, with `phi_0`, `phi`, `omega_0`, `anhar` and optionally `d`), and optionally `rise_time` > 0 for a
    Response stage between DAC and Mixer (devices.py:585-642).  Values are scalars or arrays of B per-sample values.  With
    `sim_res` a rise_time too short for one tap is refused here (the library refuses it on host-pointer calls).
    """
    K = len(lines)
    kinds = np.zeros(K, dtype=np.int32)
    params = np.zeros((B, K, LINE_NPAR), dtype=np.float64)
    for k, line in enumerate(lines):
        name = line.get("kind", "drive")
        if name not in LINE_KINDS:
            raise C3PropError(f"C3:Error: line kind {name!r} is not available on the device (have {sorted(LINE_KINDS)})")
        kinds[k] = LINE_KINDS[name]
        for key, val in line.items():
            if key == "kind":
                continue
            if key not in LINE_SLOTS:
                raise C3PropError(f"C3:Error: unknown line parameter {key!r}")
            params[:, k, LINE_SLOTS[key]] = np.asarray(val, dtype=np.float64)
        if name == "flux":
            for key in ("phi_0", "phi", "omega_0", "anhar"):  # FluxTuning.__init__ (devices.py:475-479)
                if key not in line:
                    raise C3PropError(f"C3:Error: a flux line needs a '{key}' parameter")
    _check_lines(kinds, params, sim_res)
    return kinds, params


def _check_filters(kinds: np.ndarray, params: Optional[np.ndarray], sim_res: Optional[float]) -> None:
    """what the library refuses on host-pointer calls; `params` None: the kinds alone (device rows are not looked at)"""
    if kinds.size and kinds.max() >= len(FILT_KINDS):
        raise C3PropError(f"C3:Error: filter kinds hold an unknown kind id (have {FILT_KINDS})")
    if params is None:
        return
    used = np.broadcast_to(kinds >= 0, params.shape[:-1])
    tau, amp = params[..., FILT_SLOTS["tau"]], params[..., FILT_SLOTS["amp"]]
    if (used & ~(np.isfinite(tau) & np.isfinite(amp))).any():
        raise C3PropError("C3:Error: a filter parameter is not finite")
    if (used & (kinds != FILT_KINDS["skin_effect"]) & ~(tau > 0)).any():
        raise C3PropError("C3:Error: a filter's time constant must be positive")
    if sim_res is not None and (used & (kinds == FILT_KINDS["response_fft"]) & (np.floor(tau * float(sim_res)) < 1)).any():
        raise C3PropError(f"C3:Error: a response_fft rise_time gives no tap at sim_res={sim_res:g}")


def pack_line_filters(lines: Sequence[Sequence[Dict]], B: int = 1, sim_res: Optional[float] = None):
    """Distortion stages per line -> (filt_kind int32 [K,F], filt_params [B,K,F,FILT_NPAR]).

    `lines[k]` lists the stages of line k in the order they act, between DAC (and the legacy Response of `pack_lines`) and
    Mixer, as dicts keyed like the reference's devices: `{"kind": "exp_iir", "time_iir": .., "amp": ..}` (ExponentialIIR,
    devices.py:735-751), `{"kind": "highpass_exp", "time_hp": ..}` (:755-769), `{"kind": "skin_effect", "alpha": ..}`
    (:773-787), `{"kind": "response_fft", "rise_time": ..}` (:646-701).  Values are scalars or arrays of B per-sample values.
    Lines with fewer stages than the longest keep unused slots (kind -1) at the end.
    """
    K = len(lines)
    F = max([len(st) for st in lines] + [0])
    kinds = np.full((K, F), -1, dtype=np.int32)
    params = np.zeros((B, K, F, FILT_NPAR), dtype=np.float64)
    for k, stages in enumerate(lines):
        for f, stage in enumerate(stages):
            name = stage.get("kind")
            if name not in FILT_KINDS:
                raise C3PropError(f"C3:Error: filter kind {name!r} is not available on the device (have {sorted(FILT_KINDS)})")
            keys = _FILT_KEYS[name]
            for key, val in stage.items():
                if key == "kind":
                    continue
                if key not in keys:
                    raise C3PropError(f"C3:Error: filter kind {name!r} takes no parameter {key!r} (takes {sorted(keys)})")
                v = np.asarray(val, dtype=np.float64)
                if v.shape not in ((), (B,)):
                    raise C3PropError(f"C3:Error: '{key}' must be a scalar or [{B}], got {v.shape}")
                params[:, k, f, FILT_SLOTS[keys[key]]] = v
            for key in keys:
                if key not in stage:
                    raise C3PropError(f"C3:Error: filter kind {name!r} needs '{key}'")
            kinds[k, f] = FILT_KINDS[name]
    _check_filters(kinds, params, sim_res)
    return kinds, params


def pack_crosstalk(channels: Sequence[str], crossed_channels: Sequence[str], matrix) -> np.ndarray:
    """Crosstalk.process (devices.py:262-292) as one [K,K] matrix over all lines: `matrix` [C,C] mixes the lines named in
    `crossed_channels` (in that order) among themselves, every other line keeps its identity row."""
    channels, crossed = list(channels), list(crossed_channels)
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (len(crossed), len(crossed)):
        raise C3PropError(f"C3:Error: the crosstalk matrix must be [{len(crossed)},{len(crossed)}], got {m.shape}")
    if len(set(crossed)) != len(crossed):
        raise C3PropError("C3:Error: a crossed channel is named twice")
    for ch in crossed:
        if ch not in channels:
            raise C3PropError(f"C3:Error: crossed channel {ch!r} is not a line (have {channels})")
    idx = [channels.index(ch) for ch in crossed]
    out = np.eye(len(channels), dtype=np.float64)
    out[np.ix_(idx, idx)] = m
    return out


_shapes_memo = TensorMemo()  # device shape tables: per tensor object (weak reference + version), never per address
_shapes_upload: Dict[tuple, object] = {}  # content-keyed uploads of host tables


def _shapes(call, env_shapes, K: int, E: int, tables: bool = False):
    """(host int32 [K,E], the array the library call takes): validated once per distinct table; on the device path the upload
    is cached -- an optimiser calls the synthesis and its vjp every iteration with the same shapes, and a pageable
    host-to-device copy per call is a synchronisation (and illegal inside a stream capture).  A device table is remembered
    per tensor OBJECT; the [K,E] check against the parameter rows runs on every call, hit or not."""
    on_dev = _is_torch(env_shapes) and env_shapes.is_cuda
    mkey = (str(env_shapes.dtype), str(call.dev), tables) if on_dev else None  # the upload lives on call.dev
    hit = _shapes_memo.get(env_shapes, mkey) if on_dev else None
    if hit is not None:
        if hit[0].shape != (K, E):
            raise C3PropError(f"C3:Error: env_shapes must be [{K},{E}], got {hit[0].shape}")
        return hit
    shapes_np = np.ascontiguousarray(np.asarray(env_shapes.cpu() if _is_torch(env_shapes) else env_shapes, dtype=np.int32))
    if shapes_np.shape != (K, E):
        raise C3PropError(f"C3:Error: env_shapes must be [{K},{E}], got {shapes_np.shape}")
    unknown = shapes_np >= len(ENV_SHAPES)
    if tables:  # only a call that brings a coefficient table takes the TAB_SHAPES ids
        unknown &= ~np.isin(shapes_np, list(TAB_SHAPES.values()))
    if unknown.any():
        raise C3PropError("C3:Error: env_shapes holds an unknown shape id" + ("" if tables else " (the TAB_SHAPES need env_tables and table_index)"))
    if not call.device:
        return shapes_np, shapes_np
    key2 = (shapes_np.tobytes(), shapes_np.shape, str(call.dev))
    shp = _shapes_upload.get(key2)
    if shp is None:
        if len(_shapes_upload) > 64:
            _shapes_upload.clear()
        shp = _shapes_upload[key2] = call.torch.as_tensor(shapes_np, device=call.dev)
    if on_dev:
        _shapes_memo.put(env_shapes, mkey, (shapes_np, shp))
    return shapes_np, shp


def _table_index(call, table_index, shapes_np: np.ndarray, T: int, Na: int):
    """The index table as the library call takes it, treated as `_shapes` treats the shape table: checked on the host once per
    distinct (index, shapes, T, Na) -- blocks inside the row and apart from each other, M = Na for pwc, M >= 2 for the
    interpolated shapes -- and, on the device route, uploaded once."""
    K, E = shapes_np.shape
    on_dev = _is_torch(table_index) and table_index.is_cuda
    mkey = ("tidx", str(call.dev), shapes_np.tobytes(), T, Na) if on_dev else None
    hit = _shapes_memo.get(table_index, mkey) if on_dev else None
    if hit is not None:
        return hit
    idx = np.ascontiguousarray(np.asarray(table_index.cpu() if _is_torch(table_index) else table_index, dtype=np.int32))
    if idx.shape != (K, E, 2):
        raise C3PropError(f"C3:Error: table_index must be [{K},{E},2], got {idx.shape}")
    key = ("tidx", idx.tobytes(), shapes_np.tobytes(), T, Na, str(call.dev) if call.device else None)
    up = _shapes_upload.get(key)
    if up is None:
        spans = []
        for k in range(K):
            for e in range(E):
                name = _TAB_NAMES.get(int(shapes_np[k, e]))
                if name is None:
                    continue
                off, M = (int(x) for x in idx[k, e])
                if off < 0 or M < 1 or off + table_block_len(name, M) > T:
                    raise C3PropError(f"C3:Error: table_index[{k},{e}]=({off},{M}): the block of {name!r} does not lie inside the row (T={T})")
                if name == "pwc" and M != Na:
                    raise C3PropError(f"C3:Error: component [{k},{e}]: 'pwc' holds one pair per AWG sample, M={M} but Na={Na}")
                if name in ("pwc_shape", "pwc_symmetric") and M < 2:
                    raise C3PropError(f"C3:Error: component [{k},{e}]: {name!r} needs at least two knots, got {M}")
                spans.append((off, off + table_block_len(name, M)))
        spans.sort()
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            if b0 < a1:
                raise C3PropError(f"C3:Error: table_index: the blocks [{a0},{a1}) and [{b0},{b1}) overlap")
        if len(_shapes_upload) > 64:
            _shapes_upload.clear()
        up = _shapes_upload[key] = call.torch.as_tensor(idx, device=call.dev) if call.device else idx
    if on_dev:
        _shapes_memo.put(table_index, mkey, up)
    return up


def _tables(call, env_tables, table_index, shapes_np, B: int, Na: int):
    """(env_tab, tab_index, T) of a call with a coefficient table"""
    tab = call.f64(env_tables)
    if tab.ndim != 2 or int(tab.shape[0]) != B:
        raise C3PropError(f"C3:Error: env_tables must be [{B},T], got {tuple(tab.shape)}")
    T = int(tab.shape[1])
    return tab, _table_index(call, table_index, shapes_np, T, Na), T


def _lines(call, line_kinds, line_params, B: int, K: int, sim_res: float):
    """(kinds, params) as the library call takes them.  Host rows are checked here; the kind table is uploaded once per
    distinct content (as the shape table is), device rows are taken as they are -- looking at them would synchronise."""
    kinds_np = np.ascontiguousarray(np.asarray(line_kinds.cpu() if _is_torch(line_kinds) else line_kinds, dtype=np.int32))
    if kinds_np.shape != (K,):
        raise C3PropError(f"C3:Error: line_kinds must be [{K}], got {kinds_np.shape}")
    par = call.f64(line_params)
    if tuple(par.shape) != (B, K, LINE_NPAR):
        raise C3PropError(f"C3:Error: line_params must be [{B},{K},{LINE_NPAR}], got {tuple(par.shape)}")
    if _is_torch(line_params) and line_params.is_cuda:
        _check_lines(kinds_np, None, None)
    else:
        _check_lines(kinds_np, np.asarray(line_params.numpy() if _is_torch(line_params) else line_params, dtype=np.float64), sim_res)
    if not call.device:
        return kinds_np, par
    key = ("kinds", kinds_np.tobytes(), str(call.dev))
    knd = _shapes_upload.get(key)
    if knd is None:
        if len(_shapes_upload) > 64:
            _shapes_upload.clear()
        knd = _shapes_upload[key] = call.torch.as_tensor(kinds_np, device=call.dev)
    return knd, par


def _filters(call, line_filters, B: int, K: int, sim_res: float):
    """(kinds, params, F) as the library call takes them, treated as `_lines` treats the line rows"""
    if not isinstance(line_filters, (tuple, list)) or len(line_filters) != 2:
        raise C3PropError("C3:Error: line_filters is the pair (filt_kind [K,F], filt_params [B,K,F,2]) of pack_line_filters")
    fk, fp = line_filters
    kinds_np = np.ascontiguousarray(np.asarray(fk.cpu() if _is_torch(fk) else fk, dtype=np.int32))
    if kinds_np.ndim != 2 or kinds_np.shape[0] != K:
        raise C3PropError(f"C3:Error: filter kinds must be [{K},F], got {kinds_np.shape}")
    F = int(kinds_np.shape[1])
    par = call.f64(fp)
    if tuple(par.shape) != (B, K, F, FILT_NPAR):
        raise C3PropError(f"C3:Error: filter parameters must be [{B},{K},{F},{FILT_NPAR}], got {tuple(par.shape)}")
    if _is_torch(fp) and fp.is_cuda:
        _check_filters(kinds_np, None, None)
    else:
        _check_filters(kinds_np, np.asarray(fp.numpy() if _is_torch(fp) else fp, dtype=np.float64), sim_res)
    if F == 0:
        return None, None, 0
    if not call.device:
        return kinds_np, par, F
    key = ("fkinds", kinds_np.tobytes(), kinds_np.shape, str(call.dev))
    knd = _shapes_upload.get(key)
    if knd is None:
        if len(_shapes_upload) > 64:
            _shapes_upload.clear()
        knd = _shapes_upload[key] = call.torch.as_tensor(kinds_np, device=call.dev)
    return knd, par, F


def _no_table_index(call, K: int, E: int):
    """the index table of a c3p_synth_filt call without a coefficient table: every component (-1, 0)"""
    idx = np.zeros((K, E, 2), dtype=np.int32)
    idx[..., 0] = -1
    if not call.device:
        return idx
    key = ("notab", K, E, str(call.dev))
    up = _shapes_upload.get(key)
    if up is None:
        if len(_shapes_upload) > 64:
            _shapes_upload.clear()
        up = _shapes_upload[key] = call.torch.as_tensor(idx, device=call.dev)
    return up


def _begin(env_params, env_shapes, carrier, t_start, t_end, awg_res, sim_res, grad_signals, line_kinds, line_params, env_tables, table_index,
           line_filters=None, dc_offset=None, crosstalk=None):
    """What `synthesize_signals` and `synthesize_signals_vjp` (the call with `grad_signals`) share: the argument checks, and the
    one place that picks the C entry -- `c3p_synth_tab` with a coefficient table, `c3p_synth_chain` with lines alone, else
    `c3p_synth_signals`, `_vjp` appended for the vjp -- and builds the arguments all six start with.

    With any of `line_filters`, `dc_offset`, `crosstalk` the entry is `c3p_synth_filt`, whatever else travels.

    -> (call, entry, leading arguments, the arrays behind them (the caller holds them over the call), B, K, E, N, Na, T); T is
    None without a table.  A vjp's leading arguments end with grad_signals [B,K,N]."""
    if (line_kinds is None) != (line_params is None):
        raise C3PropError("C3:Error: line_kinds and line_params go together")
    if (env_tables is None) != (table_index is None):
        raise C3PropError("C3:Error: env_tables and table_index go together")
    filt = line_filters is not None or dc_offset is not None or crosstalk is not None
    call = _Call(env_params, carrier, grad_signals, line_params, env_tables, line_filters[1] if line_filters is not None and len(line_filters) == 2 else None, dc_offset, crosstalk)
    env = call.f64(env_params)
    if env.ndim != 4 or env.shape[-1] != ENV_NPAR:
        raise C3PropError(f"C3:Error: env_params must be [B,K,E,{ENV_NPAR}], got {tuple(env.shape)}")
    B, K, E, _ = env.shape
    shapes_np, shp = _shapes(call, env_shapes, K, E, tables=env_tables is not None)
    car = call.f64(carrier)
    if tuple(car.shape) != (B, K, 2):
        raise C3PropError(f"C3:Error: carrier must be [{B},{K},2], got {tuple(car.shape)}")
    N, Na = slice_num(t_start, t_end, sim_res), slice_num(t_start, t_end, awg_res)
    if N <= 0 or Na <= 1:
        raise C3PropError(f"C3:Error: empty time grid (N={N}, AWG samples={Na})")
    gs = call.f64(grad_signals)
    if gs is not None and tuple(gs.shape) != (B, K, N):
        raise C3PropError(f"C3:Error: grad_signals must be [{B},{K},{N}], got {tuple(gs.shape)}")
    tab = tidx = T = knd = par = None
    if env_tables is not None:
        tab, tidx, T = _tables(call, env_tables, table_index, shapes_np, B, Na)
    if line_kinds is not None:
        knd, par = _lines(call, line_kinds, line_params, B, K, sim_res)
    if filt:
        fk = fp = None
        F = 0
        if line_filters is not None:
            fk, fp, F = _filters(call, line_filters, B, K, sim_res)
        dc, xt = call.f64(dc_offset), call.f64(crosstalk)
        if dc is not None and tuple(dc.shape) != (B, K):
            raise C3PropError(f"C3:Error: dc_offset must be [{B},{K}], got {tuple(dc.shape)}")
        if xt is not None and tuple(xt.shape) == (K, K):  # one matrix for the batch
            xt = (xt.expand(B, K, K) if call.device else np.broadcast_to(xt, (B, K, K)))
            xt = xt.contiguous() if call.device else np.ascontiguousarray(xt)
        if xt is not None and tuple(xt.shape) != (B, K, K):
            raise C3PropError(f"C3:Error: crosstalk must be [{K},{K}] or [{B},{K},{K}], got {tuple(xt.shape)}")
        if T is None:
            tidx = _no_table_index(call, K, E)
        name = "c3p_synth_filt"
        head = (_ptr(env), _ptr(shp), _ptr(tab), _ptr(tidx), T or 0, _ptr(car), _ptr(knd), _ptr(par), _ptr(fk), _ptr(fp), F, _ptr(dc), _ptr(xt))
        held = (env, shp, tab, tidx, car, knd, par, gs, fk, fp, dc, xt)
        head += (float(t_start), float(t_end), float(awg_res), float(sim_res), B, K, E, call.flags)
        if gs is not None:
            name, head = name + "_vjp", head + (_ptr(gs),)
        return call, getattr(_lib.load(), name), head, held, B, K, E, N, Na, T
    if T is not None:
        name, head = "c3p_synth_tab", (_ptr(env), _ptr(shp), _ptr(tab), _ptr(tidx), T, _ptr(car), _ptr(knd), _ptr(par))
    elif knd is not None:
        name, head = "c3p_synth_chain", (_ptr(env), _ptr(shp), _ptr(car), _ptr(knd), _ptr(par))
    else:
        name, head = "c3p_synth_signals", (_ptr(env), _ptr(shp), _ptr(car))
    head += (float(t_start), float(t_end), float(awg_res), float(sim_res), B, K, E, call.flags)
    if gs is not None:
        name, head = name + "_vjp", head + (_ptr(gs),)
    return call, getattr(_lib.load(), name), head, (env, shp, tab, tidx, car, knd, par, gs), B, K, E, N, Na, T


def _empty(call, shape):
    """an uninitialised f64 output where the call's inputs live"""
    return call.torch.empty(shape, dtype=call.torch.float64, device=call.dev) if call.device else np.empty(shape, dtype=np.float64)


def synthesize_signals(env_params, env_shapes, carrier, t_start: float, t_end: float, awg_res: float, sim_res: float, *, want_iq: bool = False, device=None, line_kinds=None, line_params=None, env_tables=None, table_index=None,
                       line_filters=None, dc_offset=None, crosstalk=None):
    """signals [B,K,N] (and optionally the AWG-resolution I/Q [B,K,2,Na]) from parameter rows.

    With `line_kinds` [K] int32 and `line_params` [B,K,LINE_NPAR] (see `pack_lines`) every line runs the chain
    AWG -> DAC -> Response -> Mixer -> VoltsToHertz | FluxTuning (`c3p_synth_chain`); without them the standard drive line.

    With `env_tables` [B,T] f64 and `table_index` [K,E,2] int32 (see `pack_table_components`) `env_shapes` may hold TAB_SHAPES
    ids: sampled (pwc, pwc_shape, pwc_symmetric) and Fourier envelopes that read their coefficients from the table
    (`c3p_synth_tab`, on either kind of line).  Without the two keywords every call goes where it went before them.

    With `line_filters` = (filt_kind [K,F] int32, filt_params [B,K,F,FILT_NPAR]) (see `pack_line_filters`), `dc_offset` [B,K]
    or `crosstalk` [K,K] | [B,K,K] (see `pack_crosstalk`) the call goes to `c3p_synth_filt`: the stages act on the I/Q pair
    between DAC (after the legacy Response) and Mixer, each the causal convolution of tf_convolve with the stage's impulse
    response on the signal's own time grid; the offset is added to the mixer output (DC_Offset, devices.py:1039-1059), and
    the matrix mixes the finished lines (Crosstalk, devices.py:225-292).  Without the three the call goes where it went before.

    env_params [B,K,E,NPAR] f64, env_shapes [K,E] int32, carrier [B,K,2] f64 = (LO angular
    frequency, V_to_Hz).  numpy in -> numpy out (staged by the library); with `device` (or any torch
    CUDA input) the outputs are torch CUDA tensors that `propagate_batch` takes zero-copy.
    """
    if device is not None:
        import torch

        env_params = torch.as_tensor(np.asarray(env_params, dtype=np.float64) if not _is_torch(env_params) else env_params, device=device)
        if env_tables is not None and table_index is not None and not _is_torch(env_tables):
            env_tables = torch.as_tensor(np.asarray(env_tables, dtype=np.float64), device=device)
    call, entry, head, held, B, K, _, N, Na, _ = _begin(env_params, env_shapes, carrier, t_start, t_end, awg_res, sim_res, None, line_kinds, line_params, env_tables, table_index,
                                                        line_filters, dc_offset, crosstalk)
    sig = _empty(call, (B, K, N))
    iq = _empty(call, (B, K, 2, Na)) if want_iq else None
    _lib.check(entry(*head, _ptr(iq), _ptr(sig), call.stream))
    return (sig, iq) if want_iq else sig


def synthesize_signals_vjp(env_params, env_shapes, carrier, t_start: float, t_end: float, awg_res: float, sim_res: float, grad_signals, *, line_kinds=None, line_params=None, env_tables=None, table_index=None,
                           line_filters=None, dc_offset=None, crosstalk=None):
    """(grad_env [B,K,E,NPAR], grad_carrier [B,K,2]) from d loss / d signals [B,K,N]; with `line_kinds` / `line_params`
    (the chain of `synthesize_signals`) also grad_line [B,K,LINE_NPAR]: phi_0, phi, omega_0, anhar, d in their LINE_SLOTS,
    0 for rise_time (the tap count is a floor) and, in grad_carrier, for V_to_Hz on a flux line.  With `env_tables` /
    `table_index` (the coefficient table of `synthesize_signals`) grad_tables [B,T] is an additional last value: the
    cotangent of every coefficient in the layout of env_tables, exactly 0 in the t_bin_start / t_bin_end slots (they are
    not differentiated) and outside the blocks.

    With `line_filters`, `dc_offset`, `crosstalk` (as `synthesize_signals` takes them) the values above are followed by
    grad_filt [B,K,F,FILT_NPAR] (time_iir and amp of exp_iir, time_hp, alpha; exactly 0 for a response_fft rise_time and in
    unused slots), grad_dc [B,K] and grad_xtalk [B,K,K], for those of the three that were passed, in that order.

    Differentiates amp, xy_angle, freq_offset, delta (their ENV_SLOTS) and the carrier pair; the
    reference gets the same numbers from the tape that also covers the propagation
    (optimizers/optimizer.py:206-216, gates.py:341-370).  Chain with `propagate_batch_vjp`.
    """
    call, entry, head, held, B, K, E, _, _, T = _begin(env_params, env_shapes, carrier, t_start, t_end, awg_res, sim_res, grad_signals, line_kinds, line_params, env_tables, table_index,
                                                       line_filters, dc_offset, crosstalk)
    outs = (_empty(call, (B, K, E, ENV_NPAR)), _empty(call, (B, K, 2)))
    if line_kinds is not None:
        outs += (_empty(call, (B, K, LINE_NPAR)),)
    if line_filters is not None or dc_offset is not None or crosstalk is not None:
        F = int(held[9].shape[2]) if held[9] is not None else 0
        gl = outs[2] if line_kinds is not None else None
        gt = _empty(call, (B, T)) if T is not None else None
        gf = (_empty(call, (B, K, F, FILT_NPAR)) if line_filters is not None else None)
        gd = _empty(call, (B, K)) if dc_offset is not None else None
        gx = _empty(call, (B, K, K)) if crosstalk is not None else None
        _lib.check(entry(*head, _ptr(outs[0]), _ptr(outs[1]), _ptr(gl), _ptr(gt) if T else None, _ptr(gf) if F else None, _ptr(gd), _ptr(gx), call.stream))
        return outs + tuple(g for g in (gt, gf, gd, gx) if g is not None)
    if T is None:
        _lib.check(entry(*head, *map(_ptr, outs), call.stream))
    else:  # the table entry takes grad_line whether lines travel or not
        outs += (_empty(call, (B, T)),)
        _lib.check(entry(*head, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]) if line_kinds is not None else None, _ptr(outs[-1]), call.stream))
    return outs


def create_ts(t_start: float, t_end: float, resolution: float) -> np.ndarray:
    """Centred sample times (devices.py:86-122)."""
    num = slice_num(t_start, t_end, resolution)
    dt = 1.0 / resolution
    return np.linspace(t_start + dt / 2, t_end - dt / 2, num)


def generate_signals(channels: Dict[str, Dict], t_start: float, t_end: float, awg_res: float, sim_res: float) -> Dict[str, Dict[str, np.ndarray]]:
    """`Generator.generate_signals(instr)`-shaped result (generator.py:172-229) for one instruction.

    `channels[name] = {"components": [envelope dicts], "lo_freq": w [rad/s], "v_to_hz": f}`;
    returns `{name: {"values": [N], "ts": [N]}}` -- what `pwc` reads (propagation.py:289-294).
    A channel may carry `"response": {"rise_time": s}` (a Response device between DAC and Mixer) and
    `"flux_tuning": {"phi_0", "phi", "omega_0", "anhar", "d"}` (FluxTuning in place of VoltsToHertz): the chains of the
    reference's tunable-coupler generator (test/test_tunable_coupler.py:190-218).
    """
    names = list(channels)
    env, shapes = pack_components([channels[n]["components"] for n in names], B=1)
    carrier = np.array([[[channels[n]["lo_freq"], channels[n].get("v_to_hz", 1.0)] for n in names]], dtype=np.float64)
    if any("response" in channels[n] or "flux_tuning" in channels[n] for n in names):
        lines = []
        for n in names:
            ch = channels[n]
            line = dict(ch["flux_tuning"], kind="flux") if "flux_tuning" in ch else {"kind": "drive"}
            if "response" in ch:
                line["rise_time"] = ch["response"]["rise_time"]
            lines.append(line)
        kinds, params = pack_lines(lines, B=1, sim_res=sim_res)
        sig = synthesize_signals(env, shapes, carrier, t_start, t_end, awg_res, sim_res, line_kinds=kinds, line_params=params)
    else:
        sig = synthesize_signals(env, shapes, carrier, t_start, t_end, awg_res, sim_res)
    ts = create_ts(t_start, t_end, sim_res)
    return {n: {"values": np.asarray(sig[0, k]), "ts": ts} for k, n in enumerate(names)}
