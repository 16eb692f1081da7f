"""`c3p_synth_tab` / `c3p_synth_tab_vjp` on the GPU: sampled (pwc, pwc_shape, pwc_symmetric) and Fourier envelopes from a
coefficient table, against the numpy restatement (tests/sampled_envelope_ref.py) on both pointer routes, the cotangents of
every coefficient, agreement with the existing entries, and the route through the optimiser bodies.  -m gpu."""
import numpy as np
import pytest

import sampled_envelope_ref as ref
import signal_chain_ref as chain
from c3_amd import signals as sg
from oracle import c3_oracle as o

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi
SIM_RES = 100e9
GRID10 = (0.0, 10e-9, 2.4e9, SIM_RES)  # Na = 24, N = 1000
GRID40 = (0.0, 40e-9, 2.4e9, SIM_RES)  # Na = 96, N = 4000
FWD_TOL = 1e-12  # forward values: of max|want| per line (tests/test_gpu_signal_chain.py:154)
VJP_TOL = 1e-10  # cotangents: of the largest magnitude in the wanted block (tests/test_gpu_signal_chain.py:195)
SCALARS = ("amp", "xy_angle", "freq_offset")


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


def _scal(rng, T, **kw):
    return dict(amp=rng.uniform(0.3, 1.0), xy_angle=rng.uniform(-1, 3), freq_offset=rng.uniform(-60e6, 60e6) * TWO_PI, t_final=T, **kw)


def _gauss(rng, T):
    return dict(_scal(rng, T), shape="gaussian_nonorm", sigma=T * rng.uniform(0.15, 0.3))


def _pwc(rng, T, M):
    return dict(_scal(rng, T), shape="pwc", inphase=rng.uniform(-1, 1, M), quadrature=rng.uniform(-1, 1, M))


def _interp(rng, T, M, name="pwc_shape", t_bin=(1e-10, 9.9e-9), **kw):
    return dict(_scal(rng, T, **kw), shape=name, t_bin_start=t_bin[0], t_bin_end=t_bin[1], inphase=rng.uniform(-1, 1, M))


def _fsin(rng, T, freqs, **kw):
    M = len(freqs)
    return dict(_scal(rng, T, **kw), shape="fourier_sin", amps=rng.uniform(-1, 1, M), freqs=np.asarray(freqs, dtype=float), phases=rng.uniform(-1, 1, M))


def _fcos(rng, T, freqs, **kw):
    return dict(_scal(rng, T, **kw), shape="fourier_cos", amps=rng.uniform(-1, 1, len(freqs)), freqs=np.asarray(freqs, dtype=float))


def _flux(rng):
    return dict(chain.TC_LINE, kind="flux", rise_time=chain.TC_RISE_TIME, phi=chain.TC_LINE["phi"] * rng.uniform(0.9, 1.1))


# name -> (grid, B, per-sample lines: rng -> [[component, ...] per line], per-sample line dicts or None)
WIN = dict(delay=2.1e-9)  # with t_final = 5e-9: the window 2.1 .. 7.095 ns inside the 10 ns instruction
CASES = {
    # 1. drive route, per-sample coefficients; the Fourier frequencies of the reference's test (test/test_envelopes.py:87)
    "drive_pwc_shape_sin": (GRID10, 3, lambda r: [[_gauss(r, 10e-9), _pwc(r, 10e-9, 24)], [_interp(r, 10e-9, 8), _fsin(r, 10e-9, [1e6, 1e10])]], None),
    "drive_symmetric_cos": (GRID10, 3, lambda r: [[_interp(r, 10e-9, 8, "pwc_symmetric", (1e-10, 4.9e-9)), _fcos(r, 10e-9, [1e6, 1e10])], [_gauss(r, 10e-9), _pwc(r, 10e-9, 24)]], None),
    # 2. offset windows: t_bin_start inside the window and t_bin_end beyond it, one interval and two; the mirror about 2.5 ns;
    #    a t_bin_start before t_before under use_t_before (t_before = -2.31 ns, one AWG period before the instruction's first
    #    sample seen from the delayed component: it lies on the knot grid, so the offset term is non-zero)
    "window_M2_M3": (GRID10, 2, lambda r: [[_interp(r, 5e-9, 2, t_bin=(0.7e-9, 6.2e-9), **WIN), _interp(r, 5e-9, 3, t_bin=(0.7e-9, 6.2e-9), **WIN)],
                                           [_interp(r, 5e-9, 3, "pwc_symmetric", (0.3e-9, 2.9e-9), **WIN), _interp(r, 5e-9, 5, t_bin=(-2.6e-9, 4.1e-9), use_t_before=True, **WIN)]], None),
    "window_before_fourier": (GRID10, 2, lambda r: [[_fsin(r, 5e-9, [3e8, 2e9, 7e9], use_t_before=True, **WIN), _fcos(r, 5e-9, [4e8, 5e9], use_t_before=True, **WIN)],
                                                    [_interp(r, 5e-9, 4, "pwc_symmetric", (-2.5e-9, 2.2e-9), use_t_before=True, **WIN)]], None),
    # 3. more AWG samples, knots and Fourier terms than one wavefront has lanes
    "past_one_wavefront": (GRID40, 2, lambda r: [[_pwc(r, 40e-9, 96), _fsin(r, 40e-9, r.uniform(1e8, 3e9, 70))], [_interp(r, 40e-9, 70, t_bin=(1e-10, 39.5e-9))]], None),
    # 4. chain route: a pwc_shape flux pulse behind Response and FluxTuning, beside a drive line with a pwc component
    "chain_flux_pwc_shape": (GRID10, 2, lambda r: [[_interp(r, 10e-9, 8)], [_pwc(r, 10e-9, 24), _fcos(r, 10e-9, [2e8, 3e9])]], lambda r: [_flux(r), {"kind": "drive"}]),
}


def _stack(per_sample):
    """[b][k][e] component dicts -> the packer's channels: every numeric value stacked over the samples"""
    first = per_sample[0]
    out = []
    for k, comps in enumerate(first):
        line = []
        for e, comp in enumerate(comps):
            d = {}
            for key, v in comp.items():
                d[key] = v if isinstance(v, (str, bool)) else np.stack([np.asarray(s[k][e][key], dtype=float) for s in per_sample])
            line.append(d)
        out.append(line)
    return out


def _for_ref(comp):
    return comp if comp["shape"] in ref.TAB_NAMES else dict(comp, shape=sg.ENV_SHAPES[comp["shape"]])


def _check_masks(comps, grid):
    """window edges at least a hundredth of an AWG period from every AWG sample: the mask is exactly 0 or 1"""
    ts = o.create_ts(*grid[:3])
    dt = ts[1] - ts[0]
    for c in comps:
        off = ts - (grid[0] + c.get("delay", 0.0))
        assert np.abs(off).min() > 0.01 * dt and np.abs(off - 0.999 * c["t_final"]).min() > 0.01 * dt
        m = o.envelope_mask(off, c["t_final"], c["t_final"])
        assert np.all((m == 0.0) | (m == 1.0)) and m.sum() >= 2


@pytest.fixture(scope="module")
def cases():
    """Every case once: packed inputs, the restatement's I/Q and signals, and its vjp of one random cotangent."""
    out = {}
    for idx, (name, (grid, B, make, make_lines)) in enumerate(CASES.items()):
        rng = np.random.default_rng(500 + idx)
        per = [make(rng) for _ in range(B)]
        K = len(per[0])
        N, Na = sg.slice_num(*grid[:2], grid[3]), sg.slice_num(*grid[:3])
        env, shapes, tab, tidx = sg.pack_table_components(_stack(per), B=B, awg_samples=Na)
        lo = rng.uniform(0.6e9, 1.0e9, size=(B, K)) * TWO_PI
        v2hz = rng.uniform(0.9e9, 1.1e9, size=(B, K)) * TWO_PI
        lines = kinds = par = None
        if make_lines is not None:
            lines = [make_lines(rng) for _ in range(B)]
            packed = [sg.pack_lines(row, sim_res=SIM_RES) for row in lines]
            kinds, par = packed[0][0], np.concatenate([p[1] for p in packed], axis=0)
        gs = rng.normal(size=(B, K, N))
        want, wiq = np.empty((B, K, N)), np.empty((B, K, 2, Na))
        wcomp, wcar, wline = {}, {}, {}
        for b in range(B):
            for k in range(K):
                comps = [_for_ref(c) for c in per[b][k]]
                _check_masks(comps, grid)
                ln = lines[b][k] if lines else {"kind": "drive"}
                kw = dict(kind=sg.LINE_KINDS[ln["kind"]], v_to_hz=v2hz[b, k], rise_time=ln.get("rise_time", 0.0), line=ln)
                r = ref.generate(comps, lo[b, k], *grid, **kw)
                want[b, k], wiq[b, k, 0], wiq[b, k, 1] = r["values"], r["inphase"], r["quadrature"]
                wcomp[b, k], wcar[b, k], wline[b, k] = ref.generate_vjp(comps, lo[b, k], *grid, gs[b, k], **kw)
        out[name] = dict(grid=grid, B=B, K=K, N=N, Na=Na, per=per, env=env, shapes=shapes, tab=tab, tidx=tidx, carrier=np.stack([lo, v2hz], axis=-1), lines=lines,
                         kinds=kinds, par=par, gs=gs, want=want, wiq=wiq, wcomp=wcomp, wcar=wcar, wline=wline)
    return out


def _dev(x):
    import torch

    return torch.as_tensor(x, device="cuda:0")


def _chain_kw(c, device_resident):
    if c["kinds"] is None:
        return {}
    return dict(line_kinds=c["kinds"], line_params=_dev(c["par"]) if device_resident else c["par"])


def _forward(c, device_resident):
    if device_resident:
        sig, iq = sg.synthesize_signals(_dev(c["env"]), c["shapes"], _dev(c["carrier"]), *c["grid"], want_iq=True, env_tables=_dev(c["tab"]), table_index=c["tidx"], **_chain_kw(c, True))
        assert sig.is_cuda and iq.is_cuda
        return sig.cpu().numpy(), iq.cpu().numpy()
    return sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], want_iq=True, env_tables=c["tab"], table_index=c["tidx"], **_chain_kw(c, False))


def _vjp(c, device_resident, tab=None, tidx=None):
    tab, tidx = (c["tab"] if tab is None else tab), (c["tidx"] if tidx is None else tidx)
    if device_resident:
        r = sg.synthesize_signals_vjp(_dev(c["env"]), c["shapes"], _dev(c["carrier"]), *c["grid"], _dev(c["gs"]), env_tables=_dev(tab), table_index=_dev(tidx), **_chain_kw(c, True))
        return tuple(x.cpu().numpy() for x in r)
    return sg.synthesize_signals_vjp(c["env"], c["shapes"], c["carrier"], *c["grid"], c["gs"], env_tables=tab, table_index=tidx, **_chain_kw(c, False))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("device_resident", [False, True])
def test_forward_vs_restatement(prop, cases, name, device_resident):
    """AWG I/Q and signals of every line, every sample compared: 1e-12 max|want| of the line."""
    c = cases[name]
    sig, iq = _forward(c, device_resident)
    assert sig.shape == c["want"].shape and iq.shape == c["wiq"].shape
    worst = 0.0
    for b in range(c["B"]):
        for k in range(c["K"]):
            w, wi = c["want"][b, k], c["wiq"][b, k]
            e_sig, e_iq = np.abs(sig[b, k] - w).max() / np.abs(w).max(), np.abs(iq[b, k] - wi).max() / np.abs(wi).max()
            worst = max(worst, e_sig, e_iq)
            assert e_sig < FWD_TOL and e_iq < FWD_TOL, (b, k, e_sig, e_iq)
    print(f"{name} device_resident={device_resident}: worst {worst:.3e} max|want|")


def _block_values(c, b, k, e, arr):
    """{array name: values} of component (k, e)'s block in row b of a [B,T] array, and its two scalar slots if it has any"""
    name = c["per"][b][k][e]["shape"]
    off, M = (int(x) for x in c["tidx"][k, e])
    scalars, arrays = sg.TAB_LAYOUT[name]
    ns = len(scalars)
    return {key: arr[b, off + ns + i * M : off + ns + (i + 1) * M] for i, key in enumerate(arrays)}, arr[b, off : off + ns]


@pytest.mark.parametrize("name", list(CASES))
def test_vjp_vs_restatement(prop, cases, name):
    """grad_tables (every coefficient of every block), the amp / xy_angle / freq_offset slots, the carrier pair and, on the
    chain, the line slots against the restatement's vjp of one random cotangent: 1e-10 of the largest magnitude in the wanted
    block (scalars as tests/test_gpu_signal_chain.py:189-210).  Two calls return the same bits, and so do the two routes."""
    c = cases[name]
    got = _vjp(c, True)
    again, host = _vjp(c, True), _vjp(c, False)
    for x, y, z in zip(got, again, host):
        assert np.array_equal(x, y) and np.array_equal(x, z)  # 6. determinism
    genv, gcar = got[0], got[1]
    gline, gtab = (got[2], got[3]) if c["kinds"] is not None else (None, got[2])
    assert len(got) == (4 if c["kinds"] is not None else 3)
    assert genv.shape == c["env"].shape and gcar.shape == c["carrier"].shape and gtab.shape == c["tab"].shape
    worst = {"table": 0.0, "env": 0.0, "carrier": 0.0, "line": 0.0}
    covered = np.zeros(c["tab"].shape, dtype=bool)
    for b in range(c["B"]):
        for k in range(c["K"]):
            flux = c["lines"] is not None and c["lines"][b][k]["kind"] == "flux"
            for e, wg in enumerate(c["wcomp"][b, k]):
                top = max(abs(wg[key]) for key in SCALARS)
                for key in SCALARS:
                    scale = max(abs(wg[key]), top * (1e-9 if key == "freq_offset" else 1.0))
                    err = abs(genv[b, k, e, sg.ENV_SLOTS[key]] - wg[key])
                    worst["env"] = max(worst["env"], err / scale)
                    assert err < VJP_TOL * scale, (b, k, e, key, err / scale)
                if c["per"][b][k][e]["shape"] not in sg.TAB_SHAPES:
                    continue
                blocks, tbin = _block_values(c, b, k, e, gtab)
                assert np.all(tbin == 0.0)  # 7. t_bin_start / t_bin_end are not differentiated
                off, M = (int(x) for x in c["tidx"][k, e])
                covered[b, off : off + sg.table_block_len(c["per"][b][k][e]["shape"], M)] = True
                for key, vals in blocks.items():
                    w = wg[key]
                    assert vals.shape == w.shape and np.abs(w).max() > 0
                    err = np.abs(vals - w).max() / np.abs(w).max()
                    worst["table"] = max(worst["table"], err)
                    assert err < VJP_TOL, (b, k, e, key, err)
            wc = c["wcar"][b, k]
            for i, key in enumerate(("lo_freq", "v_to_hz")):
                err = abs(gcar[b, k, i] - wc[key])
                worst["carrier"] = max(worst["carrier"], err / max(abs(wc[key]), 1e-300))
                assert err < VJP_TOL * abs(wc[key]) + 1e-20, (b, k, key)
            if gline is not None:
                for key in chain.LINE_KEYS:
                    g, w = gline[b, k, sg.LINE_SLOTS[key]], c["wline"][b, k][key]
                    if not flux:
                        assert g == 0.0 and w == 0.0
                        continue
                    worst["line"] = max(worst["line"], abs(g - w) / abs(w))
                    assert abs(g - w) < VJP_TOL * abs(w), (b, k, key, g, w)
    assert covered.all()  # the packer's blocks tile the row
    assert np.all(genv[..., 3:] == 0.0)  # delta (no DRAG on these lines) and the undifferentiated slots
    print(f"{name}: worst relative distance {worst}")
    if name == "window_M2_M3":
        # the use_t_before component with t_bin_start < 0: its offset s(t_before) is not zero
        comp = c["per"][0][1][1]
        ts_off = o.create_ts(*c["grid"][:3]) - comp["delay"]
        assert comp["use_t_before"] and ref.pwc_shape(2 * ts_off[0] - ts_off[1], comp)[0] != 0.0


def test_gaps_and_launch_log(prop, cases):
    """7. A row with doubles that belong to no block: they come back exactly 0, the blocks' cotangents bit for bit as in the
    packed layout, forward values too; the calls launch the table-aware kernels and one table cotangent kernel."""
    from c3_amd import _lib

    c = cases["drive_pwc_shape_sin"]
    B, T = c["tab"].shape
    names = {(k, e): c["per"][0][k][e]["shape"] for k in range(c["K"]) for e in range(2)}
    order = sorted((k, e) for (k, e), n in names.items() if n in sg.TAB_SHAPES)
    tidx2 = c["tidx"].copy()
    pos, moves = 5, []
    for k, e in reversed(order):  # blocks in reverse order, three doubles between them, five before, four after
        off, M = (int(x) for x in c["tidx"][k, e])
        ln = sg.table_block_len(names[k, e], M)
        tidx2[k, e, 0] = pos
        moves.append((off, pos, ln))
        pos += ln + 3
    T2 = pos + 1
    tab2 = np.full((B, T2), 1e300)  # what lies outside the blocks is never read
    inside = np.zeros(T2, dtype=bool)
    for off, new, ln in moves:
        tab2[:, new : new + ln] = c["tab"][:, off : off + ln]
        inside[new : new + ln] = True
    for dev in (False, True):
        packed, moved = _vjp(c, dev), _vjp(c, dev, tab2, tidx2)
        assert np.array_equal(packed[0], moved[0]) and np.array_equal(packed[1], moved[1])
        assert moved[2].shape == (B, T2) and np.all(moved[2][:, ~inside] == 0.0) and inside.sum() == T
        for off, new, ln in moves:
            assert np.array_equal(moved[2][:, new : new + ln], packed[2][:, off : off + ln])
        log = _lib.last_kernel_detail()
        assert all(k in log for k in ("awg_iq_kernel<true>", "mix_bwd_kernel", "awg_bwd_kernel<true>", "tab_bwd_kernel")), log
    sig = sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], env_tables=tab2, table_index=tidx2)
    log = _lib.last_kernel_detail()
    assert "awg_iq_kernel<true>" in log and "mix_kernel" in log
    assert np.array_equal(sig, _forward(c, False)[0])
    _vjp(cases["chain_flux_pwc_shape"], False)
    log = _lib.last_kernel_detail()
    assert all(k in log for k in ("awg_iq_kernel<true>", "chain_bwd_sample_kernel", "chain_bwd_awg_kernel", "awg_bwd_kernel<true>", "tab_bwd_kernel")), log


@pytest.mark.parametrize("device_resident", [False, True])
@pytest.mark.parametrize("route", ["drive", "chain"])
def test_all_analytic_problem_equals_existing_entries(prop, route, device_resident):
    """7. Closed-form components only, through c3p_synth_tab / c3p_synth_tab_vjp with an empty table (T = 0): bit for bit
    what c3p_synth_signals / c3p_synth_chain and their vjps return."""
    rng = np.random.default_rng(77)
    B, T = 3, 10e-9
    comps = lambda: [dict(_gauss(rng, T), delta=rng.uniform(-1, 1), use_t_before=True, drag=True),
                     dict(_scal(rng, T * 0.9), shape="flattop", t_up=T * 0.1, t_down=T * 0.7, risefall=T * 0.08, delay=T * 0.05)]
    per = [[comps(), comps()] for _ in range(B)]
    env, shapes, tab, tidx = sg.pack_table_components(_stack(per), B=B)
    assert tab.shape == (B, 0) and np.all(tidx == [-1, 0])
    carrier = np.stack([rng.uniform(0.6e9, 1.0e9, size=(B, 2)) * TWO_PI, rng.uniform(0.9e9, 1.1e9, size=(B, 2)) * TWO_PI], axis=-1)
    gs = rng.normal(size=(B, 2, 1000))
    kw = {}
    if route == "chain":
        packed = [sg.pack_lines([_flux(rng), {"kind": "drive"}], sim_res=SIM_RES) for _ in range(B)]
        kw = dict(line_kinds=packed[0][0], line_params=np.concatenate([p[1] for p in packed], axis=0))
    up = _dev if device_resident else (lambda x: x)
    args = (up(env), shapes, up(carrier), *GRID10)
    if device_resident and kw:
        kw["line_params"] = _dev(kw["line_params"])
    num = lambda x: x.cpu().numpy() if device_resident else x
    old = sg.synthesize_signals(*args, want_iq=True, **kw)
    new = sg.synthesize_signals(*args, want_iq=True, env_tables=up(tab), table_index=tidx, **kw)
    for x, y in zip(old, new):
        assert num(x).tobytes() == num(y).tobytes()
    old = sg.synthesize_signals_vjp(*args, up(gs), **kw)
    new = sg.synthesize_signals_vjp(*args, up(gs), env_tables=up(tab), table_index=tidx, **kw)
    assert len(new) == len(old) + 1 and tuple(new[-1].shape) == (B, 0)
    for x, y in zip(old, new):
        assert num(x).tobytes() == num(y).tobytes()
    assert np.abs(num(old[0])[:, :, 0, sg.ENV_SLOTS["delta"]]).min() > 0  # the DRAG rows took part


def test_goal_run_with_pwc_line(prop):
    """8. GRAPE's coordinates end to end: workloads.make_workload(1, B=2) (D = 3, N = 200), the AWG at 12 GS/s (Na = 24), one
    pwc line.  d goal / d (two inphase, one quadrature sample) from goal_run_with_grad, fused and three-call route, and from
    goal_run_ode_with_grad, against central differences of the goal through the CPU oracle on restated signals: 1e-6
    relative (tests/test_gpu_signal_chain.py:283); robust_goal_run_with_grad returns the mean over the batch."""
    from c3_amd import optimal_control as oc, workloads

    wl = workloads.make_workload(1, B=2)
    B, T, awg_res = 2, 2e-9, 12e9
    assert (wl.D, wl.N, wl.K) == (3, 200, 1) and sg.slice_num(0.0, T, SIM_RES) == 200 and sg.slice_num(0.0, T, awg_res) == 24
    rng = np.random.default_rng(9)
    per = [[[dict(shape="pwc", amp=1.0, xy_angle=0.2, freq_offset=0.0, t_final=T, inphase=rng.uniform(-1, 1, 24), quadrature=rng.uniform(-1, 1, 24))]] for _ in range(B)]
    _check_masks(per[0][0], (0.0, T, awg_res))
    env, shapes, tab, tidx = sg.pack_table_components(_stack(per), B=B, awg_samples=24)
    lo, v2hz = 5.05e9 * TWO_PI, 0.4e9 * TWO_PI
    carrier = np.tile(np.array([[lo, v2hz]]), (B, 1, 1))
    ideal = np.array([[0, 1], [1, 0]], dtype=complex)
    ts = o.create_ts(0.0, T, SIM_RES)
    init = np.array([[1], [0], [0]], dtype=complex)
    tgt = np.array([[1], [-1j], [0]], dtype=complex) / np.sqrt(2)

    def signal(b, key, j, h):
        c = dict(per[b][0][0])
        c[key] = c[key].copy()
        c[key][j] += h
        return ref.generate([c], lo, 0.0, T, awg_res, SIM_RES, v_to_hz=v2hz)["values"]

    def gate_goal(b, key="inphase", j=0, h=0.0):
        U = o.propagate_batch(wl.h0, wl.hks, signal(b, key, j, h)[None, None], ts[1] - ts[0])[0]
        return o.unitary_infid(ideal, U, index=[0], dims=[3])

    def state_goal(b, key="inphase", j=0, h=0.0):
        fin = o.ode_solver_arrays(wl.h0, wl.hks, signal(b, key, j, h)[None], ts, init, "rk4", "schrodinger", final_only=True)["states"]
        return 1 - abs(np.vdot(tgt, fin))

    runs = {f"fused={f}": oc.goal_run_with_grad(wl.h0, wl.hks, env, shapes, carrier, 0.0, T, awg_res, SIM_RES, ideal, [0], [3], fused=f, env_tables=tab, table_index=tidx) for f in (True, False)}
    for key in ("goal", "grad_env", "grad_carrier", "grad_tables"):
        x, y = (runs[f"fused={f}"][key].cpu().numpy() for f in (True, False))
        assert np.abs(x - y).max() <= 1e-12 * np.abs(y).max(), key
    runs["ode"] = oc.goal_run_ode_with_grad(wl.h0, wl.hks, env, shapes, carrier, 0.0, T, awg_res, SIM_RES, init, tgt, solver="rk4", env_tables=tab, table_index=tidx)
    h = 1e-5
    picks = {"fused=True": [("inphase", 3), ("inphase", 17), ("quadrature", 11)], "fused=False": [("inphase", 3), ("inphase", 17), ("quadrature", 11)], "ode": [("quadrature", 8)]}
    for name, r in runs.items():
        f = state_goal if name == "ode" else gate_goal
        goal, gtab = r["goal"].cpu().numpy(), r["grad_tables"].cpu().numpy()
        assert gtab.shape == (B, 48) and "grad_line" not in r
        for b in range(B):
            assert abs(goal[b] - f(b)) < 1e-9
            for key, j in picks[name]:
                fd = (f(b, key, j, h) - f(b, key, j, -h)) / (2 * h)
                got = gtab[b, j + (24 if key == "quadrature" else 0)]
                print(f"{name} b={b} {key}[{j}]: goal {goal[b]:.6f}  d goal {got:.9e} (fd {fd:.9e}, {abs(got - fd) / abs(fd):.2e})")
                assert abs(got - fd) < 1e-6 * abs(fd), (name, b, key, j)
    rb = oc.robust_goal_run_with_grad(wl.h0, wl.hks, env, shapes, carrier, 0.0, T, awg_res, SIM_RES, ideal, [0], [3], env_tables=tab, table_index=tidx)
    assert np.allclose(rb["grad_tables"].cpu().numpy(), runs["fused=True"]["grad_tables"].cpu().numpy().mean(axis=0), rtol=1e-12, atol=0)


def test_refusals_on_host_pointer_calls(prop, cases):
    """9. What the library refuses through c3p_last_error when it can look at its arguments (the raw entries: the Python
    layer refuses most of these before the call)."""
    import ctypes as C

    from c3_amd import _lib

    lib = _lib.load()
    c = cases["drive_pwc_shape_sin"]
    B, K, E, T = c["B"], c["K"], 2, c["tab"].shape[1]
    t0, t1, awg_res, sim_res = c["grid"]
    sig = np.empty((B, K, c["N"]))
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(env=c["env"], shapes=c["shapes"], tab=c["tab"], tidx=c["tidx"], T=T):
        env, shapes, tab, tidx = np.ascontiguousarray(env), np.ascontiguousarray(shapes, dtype=np.int32), np.ascontiguousarray(tab), np.ascontiguousarray(tidx, dtype=np.int32)
        rc = lib.c3p_synth_tab(p(env), p(shapes), p(tab), p(tidx), T, p(c["carrier"]), None, None, t0, t1, awg_res, sim_res, B, K, E, _lib.HOST_PTRS, None, p(sig), None)
        return rc, lib.c3p_last_error().decode()

    assert call()[0] == 0
    flags = sg.ENV_SLOTS["flags"]

    def edit(arr, where, value):
        out = arr.copy()
        out[where] = value
        return out

    # (k, e): [0,1] pwc at (0, 24), [1,0] pwc_shape at (48, 8), [1,1] fourier_sin at (58, 2)
    bad = {
        "pwc M != Na": (dict(tidx=edit(c["tidx"], (0, 1, 1), 23)), "Na"),
        "overlapping blocks": (dict(tidx=edit(c["tidx"], (1, 0, 0), 40)), "overlap"),
        "a block past T": (dict(tidx=edit(c["tidx"], (1, 1, 0), T - 5)), "leaves the row"),
        "DRAG on a table shape": (dict(env=edit(c["env"], (1, 1, 0, flags), float(sg.ENVF_DRAG))), "DRAG"),
        "T_BEFORE on pwc": (dict(env=edit(c["env"], (2, 0, 1, flags), float(sg.ENVF_T_BEFORE))), "T_BEFORE"),
        "one knot": (dict(tidx=edit(c["tidx"], (1, 0, 1), 1)), "M >= 2"),
        "t_bin_end <= t_bin_start": (dict(tab=edit(c["tab"], (0, 49), 1e-10)), "t_bin_end"),
        "unknown id": (dict(shapes=edit(c["shapes"], (0, 0), 12)), "id"),
    }
    for what, (kw, match) in bad.items():
        rc, msg = call(**kw)
        assert rc != 0 and match in msg, (what, msg)
    # a table id handed to the entries without a table
    for kw in ({}, dict(line_kinds=np.zeros(K, dtype=np.int32), line_params=np.zeros((B, K, sg.LINE_NPAR)))):
        with pytest.raises(Exception, match="C3:Error.*unknown shape id"):
            sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], **kw)
    rc = lib.c3p_synth_signals(p(c["env"]), p(c["shapes"]), p(c["carrier"]), t0, t1, awg_res, sim_res, B, K, E, _lib.HOST_PTRS, None, p(sig), None)
    assert rc != 0 and "C3P_ENV_*" in lib.c3p_last_error().decode()
    # the Python layer: the index table is checked before the call on either route
    with pytest.raises(Exception, match="C3:Error.*overlap"):
        sg.synthesize_signals(_dev(c["env"]), c["shapes"], _dev(c["carrier"]), *c["grid"], env_tables=_dev(c["tab"]), table_index=edit(c["tidx"], (1, 0, 0), 40))
    with pytest.raises(Exception, match="C3:Error.*go together"):
        sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], env_tables=c["tab"])
