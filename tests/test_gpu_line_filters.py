"""`c3p_synth_filt` on the GPU: distortion stages between DAC and Mixer, the DC offset and the crosstalk, against the numpy
restatement (tests/line_filter_ref.py, direct-sum route) on the smallest shapes where the convolution kernel can go wrong, its
vector-Jacobian product, the identities with the entries that were there before, and the route through goal_run_with_grad.
-m gpu.

The convolution kernel works on tiles of 1024 outputs (128 threads x 8 consecutive outputs each), stages 256 taps per LDS
chunk, and the mix / cotangent kernels on tiles of 256 samples.  The shapes: N = 64 (less than one register group of every
thread but the first eight), 300, 700 with Na = 16 (ragged tile, sim_res / awg_res = 43.75), 1030 (a second tile of six
outputs: one thread, a ragged register group), 2600 (three tiles, eleven tap chunks, eleven sample tiles)."""
import numpy as np
import pytest

import line_filter_ref as ref
from c3_amd import signals as sg
from oracle import c3_oracle as o
from test_line_filters import transmon_flux_iq
from test_signals import tunable_coupler_flux_component

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi
SIM_RES = 100e9
ENV_KEYS = ("amp", "xy_angle", "freq_offset", "delta")
chain = ref.chain


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


def _grid(N, Na, t0=0.0):
    """(t_end, awg_res) giving N simulation and Na AWG samples from t0 (the counts are truncations, devices.py:72-84)"""
    t1 = t0 + (N + 0.5) / SIM_RES
    awg_res = (Na + 0.5) / (t1 - t0)
    assert sg.slice_num(t0, t1, SIM_RES) == N and sg.slice_num(t0, t1, awg_res) == Na
    return t1, awg_res


def _rise(M):
    rt = (M + 0.5) / SIM_RES
    assert chain.response_tap_count(rt, SIM_RES) == M
    return rt


def _stage(rng, kind):
    if kind == "exp_iir":
        return {"kind": kind, "time_iir": rng.uniform(1e-9, 6e-9), "amp": rng.uniform(0.05, 0.25) * rng.choice([-1, 1])}
    if kind == "highpass_exp":
        return {"kind": kind, "time_hp": rng.uniform(15e-9, 60e-9)}
    if kind == "skin_effect":
        return {"kind": kind, "alpha": rng.uniform(1e-4, 4e-4)}
    return {"kind": "response_fft", "rise_time": _rise(int(kind[len("response_fft"):]))}


def _flux_line(rng, M):
    return dict(kind="flux", **({"rise_time": _rise(M)} if M else {}), phi_0=10.0 * rng.uniform(0.95, 1.05), phi=2.3 * rng.uniform(0.9, 1.1),
                omega_0=8.1e9 * TWO_PI * rng.uniform(0.95, 1.05), anhar=-286e6 * TWO_PI * rng.uniform(0.9, 1.1), d=0.36 * rng.uniform(0.9, 1.1))


def _components(rng, T, Na, table):
    comps = [dict(shape="gaussian_nonorm", amp=rng.uniform(0.5, 1.0), xy_angle=rng.uniform(-1, 3), freq_offset=rng.uniform(-60e6, 60e6) * TWO_PI, delta=rng.uniform(-1, 1),
                  t_final=T, sigma=T * rng.uniform(0.15, 0.3), use_t_before=True, drag=True),
             dict(shape="flattop", amp=rng.uniform(0.2, 0.5), xy_angle=rng.uniform(-1, 3), freq_offset=rng.uniform(-60e6, 60e6) * TWO_PI, delta=rng.uniform(-1, 1),
                  t_final=T * 0.9, t_up=T * 0.1, t_down=T * 0.7, risefall=T * 0.08, delay=T * 0.05)]
    if table:
        comps.append(dict(shape="pwc", amp=rng.uniform(0.3, 0.6), xy_angle=rng.uniform(-1, 3), freq_offset=rng.uniform(-60e6, 60e6) * TWO_PI, t_final=T,
                          inphase=rng.normal(size=Na), quadrature=rng.normal(size=Na)))
    return comps


# name -> N, Na, B, lines [(line kind, legacy Response taps or 0, stage kinds ("response_fftM": M taps))], and what else travels
SHAPES = {
    "N64_exp_iir": dict(N=64, Na=3, lines=[("drive", 0, ["exp_iir"])]),
    "N300_highpass": dict(N=300, Na=7, lines=[("drive", 0, ["highpass_exp"])]),
    "N700_skin_flux": dict(N=700, Na=16, lines=[("flux", 0, ["skin_effect"])]),
    "N2600_response_fft": dict(N=2600, Na=60, lines=[("drive", 0, ["response_fft300"])]),  # 300 taps: past one tap chunk
    "N1030_cascade": dict(N=1030, Na=24, lines=[("drive", 0, ["response_fft30", "exp_iir"])]),
    "N2600_exp_iir": dict(N=2600, Na=60, lines=[("flux", 0, ["exp_iir"])], dc=True),
    "legacy_and_stage": dict(N=700, Na=16, lines=[("flux", 30, ["exp_iir"])]),
    "B3_per_sample": dict(N=300, Na=7, B=3, lines=[("drive", 0, ["exp_iir", "skin_effect"])], dc=True),
    "K2_drive_flux_unused_slot": dict(N=700, Na=16, B=2, lines=[("drive", 0, ["highpass_exp", "exp_iir"]), ("flux", 12, ["skin_effect"])], dc=True, xtalk=True),
    "t_start_table": dict(N=300, Na=7, t0=3e-9, lines=[("drive", 7, ["exp_iir"])], table=True, dc=True),
    "K3_crosstalk_only": dict(N=300, Na=7, B=2, lines=[("drive", 0, []), ("flux", 0, []), ("drive", 0, [])], xtalk=True),
}


def _build(name, spec, seed):
    rng = np.random.default_rng(seed)
    N, Na, B, t0 = spec["N"], spec["Na"], spec.get("B", 1), spec.get("t0", 0.0)
    K = len(spec["lines"])
    t1, awg_res = _grid(N, Na, t0)
    table = spec.get("table", False)
    chans = [[_components(rng, t1 - t0, Na, table) for _ in range(K)] for _ in range(B)]
    lines = [[{"kind": "drive", **({"rise_time": _rise(M)} if M else {})} if kind == "drive" else _flux_line(rng, M) for kind, M, _ in spec["lines"]] for _ in range(B)]
    stages = [[[_stage(rng, s) for s in st] for _, _, st in spec["lines"]] for _ in range(B)]
    lo = rng.uniform(0.6e9, 1.0e9, size=(B, K)) * TWO_PI
    v2hz = rng.uniform(0.9e9, 1.1e9, size=(B, K)) * TWO_PI
    dc = rng.uniform(-0.2, 0.2, size=(B, K)) if spec.get("dc") else None
    xt = np.eye(K) + rng.uniform(-0.3, 0.3, size=(B, K, K)) if spec.get("xtalk") else None
    if table:
        packed = [sg.pack_table_components(c, awg_samples=Na) for c in chans]
        env, shapes, tab, tidx = np.concatenate([p[0] for p in packed]), packed[0][1], np.concatenate([p[2] for p in packed]), packed[0][3]
    else:
        env, shapes, tab, tidx = np.concatenate([sg.pack_components(c)[0] for c in chans]), sg.pack_components(chans[0])[1], None, None
    pl = [sg.pack_lines(row, sim_res=SIM_RES) for row in lines]
    kinds, par = pl[0][0], np.concatenate([p[1] for p in pl])
    pf = [sg.pack_line_filters([[{k: v for k, v in s.items()} for s in st] for st in row], sim_res=SIM_RES) for row in stages]
    fk, fp = pf[0][0], np.concatenate([p[1] for p in pf])
    gs = rng.normal(size=(B, K, N))
    pre = np.empty((B, K, N))
    kw = {}
    for b in range(B):
        for k in range(K):
            line = lines[b][k]
            comps = [c if c["shape"] == "pwc" else dict(c, shape=sg.ENV_SHAPES[c["shape"]]) for c in chans[b][k]]
            kw[b, k] = dict(components=comps, lo_freq=lo[b, k], stages=stages[b][k], dc=0.0 if dc is None else dc[b, k], kind=sg.LINE_KINDS[line["kind"]], v_to_hz=v2hz[b, k],
                            rise_time=line.get("rise_time", 0.0), line=line)
            a = dict(kw[b, k])
            pre[b, k] = ref.generate(a.pop("components"), a.pop("lo_freq"), t0, t1, awg_res, SIM_RES, **a)
    want = pre if xt is None else np.einsum("bkj,bjn->bkn", xt, pre)
    gpre = gs if xt is None else np.einsum("bkj,bkn->bjn", xt, gs)
    wx = None if xt is None else np.einsum("bkn,bjn->bkj", gs, pre)
    wv = {}
    for (b, k), a in kw.items():
        a = dict(a)
        wv[b, k] = ref.generate_vjp(a.pop("components"), a.pop("lo_freq"), t0, t1, awg_res, SIM_RES, gpre[b, k], **a)
    call = dict(line_kinds=kinds, line_params=par, line_filters=(fk, fp))
    if table:
        call.update(env_tables=tab, table_index=tidx)
    if dc is not None:
        call["dc_offset"] = dc
    if xt is not None:
        call["crosstalk"] = xt
    return dict(N=N, Na=Na, B=B, K=K, grid=(t0, t1, awg_res, SIM_RES), env=env, shapes=shapes, carrier=np.stack([lo, v2hz], axis=-1), call=call, chans=chans, lines=lines,
                stages=stages, fk=fk, gs=gs, want=want, pre=pre, wv=wv, wx=wx, tidx=tidx)


@pytest.fixture(scope="module")
def cases():
    """Every shape once: packed inputs, the restatement's signals and the restatement's vjp of one random cotangent."""
    return {name: _build(name, spec, 300 + i) for i, (name, spec) in enumerate(SHAPES.items())}


def _on_device(call):
    import torch

    dev = lambda x: torch.as_tensor(x, device="cuda:0")
    out = dict(call)
    for key in ("line_params", "env_tables", "dc_offset", "crosstalk"):
        if key in out:
            out[key] = dev(out[key])
    out["line_filters"] = (call["line_filters"][0], dev(call["line_filters"][1]))
    return out


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("device_resident", [False, True])
def test_filtered_lines_vs_restatement(prop, cases, name, device_resident):
    """1e-12 max|signal| per line (the bar of tests/test_signals.py:170)."""
    c = cases[name]
    if device_resident:
        import torch

        sig = sg.synthesize_signals(torch.as_tensor(c["env"], device="cuda:0"), c["shapes"], torch.as_tensor(c["carrier"], device="cuda:0"), *c["grid"], **_on_device(c["call"]))
        assert sig.is_cuda
    else:
        sig = sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], **c["call"])
    sig = _np(sig)
    assert sig.shape == c["want"].shape
    for b in range(c["B"]):
        for k in range(c["K"]):
            w = c["want"][b, k]
            err = np.abs(sig[b, k] - w).max()
            print(f"{name} [{b},{k}]: {err / np.abs(w).max():.3e} max|signal|")
            assert err < 1e-12 * np.abs(w).max(), (b, k)


def _vjp(c, device_resident):
    if device_resident:
        import torch

        dev = lambda x: torch.as_tensor(x, device="cuda:0")
        r = sg.synthesize_signals_vjp(dev(c["env"]), c["shapes"], dev(c["carrier"]), *c["grid"], dev(c["gs"]), **_on_device(c["call"]))
    else:
        r = sg.synthesize_signals_vjp(c["env"], c["shapes"], c["carrier"], *c["grid"], c["gs"], **c["call"])
    r = [_np(x) for x in r]
    out = {"env": r[0], "carrier": r[1], "line": r[2]}
    rest = r[3:]
    for key, flag in (("tab", "env_tables"), ("filt", "line_filters"), ("dc", "dc_offset"), ("xtalk", "crosstalk")):
        if flag in c["call"]:
            out[key] = rest.pop(0)
    assert not rest
    return out


def _close(got, want, top, what):
    """1e-10 of the entry, or of the largest entry of its array where the entry is smaller (tests/test_gpu_signal_chain.py:175)"""
    scale = max(abs(want), top)
    assert abs(got - want) <= 1e-10 * scale, (what, got, want, abs(got - want) / scale)
    return abs(got - want) / scale if scale else 0.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_filtered_vjp_vs_restatement(prop, cases, name):
    """Every output against the restatement's vjp of a random cotangent; two calls return the same bits, host-pointer and
    device-pointer calls too; undifferentiated and unused slots are exactly 0.  `top`, the largest entry of the array an
    entry is measured against when it is small itself, is taken over the entries of the same unit: the component's own four
    for the envelope rows (freq_offset, in seconds, at 1e-9 of it, as tests/test_gpu_signal_chain.py does), the same slot
    over the batch for stage parameters, the whole array for offsets and the crosstalk."""
    c = cases[name]
    g = _vjp(c, True)
    again, host = _vjp(c, True), _vjp(c, False)
    for key in g:
        assert np.array_equal(g[key], again[key]) and np.array_equal(g[key], host[key]), key
    B, K = c["B"], c["K"]
    F = c["fk"].shape[1]
    assert g["env"].shape == c["env"].shape and g["carrier"].shape == (B, K, 2) and g["line"].shape == (B, K, sg.LINE_NPAR) and g["filt"].shape == (B, K, F, sg.FILT_NPAR)
    worst = dict.fromkeys(g, 0.0)
    ftop = {}
    for (b, k), wv in c["wv"].items():
        for f, gst in enumerate(wv[3]):
            for key, val in gst.items():
                ftop[k, f, key] = max(ftop.get((k, f, key), 0.0), abs(val))
    for (b, k), (wcomp, wcar, wline, wst, wdc) in c["wv"].items():
        flux = c["lines"][b][k]["kind"] == "flux"
        for e, wg in enumerate(wcomp):
            top = max(abs(wg[x]) for x in ENV_KEYS if x in wg)
            for key in ENV_KEYS:
                want = wg.get(key, 0.0)
                worst["env"] = max(worst["env"], _close(g["env"][b, k, e, sg.ENV_SLOTS[key]], want, top * (1e-9 if key == "freq_offset" else 1.0), (b, k, e, key)))
            if "inphase" in wg:  # the pwc block of the table
                off, M = (int(x) for x in c["tidx"][k, e])
                wt = np.concatenate([wg["inphase"], wg["quadrature"]])
                for i in range(2 * M):
                    worst["tab"] = max(worst["tab"], _close(g["tab"][b, off + i], wt[i], np.abs(wt).max(), (b, k, e, i)))
        for i, key in enumerate(("lo_freq", "v_to_hz")):
            worst["carrier"] = max(worst["carrier"], _close(g["carrier"][b, k, i], wcar[key], 0.0, (b, k, key)))
        if flux:
            assert g["carrier"][b, k, 1] == 0.0
        for key in chain.LINE_KEYS:
            got = g["line"][b, k, sg.LINE_SLOTS[key]]
            if not flux:
                assert got == 0.0 and wline[key] == 0.0
                continue
            worst["line"] = max(worst["line"], _close(got, wline[key], 0.0, (b, k, key)))
        assert g["line"][b, k, sg.LINE_SLOTS["rise_time"]] == 0.0
        for f in range(F):
            row = g["filt"][b, k, f]
            if f >= len(wst):
                assert c["fk"][k, f] < 0 and np.all(row == 0.0)  # unused slot
                continue
            st = c["stages"][b][k][f]
            slots = {"time_iir": 0, "amp": 1, "time_hp": 0, "alpha": 0}
            for key, want in wst[f].items():
                worst["filt"] = max(worst["filt"], _close(row[slots[key]], want, ftop[k, f, key], (b, k, f, key)))
            if st["kind"] != "exp_iir":
                assert row[1] == 0.0
            if st["kind"] == "response_fft":
                assert row[0] == 0.0
        if "dc" in g:
            worst["dc"] = max(worst["dc"], _close(g["dc"][b, k], wdc, max(abs(v[4]) for v in c["wv"].values()), (b, k, "dc")))
    if "xtalk" in g:
        assert g["xtalk"].shape == (B, K, K)
        for idx in np.ndindex(B, K, K):
            worst["xtalk"] = max(worst["xtalk"], _close(g["xtalk"][idx], c["wx"][idx], np.abs(c["wx"]).max(), idx))
    if "tab" in g:
        used = np.zeros(g["tab"].shape[1], dtype=bool)
        for k, e in np.ndindex(*c["tidx"].shape[:2]):
            off, M = (int(x) for x in c["tidx"][k, e])
            if off >= 0:
                used[off : off + 2 * M] = True
        assert np.all(g["tab"][:, ~used] == 0.0)
    print(f"{name}: worst distance / scale {worst}")
    assert np.all(g["env"][..., 4:] == 0.0)


# ------------------------------------------------------------------------------------------------ goldens
def test_stored_transmon_signal_through_the_device(prop, golden_dir):
    """The flattop_cut samples of test/test_transmon_expanded.py as a pwc table component through a response_fft stage of 0.3 ns:
    N = 20, Na = 5, six taps, LO frequency 0, no V->Hz; 1e-12 max against the reference's stored signal."""
    g = np.load(golden_dir + "/transmon_expanded.npz")
    inph, quad = transmon_flux_iq()
    ts_awg = o.create_ts(0.0, 1e-9, 5e9)
    mask = o.envelope_mask(ts_awg, 1e-9, 1e-9)
    assert np.all(mask > 0.99)
    comp = dict(shape="pwc", amp=1.0, t_final=1e-9, inphase=inph / mask, quadrature=quad)
    env, shapes, tab, tidx = sg.pack_table_components([[comp]], awg_samples=5)
    filt = sg.pack_line_filters([[{"kind": "response_fft", "rise_time": 0.3e-9}]], sim_res=20e9)
    sig = sg.synthesize_signals(env, shapes, np.array([[[0.0, 1.0]]]), 0.0, 1e-9, 5e9, 20e9, env_tables=tab, table_index=tidx, line_filters=filt)
    assert sig.shape == (1, 1, 20)
    err = np.abs(sig[0, 0] - g["sig_q1"]).max()
    print(f"device ResponseFFT vs sig_q1: {err:.3e} = {err / np.abs(g['sig_q1']).max():.3e} max")
    assert err < 1e-12 * np.abs(g["sig_q1"]).max()


def test_long_line(prop):
    """The tunable-coupler flux line (N = 10 000, Na = 240, legacy Response of 30 taps; ten convolution tiles, forty tap chunks)
    with one exp_iir stage against the restatement: 1e-12 max|signal|, forward; the stage's two cotangents at 1e-10."""
    comp = dict(tunable_coupler_flux_component(), shape="flattop")
    env, shapes = sg.pack_components([[comp]])
    carrier = np.array([[[chain.TC_LO_FREQ, 1.0]]])
    line = dict(chain.TC_LINE, kind="flux", rise_time=chain.TC_RISE_TIME)
    kinds, par = sg.pack_lines([line], sim_res=SIM_RES)
    st = {"kind": "exp_iir", "time_iir": 12e-9, "amp": -0.15}
    filt = sg.pack_line_filters([[st]], sim_res=SIM_RES)
    sig = sg.synthesize_signals(env, shapes, carrier, *chain.TC_GRID, line_kinds=kinds, line_params=par, line_filters=filt)
    rcomp = [dict(comp, shape=sg.ENV_SHAPES["flattop"])]
    kw = dict(stages=[st], kind=chain.KIND_FLUX, rise_time=chain.TC_RISE_TIME, line=line)
    want = ref.generate(rcomp, chain.TC_LO_FREQ, *chain.TC_GRID, **kw)
    err = np.abs(sig[0, 0] - want).max()
    print(f"long line: {err / np.abs(want).max():.3e} max|signal|")
    assert err < 1e-12 * np.abs(want).max()
    gs = np.random.default_rng(9).normal(size=(1, 1, 10000))
    r = sg.synthesize_signals_vjp(env, shapes, carrier, *chain.TC_GRID, gs, line_kinds=kinds, line_params=par, line_filters=filt)
    wst = ref.generate_vjp(rcomp, chain.TC_LO_FREQ, *chain.TC_GRID, gs[0, 0], **kw)[3][0]
    for slot, key in enumerate(("time_iir", "amp")):
        print(f"long line d/d {key}: {r[3][0, 0, 0, slot]:.12e} (restatement {wst[key]:.12e})")
        assert abs(r[3][0, 0, 0, slot] - wst[key]) <= 1e-10 * abs(wst[key])


# ------------------------------------------------------------------------------------------------ identities
def test_no_stage_is_the_table_entry_bit_for_bit(prop, cases):
    """F = 0 with no offset and no crosstalk equals c3p_synth_tab's output, and so does an identity matrix with a zero offset;
    on a drive line without lines at all, and on a flux line with a legacy Response."""
    c = cases["t_start_table"]
    B, K = c["B"], c["K"]
    tabs = dict(env_tables=c["call"]["env_tables"], table_index=c["call"]["table_index"])
    none = (np.zeros((K, 0), dtype=np.int32), np.zeros((B, K, 0, sg.FILT_NPAR)))
    flux = sg.pack_lines([_flux_line(np.random.default_rng(1), 12)], sim_res=SIM_RES)
    for lines in ({}, dict(line_kinds=c["call"]["line_kinds"], line_params=c["call"]["line_params"]), dict(line_kinds=flux[0], line_params=flux[1])):
        plain = sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], **tabs, **lines)
        a = sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], **tabs, **lines, line_filters=none)
        b = sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], **tabs, **lines, dc_offset=np.zeros((B, K)), crosstalk=np.eye(K))
        assert np.abs(plain).max() > 0
        assert np.array_equal(a, plain) and np.array_equal(b, plain)


def test_exp_iir_without_amplitude_is_the_identity(prop, cases):
    """s(t) = 1: h = (1, 0, 0, ..), to 1e-12 max"""
    c = cases["N700_skin_flux"]
    lines = dict(line_kinds=c["call"]["line_kinds"], line_params=c["call"]["line_params"])
    plain = sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], **lines)
    filt = sg.pack_line_filters([[{"kind": "exp_iir", "time_iir": 3e-9, "amp": 0.0}]], sim_res=SIM_RES)
    got = sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], **lines, line_filters=filt)
    assert np.abs(got - plain).max() <= 1e-12 * np.abs(plain).max()


def test_crosstalk_makes_both_lines_equal(prop, cases):
    """the reference's own test_crosstalk: [[1,0],[1,0]]"""
    c = cases["K2_drive_flux_unused_slot"]
    call = dict(c["call"], crosstalk=sg.pack_crosstalk(["a", "b"], ["a", "b"], [[1, 0], [1, 0]]))
    got = sg.synthesize_signals(c["env"], c["shapes"], c["carrier"], *c["grid"], **call)
    assert np.array_equal(got[:, 0], got[:, 1])
    assert np.abs(got[:, 0] - c["pre"][:, 0]).max() <= 1e-12 * np.abs(c["pre"][:, 0]).max()


# ------------------------------------------------------------------------------------------------ errors and launch log
def test_filter_launch_log_and_errors(prop, cases):
    from c3_amd import _lib

    c = cases["K2_drive_flux_unused_slot"]
    args = (c["env"], c["shapes"], c["carrier"], *c["grid"])
    sg.synthesize_signals(*args, **c["call"])
    log = _lib.last_kernel_detail()
    fwd = ("awg_iq_kernel", "chain_taps_kernel", "filt_taps_kernel", "filt_up_kernel", "filt_conv_kernel", "filt_mix_kernel", "xtalk_fwd_kernel")
    assert all(k in log for k in fwd), log
    assert "chain_fwd_kernel" not in log and "mix_kernel" not in log.replace("filt_mix_kernel", "")
    sg.synthesize_signals_vjp(*args, c["gs"], **c["call"])
    log = _lib.last_kernel_detail()
    bwd = ("filt_conv_kernel", "filt_bwd_sample_kernel", "filt_par_kernel", "filt_bwd_awg_kernel", "xtalk_bwd_mat_kernel", "xtalk_bwd_sig_kernel", "awg_bwd_kernel")
    assert all(k in log for k in bwd), log
    # calls without the new keywords log what they log today
    lines = dict(line_kinds=c["call"]["line_kinds"], line_params=c["call"]["line_params"])
    sg.synthesize_signals(*args, **lines)
    log = _lib.last_kernel_detail()
    assert all(k in log for k in ("awg_iq_kernel", "chain_taps_kernel", "chain_fwd_kernel")) and "filt_" not in log and "xtalk" not in log
    sg.synthesize_signals(*args)
    log = _lib.last_kernel_detail()
    assert "mix_kernel" in log and "filt_" not in log and "chain_" not in log

    # refusals of the library itself (the packers' own are tests/test_line_filters.py): raw arrays, host pointers
    fk, fp = c["call"]["line_filters"]

    def call(fk=fk, fp=fp):
        lib = _lib.load()
        B, K, E = c["env"].shape[:3]
        F = c["fk"].shape[1]
        tidx = np.zeros((K, E, 2), dtype=np.int32)
        tidx[..., 0] = -1
        sig = np.empty((B, K, c["N"]))
        ptr = lambda a: None if a is None else a.ctypes.data
        env, shp, car = np.ascontiguousarray(c["env"]), np.ascontiguousarray(c["shapes"], dtype=np.int32), np.ascontiguousarray(c["carrier"])
        fk = None if fk is None else np.ascontiguousarray(fk, dtype=np.int32)
        fp = None if fp is None else np.ascontiguousarray(fp)
        t0, t1, awg_res, sim_res = c["grid"]
        _lib.check(lib.c3p_synth_filt(ptr(env), ptr(shp), None, ptr(tidx), 0, ptr(car), None, None, ptr(fk), ptr(fp), F, None, None, t0, t1, awg_res, sim_res, B, K, E,
                                      _lib.HOST_PTRS, None, ptr(sig), None))
        return sig

    assert np.isfinite(call()).all()

    def with_par(k, f, slot, v):
        p = fp.copy()
        p[0, k, f, slot] = v
        return p

    bad_kind = fk.copy()
    bad_kind[0, 0] = 4
    for kw, text in ((dict(fk=bad_kind), "C3P_FILT"), (dict(fp=with_par(0, 0, 0, 0.0)), "positive"), (dict(fp=with_par(0, 0, 0, np.inf)), "finite"),
                     (dict(fp=with_par(0, 1, 1, np.nan)), "finite"), (dict(fp=with_par(1, 0, 0, np.inf)), "finite"), (dict(fp=None), "go together"),
                     (dict(fk=None), "go together")):
        with pytest.raises(Exception, match="C3:Error.*" + text):
            call(**kw)
    fft = np.array([[0, -1], [-1, -1]], dtype=np.int32)
    with pytest.raises(Exception, match="C3:Error.*no ResponseFFT tap"):
        call(fk=fft, fp=np.full_like(fp, 0.001e-9))
    # the same through the Python layer
    with pytest.raises(Exception, match="C3:Error.*kind"):
        sg.synthesize_signals(*args, line_filters=(bad_kind, fp))
    with pytest.raises(Exception, match="C3:Error.*dc_offset"):
        sg.synthesize_signals(*args, dc_offset=np.zeros((1, 1)))
    with pytest.raises(Exception, match="C3:Error.*crosstalk"):
        sg.synthesize_signals(*args, crosstalk=np.eye(3))


# ------------------------------------------------------------------------------------------------ end to end
def test_goal_run_with_filtered_flux_line(prop):
    """The D = 3 flux-tuned transmon of test_goal_run_with_flux_line (T = 5 ns, N = 500, Na = 12, B = 2) with an exp_iir stage
    and a DC offset behind the mixer: d goal / d amp, d goal / d time_iir and d goal / d dc_offset from goal_run_with_grad
    against central differences of the goal through the CPU oracle's propagator on restated signals, 1e-6 relative (the bar of
    tests/test_signals.py:191).  Steps: 1e-6 for amp and the offset, 1e-6 relative for time_iir; on the CPU these and steps
    three times as large agree to 2e-8 relative or better.  robust_goal_run_with_grad over B = 4 offsets returns the means of the
    per-instance values."""
    from c3_amd import optimal_control as oc

    T, awg_res = 5e-9, 2.4e9
    assert sg.slice_num(0.0, T, SIM_RES) == 500 and sg.slice_num(0.0, T, awg_res) == 12
    B = 2
    a = np.diag(np.sqrt(np.arange(1, 3)), 1).astype(complex)
    n = a.conj().T @ a
    h0 = -286e6 * TWO_PI / 2 * (n @ n - n) + 15e6 * TWO_PI * (a + a.conj().T)
    hks = n[None]
    amps, phis, iir_amp, iir_t, dcs = [0.8, 1.1], [2.3, 2.1], [-0.12, 0.2], [1.5e-9, 0.9e-9], [0.03, -0.05]
    comp = lambda b: dict(shape="flattop", amp=amps[b], t_final=T, t_up=0.8e-9, t_down=T - 0.8e-9, risefall=0.5e-9, freq_offset=0.0, xy_angle=0.359)
    line = lambda b: dict(chain.TC_LINE, kind="flux", rise_time=chain.TC_RISE_TIME, phi=phis[b])
    stage = lambda b: {"kind": "exp_iir", "time_iir": iir_t[b], "amp": iir_amp[b]}
    env = np.concatenate([sg.pack_components([[comp(b)]])[0] for b in range(B)], axis=0)
    shapes = sg.pack_components([[comp(0)]])[1]
    packed = [sg.pack_lines([line(b)], sim_res=SIM_RES) for b in range(B)]
    kinds, par = packed[0][0], np.concatenate([p[1] for p in packed], axis=0)
    fk, fp = sg.pack_line_filters([[{"kind": "exp_iir", "time_iir": iir_t, "amp": iir_amp}]], B=B, sim_res=SIM_RES)
    lo = 829e6 * TWO_PI
    carrier = np.tile(np.array([[lo, 1.0]]), (B, 1, 1))
    ideal = np.eye(2, dtype=complex)
    dc = np.array(dcs)[:, None]
    kw = dict(line_kinds=kinds, line_params=par, line_filters=(fk, fp), dc_offset=dc)
    runs = [oc.goal_run_with_grad(h0, hks, env, shapes, carrier, 0.0, T, awg_res, SIM_RES, ideal, [0], [3], fused=fused, **kw) for fused in (True, False)]
    for key in ("goal", "grad_env", "grad_carrier", "grad_line", "grad_filters", "grad_dc_offset", "U"):
        x, y = runs[0][key].cpu().numpy(), runs[1][key].cpu().numpy()
        assert np.abs(x - y).max() <= 1e-12 * np.abs(y).max(), key
    ts = o.create_ts(0.0, T, SIM_RES)

    def goal(b, amp=None, t_iir=None, off=None):
        st = {"kind": "exp_iir", "time_iir": iir_t[b] if t_iir is None else t_iir, "amp": iir_amp[b] if amp is None else amp}
        sig = ref.generate([dict(comp(b), shape=o.ENV_FLATTOP)], lo, 0.0, T, awg_res, SIM_RES, stages=[st], dc=dcs[b] if off is None else off, kind=chain.KIND_FLUX,
                           rise_time=chain.TC_RISE_TIME, line=line(b))
        U = o.propagate_batch(h0, hks, sig[None, None], ts[1] - ts[0])[0]
        return o.unitary_infid(ideal, U, index=[0], dims=[3])

    h = 1e-6
    for fused, r in zip((True, False), runs):
        g, gf, gd = r["goal"].cpu().numpy(), r["grad_filters"].cpu().numpy(), r["grad_dc_offset"].cpu().numpy()
        assert gf.shape == (B, 1, 1, sg.FILT_NPAR) and gd.shape == (B, 1)
        for b in range(B):
            assert abs(g[b] - goal(b)) < 1e-9  # ten times the propagator bar (tests/test_gpu_parity.py TOL)
            ht = h * iir_t[b]
            fd = {"amp": (goal(b, amp=iir_amp[b] + h) - goal(b, amp=iir_amp[b] - h)) / (2 * h),
                  "time_iir": (goal(b, t_iir=iir_t[b] + ht) - goal(b, t_iir=iir_t[b] - ht)) / (2 * ht),
                  "dc_offset": (goal(b, off=dcs[b] + h) - goal(b, off=dcs[b] - h)) / (2 * h)}
            got = {"amp": gf[b, 0, 0, sg.FILT_SLOTS["amp"]], "time_iir": gf[b, 0, 0, sg.FILT_SLOTS["tau"]], "dc_offset": gd[b, 0]}
            for key in fd:
                print(f"fused={fused} b={b}: goal {g[b]:.6f}  d/d {key} {got[key]:.9e} (fd {fd[key]:.9e})")
                assert abs(got[key] - fd[key]) < 1e-6 * abs(fd[key]), key
    # noise instances: four members that differ in the offset alone
    offs = np.array([-0.04, -0.01, 0.02, 0.05])[:, None]
    rep = lambda x: np.repeat(x[:1], 4, axis=0)
    args = (h0, hks, rep(env), shapes, rep(carrier), 0.0, T, awg_res, SIM_RES, ideal, [0], [3])
    kw4 = dict(line_kinds=kinds, line_params=rep(par), line_filters=(fk, rep(fp)), dc_offset=offs)
    each = oc.goal_run_with_grad(*args, **kw4)
    mean = oc.robust_goal_run_with_grad(*args, **kw4)
    assert np.unique(each["goal"].cpu().numpy()).size == 4
    assert abs(mean["goal"].item() - each["goal"].cpu().numpy().mean()) < 1e-15
    for key in ("grad_env", "grad_line", "grad_filters", "grad_dc_offset"):
        x, y = mean[key].cpu().numpy(), each[key].cpu().numpy().mean(axis=0)
        assert x.shape == y.shape and np.abs(x - y).max() <= 1e-15 * np.abs(y).max(), key
