"""The six synthesis entries (`c3p_synth_signals`, `c3p_synth_chain`, `c3p_synth_tab` and their vjps) pinned to recorded runs:
for every entry, with and without lines and table where it takes them, on host and on device pointers, the launch log and the
sha256 of every output equal what tests/golden/synth_entries.json holds (written by tests/golden/make_golden_synth_entries.py
from the library before the entries were given one call record).  The kernels use no atomics, so the bits repeat.  -m gpu."""
import hashlib
import json

import numpy as np
import pytest

TWO_PI = 2 * np.pi
GRID = (0.0, 3e-9, 2e9, 100e9)  # N = 300, Na = 6: two chain tiles, the second ragged
B, K, E, N, NA = 3, 2, 2, 300, 6
T_TABLE = 25  # pwc block [0,12) | 4 unused doubles | fourier_sin block [16,25)
# configuration -> (a coefficient table travels, T > 0, lines travel); the entry follows from the first and the last
CONFIGS = {
    "signals": (False, False, False),
    "chain": (False, False, True),
    "tab25": (True, True, False),
    "tab25_lines": (True, True, True),
    "tab0": (True, False, False),
    "tab0_lines": (True, False, True),
}
MODES = ("forward", "forward_iq", "vjp")
ROUTES = ("host", "device")
CASE_IDS = [f"{c}-{m}-{r}" for c in CONFIGS for m in MODES for r in ROUTES]


def make_inputs(sg, config):
    """(env, shapes, carrier, grad_signals, keywords) of a configuration, all numpy, from a generator seeded per configuration"""
    table, filled, lines = CONFIGS[config]
    rng = np.random.default_rng(2200 + list(CONFIGS).index(config))
    T = GRID[1]
    scal = lambda **kw: dict(amp=rng.uniform(0.3, 1.0, B), xy_angle=rng.uniform(-1, 3, B), freq_offset=rng.uniform(-60e6, 60e6, B) * TWO_PI, t_final=T, **kw)
    closed = [
        [scal(shape="gaussian_nonorm", sigma=T * rng.uniform(0.15, 0.3, B), delta=rng.uniform(-1, 1, B), drag=True), scal(shape="cosine")],
        [scal(shape="flattop", t_up=0.4e-9, t_down=2.5e-9, risefall=0.3e-9), scal(shape="gaussian_nonorm", sigma=T / 5, use_t_before=True)],
    ]
    kw = {}
    if filled:
        chans = [
            [scal(shape="pwc", inphase=rng.uniform(-1, 1, (B, NA)), quadrature=rng.uniform(-1, 1, (B, NA))), closed[0][1]],
            [scal(shape="fourier_sin", amps=rng.uniform(-1, 1, (B, 3)), freqs=rng.uniform(1e8, 3e9, (B, 3)), phases=rng.uniform(-1, 1, (B, 3))), closed[1][0]],
        ]
        env, shapes, packed, index = sg.pack_table_components(chans, B=B, awg_samples=NA)
        assert packed.shape == (B, 21) and index[0, 0].tolist() == [0, NA] and index[1, 0].tolist() == [12, 3]
        tab = rng.uniform(-1, 1, (B, T_TABLE))  # the gap holds numbers nothing may read
        tab[:, :12], tab[:, 16:] = packed[:, :12], packed[:, 12:]
        index[1, 0, 0] = 16
        kw.update(env_tables=tab, table_index=index)
    elif table:
        env, shapes, tab, index = sg.pack_table_components(closed, B=B, awg_samples=NA)
        assert tab.shape == (B, 0)
        kw.update(env_tables=tab, table_index=index)
    else:
        env, shapes = sg.pack_components(closed, B=B)
    assert env.shape == (B, K, E, sg.ENV_NPAR)
    if lines:
        flux = dict(kind="flux", rise_time=rng.uniform(0.45e-9, 0.55e-9, B), phi_0=10.0, phi=2.3 * rng.uniform(0.9, 1.1, B), omega_0=8.1e9 * TWO_PI, anhar=-286e6 * TWO_PI, d=0.36)
        kinds, par = sg.pack_lines([flux, {"kind": "drive"}], B=B, sim_res=GRID[3])
        kw.update(line_kinds=kinds, line_params=par)
    carrier = np.stack([rng.uniform(4e9, 6e9, (B, K)) * TWO_PI, rng.uniform(0.9e9, 1.1e9, (B, K)) * TWO_PI], axis=-1)
    return env, shapes, carrier, rng.normal(size=(B, K, N)), kw


def run_cases(sg, _lib):
    """Every case once -> {case id: {"log": launch log, "sha256": [digest of each output, in the order returned]}}.  `sg` and
    `_lib` are the modules of the library under test (the golden script hands over those of another tree)."""
    import torch

    assert (sg.slice_num(*GRID[:2], GRID[3]), sg.slice_num(*GRID[:3])) == (N, NA)
    dev = torch.device("cuda:0")
    out = {}
    for config in CONFIGS:
        env, shapes, carrier, gs, kw = make_inputs(sg, config)
        for route in ROUTES:
            up = (lambda a: torch.as_tensor(a, device=dev)) if route == "device" else (lambda a: a)
            args = (up(env), up(shapes), up(carrier)) + GRID
            kwr = {k: up(v) for k, v in kw.items()}
            for mode in MODES:
                if mode == "vjp":
                    res = sg.synthesize_signals_vjp(*args, up(gs), **kwr)
                else:
                    res = sg.synthesize_signals(*args, want_iq=mode == "forward_iq", **kwr)
                log = _lib.last_kernel_detail()
                res = res if isinstance(res, tuple) else (res,)
                arrays = [np.ascontiguousarray(r.cpu().numpy() if route == "device" else r) for r in res]
                assert all(np.isfinite(a).all() for a in arrays) and any(a.any() for a in arrays), (config, mode, route)
                out[f"{config}-{mode}-{route}"] = {"log": log, "sha256": [hashlib.sha256(a.tobytes()).hexdigest() for a in arrays]}
    return out


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(golden_dir + "/synth_entries.json"))["cases"]


@pytest.fixture(scope="module")
def results(lib):
    from c3_amd import _lib
    from c3_amd import signals as sg

    _lib.require_gpu()
    return run_cases(sg, _lib)


def test_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(CASE_IDS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASE_IDS)
def test_entry_is_the_recorded_one(results, golden, case):
    """the same kernels in the same order, and the same bits in every output"""
    config, mode, _ = case.split("-")
    table, _, lines = CONFIGS[config]
    entry = ("c3p_synth_tab" if table else "c3p_synth_chain" if lines else "c3p_synth_signals") + ("_vjp" if mode == "vjp" else "")
    got, want = results[case], golden[case]
    n_out = {"forward": 1, "forward_iq": 2}.get(mode, 2 + lines + table)
    assert len(want["sha256"]) == n_out, entry
    assert got["log"] == want["log"], entry
    assert got["sha256"] == want["sha256"], entry
