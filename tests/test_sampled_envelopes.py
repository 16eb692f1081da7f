"""Sampled and Fourier envelopes without a GPU: the numpy restatement (tests/sampled_envelope_ref.py) against the reference's
stored arrays and against finite differences of itself, the packer, and the shape table against the header."""
import os
import re

import numpy as np
import pytest

import sampled_envelope_ref as ref
from c3_amd import signals as sg
from c3_amd._lib import C3PropError
from oracle import c3_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_PI = 2 * np.pi
# the parameters of the reference's test/test_envelopes.py:34-39 and :85-90
PWC_SHAPE_PARAMS = dict(t_bin_start=1e-10, t_bin_end=9.9e-9, t_final=10e-9, inphase=[0, 0.1, 0.3, 0.5, 0.1, 1.1, 0.4, 0.1])
FOURIER_PARAMS = dict(amps=[0.5, 0.2], freqs=[1e6, 1e10], phases=[0, 1], t_final=10e-9)


@pytest.mark.parametrize("name", ["pwc_shape", "pwc_symmetric", "fourier_sin", "fourier_cos"])
def test_shapes_match_reference_arrays(golden_dir, name):
    """test/test_envelopes.py:33-50,84-102 on ts = linspace(0, 10e-9, 100), at the reference's own bar 1e-11 max."""
    want = np.load(golden_dir + "/envelopes.npz")[name]
    assert np.abs(want.imag).max() == 0.0
    want = want.real.reshape(-1)
    ts = np.linspace(0, 10e-9, 100)
    got = ref.REAL_SHAPES[name](ts, PWC_SHAPE_PARAMS if name.startswith("pwc") else FOURIER_PARAMS)
    err = np.abs(got - want).max()
    print(f"{name}: max distance {err:.3e}")
    assert got.shape == want.shape == (100,) and err < 1e-11 * np.max(want)


def test_golden_file_holds_only_the_four_arrays(golden_dir):
    assert sorted(np.load(golden_dir + "/envelopes.npz").files) == ["fourier_cos", "fourier_sin", "pwc_shape", "pwc_symmetric"]


GRID = (0.0, 10e-9, 2.4e9, 100e9)  # Na = 24, N = 1000
LO, V2HZ = 5.05e9 * TWO_PI, 1e9 * TWO_PI


def _fd_components():
    rng = np.random.default_rng(7)
    base = dict(amp=0.4, xy_angle=0.3, freq_offset=-50e6 * TWO_PI, t_final=8.2e-9, delay=0.6e-9)
    return {
        "pwc": dict(base, shape="pwc", inphase=rng.uniform(-1, 1, 24), quadrature=rng.uniform(-1, 1, 24)),
        "pwc_shape": dict(base, shape="pwc_shape", t_bin_start=-1.3e-9, t_bin_end=7.1e-9, inphase=rng.uniform(-1, 1, 7), use_t_before=True),
        "pwc_symmetric": dict(base, shape="pwc_symmetric", t_bin_start=0.2e-9, t_bin_end=4.4e-9, inphase=rng.uniform(-1, 1, 5)),
        "fourier_sin": dict(base, shape="fourier_sin", amps=rng.uniform(-1, 1, 3), freqs=rng.uniform(1e8, 3e9, 3), phases=rng.uniform(-1, 1, 3), use_t_before=True),
        "fourier_cos": dict(base, shape="fourier_cos", amps=rng.uniform(-1, 1, 3), freqs=rng.uniform(1e8, 3e9, 3), use_t_before=True),
    }


def _close(fd, an, rtol):
    return abs(fd - an) < rtol * abs(fd) or fd == an == 0.0  # tests/test_signals.py:201-204


@pytest.mark.parametrize("name", list(ref.TAB_NAMES))
@pytest.mark.parametrize("line", ["drive", "flux"])
def test_restatement_vjp_matches_finite_differences(name, line):
    """The vjp the device is pinned to against central differences of the restatement's own forward, every coefficient of
    every kind and the three scalar slots: 1e-7 relative, the bar of tests/test_signals.py:230-232.  Steps on the drive line
    as there (1e-6; 1e3 rad/s for the frequencies).  The flux line's values are ~5e10 rad/s, so the sum f ~ 3e11 carries a
    rounding of ~7e-5: over 2e-6 that is 7e-7 of a gradient of 5e7.  There the steps are 1e-4 and 1e4 rad/s (rounding 7e-9,
    truncation h^2/6 < 2e-9 relative: the phases move by at most 1e-4)."""
    comp = _fd_components()[name]
    other = dict(shape=o.ENV_GAUSSIAN_NONORM, amp=0.3, xy_angle=-0.2, freq_offset=20e6 * TWO_PI, t_final=9e-9, sigma=2e-9)
    kw = dict(kind=ref.chain.KIND_FLUX, rise_time=ref.chain.TC_RISE_TIME, line=ref.chain.TC_LINE) if line == "flux" else dict(v_to_hz=V2HZ)
    lo = ref.chain.TC_LO_FREQ if line == "flux" else LO
    gs = np.random.default_rng(3).normal(size=sg.slice_num(*GRID[:2], GRID[3]))
    f = lambda c: float(np.sum(gs * ref.generate([other, c], lo, *GRID, **kw)["values"]))
    (_, g), _, _ = ref.generate_vjp([other, comp], lo, *GRID, gs, **kw)
    h_val, h_freq = (1e-4, 1e4) if line == "flux" else (1e-6, 1e3)
    for key, h in (("amp", h_val), ("xy_angle", h_val), ("freq_offset", h_freq)):
        fd = (f(dict(comp, **{key: comp[key] + h})) - f(dict(comp, **{key: comp[key] - h}))) / (2 * h)
        assert _close(fd, g[key], 1e-7), (key, fd, g[key])
    for key in ref.TAB_ARRAYS[name]:
        h = h_freq if key == "freqs" else h_val
        assert g[key].shape == np.shape(comp[key])
        for m in range(len(comp[key])):
            step = np.zeros(len(comp[key]))
            step[m] = h
            fd = (f(dict(comp, **{key: comp[key] + step})) - f(dict(comp, **{key: comp[key] - step}))) / (2 * h)
            assert _close(fd, g[key][m], 1e-7), (key, m, fd, g[key][m])
    if name == "pwc_shape":
        # the window (t_final = 8.2 ns) ends before t_bin_end: the last knot's hat still reaches into it; t_before weighs knot 0
        assert g["inphase"][-1] != 0.0 and comp["t_bin_start"] < 0


def test_table_shape_ids_match_header():
    text = open(os.path.join(ROOT, "include", "c3prop.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define C3P_ENVT_([A-Z_]+) (\d+)", text)}
    first, end = defs.pop("FIRST"), defs.pop("END")
    assert defs == {k.upper(): v for k, v in sg.TAB_SHAPES.items()}
    assert first == min(defs.values()) and end == max(defs.values()) + 1 and first > max(sg.ENV_SHAPES.values())
    assert set(sg.TAB_SHAPES) == set(ref.TAB_NAMES) == set(sg.TAB_LAYOUT)
    assert not set(sg.TAB_SHAPES) & set(sg.ENV_SHAPES)


def _channels(B):
    rng = np.random.default_rng(11)
    return [
        [dict(shape="gaussian_nonorm", amp=0.5, t_final=10e-9, sigma=2e-9), dict(shape="pwc", amp=1.0, t_final=10e-9, inphase=rng.normal(size=(B, 24)), quadrature=rng.normal(size=24))],
        [dict(shape="pwc_shape", amp=0.7, t_final=10e-9, t_bin_start=1e-10, t_bin_end=np.linspace(9e-9, 9.9e-9, B), inphase=rng.normal(size=8), use_t_before=True),
         dict(shape="fourier_sin", amp=0.2, t_final=10e-9, amps=[0.5, 0.2], freqs=rng.uniform(1e6, 1e10, size=(B, 2)), phases=[0.0, 1.0])],
        [dict(shape="fourier_cos", amp=0.2, t_final=10e-9, amps=[0.5, 0.2, 0.1], freqs=[1e6, 1e9, 1e10])],
    ]


def test_packer_layout():
    B = 3
    ch = _channels(B)
    env, shapes, tab, idx = sg.pack_table_components(ch, B=B, awg_samples=24)
    assert env.shape == (B, 3, 2, sg.ENV_NPAR) and shapes.shape == (3, 2) and idx.shape == (3, 2, 2)
    assert shapes.dtype == np.int32 and idx.dtype == np.int32 and tab.dtype == np.float64 and tab.flags["C_CONTIGUOUS"]
    assert shapes.tolist() == [[2, 16], [17, 19], [20, -1]]
    # blocks follow each other in component order: pwc 2*24, pwc_shape 2+8, fourier_sin 3*2, fourier_cos 2*3
    assert idx.tolist() == [[[-1, 0], [0, 24]], [[48, 8], [58, 2]], [[64, 3], [-1, 0]]]
    assert tab.shape == (B, 70)
    for b in range(B):
        assert np.array_equal(tab[b, 0:24], ch[0][1]["inphase"][b]) and np.array_equal(tab[b, 24:48], ch[0][1]["quadrature"])
        assert tab[b, 48] == 1e-10 and tab[b, 49] == ch[1][0]["t_bin_end"][b] and np.array_equal(tab[b, 50:58], ch[1][0]["inphase"])
        assert np.array_equal(tab[b, 58:60], [0.5, 0.2]) and np.array_equal(tab[b, 60:62], ch[1][1]["freqs"][b]) and np.array_equal(tab[b, 62:64], [0.0, 1.0])
        assert np.array_equal(tab[b, 64:70], [0.5, 0.2, 0.1, 1e6, 1e9, 1e10])
    # the rows are what pack_components makes of the scalar slots; flags carry use_t_before
    assert env[0, 1, 0, sg.ENV_SLOTS["amp"]] == 0.7 and env[2, 1, 0, sg.ENV_SLOTS["flags"]] == sg.ENVF_T_BEFORE and env[0, 0, 1, sg.ENV_SLOTS["flags"]] == 0
    assert all(sg.table_block_len(n, 5) == len(sc) + 5 * len(ar) for n, (sc, ar) in sg.TAB_LAYOUT.items())
    # the input dicts are left as they were
    assert ch[0][1]["shape"] == "pwc" and "inphase" in ch[0][1]


def test_packer_per_sample_equals_shared():
    """Arrays and scalars given once are what B equal per-sample copies give."""
    B = 3
    shared = [[dict(shape="pwc_symmetric", amp=1.0, t_final=10e-9, t_bin_start=1e-10, t_bin_end=4e-9, inphase=[0.1, 0.4, 0.2]),
               dict(shape="fourier_sin", amp=1.0, t_final=10e-9, amps=[0.5, 0.2], freqs=[1e6, 1e10], phases=[0.0, 1.0])]]
    tiled = [[{k: (np.tile(np.asarray(v, dtype=float), (B,) + (1,) * np.ndim(v)) if k in ("inphase", "t_bin_start", "t_bin_end", "amps", "freqs", "phases") else v) for k, v in c.items()}
              for c in shared[0]]]
    a, b = sg.pack_table_components(shared, B=B), sg.pack_table_components(tiled, B=B)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[2].shape == (B, 5 + 6)
    # all-analytic channels: an empty table, every index (-1, 0), rows and shapes those of pack_components
    plain = [[dict(shape="rect", amp=1.0, t_final=1e-9)]]
    env, shapes, tab, idx = sg.pack_table_components(plain, B=2)
    assert tab.shape == (2, 0) and idx.tolist() == [[[-1, 0]]]
    assert np.array_equal(env, sg.pack_components(plain, B=2)[0]) and np.array_equal(shapes, sg.pack_components(plain, B=2)[1])


@pytest.mark.parametrize("comp, match", [
    (dict(shape="pwc", inphase=np.zeros(24), quadrature=np.zeros(23)), "quadrature"),
    (dict(shape="pwc", inphase=np.zeros(23), quadrature=np.zeros(23)), "AWG sample"),
    (dict(shape="pwc", inphase=np.zeros(24), quadrature=np.zeros(24), use_t_before=True), "use_t_before"),
    (dict(shape="pwc", inphase=np.zeros(24), quadrature=np.zeros(24), drag=True), "DRAG"),
    (dict(shape="pwc", inphase=np.zeros(24)), "quadrature"),
    (dict(shape="pwc_shape", t_bin_start=0.0, t_bin_end=1e-9, inphase=[1.0]), "two knots"),
    (dict(shape="pwc_symmetric", t_bin_start=1e-9, t_bin_end=1e-9, inphase=[1.0, 2.0]), "t_bin_end"),
    (dict(shape="pwc_shape", t_bin_start=0.0, t_bin_end=1e-9, inphase=[1.0, 2.0], drag=True), "DRAG"),
    (dict(shape="pwc_shape", t_bin_start=0.0, inphase=[1.0, 2.0]), "t_bin_end"),
    (dict(shape="fourier_sin", amps=[1.0, 2.0], freqs=[1.0], phases=[0.0, 0.0]), "freqs"),
    (dict(shape="fourier_cos", amps=np.zeros((3, 2)), freqs=[1.0, 2.0]), r"\[M\] or \[2,M\]"),
    (dict(shape="fourier_cos", amps=[], freqs=[]), "empty"),
    (dict(shape="rect", inphase=[1.0, 2.0]), "array parameter"),
    (dict(shape="slepian_fourier"), "not available"),
])
def test_packer_refusals(comp, match):
    with pytest.raises(C3PropError, match="C3:Error.*" + match):
        sg.pack_table_components([[dict(comp, amp=1.0, t_final=10e-9)]], B=2, awg_samples=24)


def test_pack_components_still_refuses_table_shapes():
    for name in sg.TAB_SHAPES:
        with pytest.raises(C3PropError, match="not available on the device"):
            sg.pack_components([[dict(shape=name, amp=1.0, t_final=1e-9, inphase=[0.0, 1.0])]])
    assert len(sg.pack_components([[dict(shape="rect", amp=1.0, t_final=1e-9)]])) == 2
