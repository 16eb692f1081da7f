"""Signal synthesis and its vector-Jacobian product on long pulses, offset windows and uneven AWG / simulation rate ratios,
against the oracle; and the whole optimiser step on such a window against central differences of the oracle pipeline.

mix_bwd_kernel walks the simulation samples one AWG sample feeds, 64 per wavefront pass, and awg_bwd_kernel the AWG samples
of a line, 64 per lane pass: the 60 ns grid takes both loops through a second pass, the 100 ns grid awg_bwd_kernel through
four."""
import numpy as np
import pytest

from c3_amd import signals as sg
from oracle import c3_oracle as o

TWO_PI = 2 * np.pi

# name: ((t_start, window, awg_res, sim_res), (N, Na) as Device.calc_slice_num counts them)
GRIDS = {
    "60ns_from_3ns": ((3e-9, 60e-9, 1.2e9, 100e9), (5999, 72)),  # 83.3 simulation samples per AWG sample; span x rate < 6000
    "100ns": ((0.0, 100e-9, 2.4e9, 100e9), (10000, 240)),
    "40ns_from_1.5ns": ((1.5e-9, 40e-9, 0.8e9, 100e9), (4000, 32)),  # 125 per AWG sample
    "33ns_from_-2ns": ((-2e-9, 33e-9, 1e9, 333e9), (10989, 33)),  # 333 per AWG sample, negative start
    "awg_finer": ((0.0, 20e-9, 100e9, 50e9), (1000, 2000)),  # every other AWG sample feeds nothing
    "ratio_1": ((0.0, 5e-9, 4e9, 4e9), (20, 20)),
}
DRIVEN = ["rect", "gaussian_nonorm", "flattop", "flattop_risefall", "cosine", "gaussian_sigma", "gaussian", "trapezoid"]
# every shape x (use_t_before, drag), dealt onto lines of 4, 5, 1, 2, 3, 4, 5, 4 and 4 components; line 0 keeps an unused
# (-1) slot between its used ones
COMBOS = [(s, tb, dr) for s in DRIVEN for tb in (False, True) for dr in (False, True)]
COUNTS = [4, 5, 1, 2, 3, 4, 5, 4, 4]
GAP = (0, 2)


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import _lib, propagation

    _lib.require_gpu()
    return propagation


def _grid(name):
    (t0, window, awg_res, sim_res), (N, Na) = GRIDS[name]
    return t0, t0 + window, awg_res, sim_res, N, Na


def _all_combos():
    it = iter(COMBOS)
    return [[next(it) for _ in range(n)] for n in COUNTS]


def _problem(rng, B, window, layout):
    """channels_b[b][k]: the component dicts of line k in sample b (shapes and flags shared by the batch); carrier [B,K,2]."""

    def comp(shape, use_t_before, drag):
        T = window * rng.uniform(0.5, 0.85)
        return dict(shape=shape, amp=rng.uniform(0.1, 0.6), xy_angle=rng.uniform(-1, 3), freq_offset=rng.uniform(-60e6, 60e6) * TWO_PI,
                    delta=rng.uniform(-1, 1), t_final=T, sigma=T * rng.uniform(0.15, 0.3), t_up=T * 0.1, t_down=T * rng.uniform(0.6, 0.8),
                    risefall=T * rng.uniform(0.05, 0.1), delay=window * rng.uniform(0.02, 0.1), use_t_before=use_t_before, drag=drag)

    channels_b = [[[comp(*c) for c in line] for line in layout] for _ in range(B)]
    K = len(layout)
    carrier = np.stack([rng.uniform(4.5e9, 6e9, size=(B, K)) * TWO_PI, rng.uniform(0.9e9, 1.1e9, size=(B, K)) * TWO_PI], axis=-1)
    return channels_b, carrier


def _pack(channels_b, gap=None):
    """(env [B,K,E,NPAR], shapes [K,E]); a gap slot holds a nonzero row under shape id -1, which the kernels must skip."""
    env = []
    for chans in channels_b:
        chans = [list(c) for c in chans]
        if gap is not None:
            chans[gap[0]].insert(gap[1], dict(shape="rect", amp=5.0, xy_angle=1.0, freq_offset=1e9, delta=2.0, t_final=1e-9, drag=True))
        e, shapes = sg.pack_components(chans, B=1)
        env.append(e)
    if gap is not None:
        shapes[gap] = -1
    return np.concatenate(env), shapes


def _oracle_line(comps):
    return [dict(c, shape=sg.ENV_SHAPES[c["shape"]]) for c in comps]


def _oracle(channels_b, carrier, t0, t1, awg_res, sim_res):
    """signals [B,K,N] and I/Q [B,K,2,Na] from the oracle, one line at a time."""
    r = [[o.generate_signal(_oracle_line(comps), carrier[b, k, 0], carrier[b, k, 1], t0, t1, awg_res, sim_res) for k, comps in enumerate(chans)]
         for b, chans in enumerate(channels_b)]
    return np.array([[x["values"] for x in rb] for rb in r]), np.array([[[x["inphase"], x["quadrature"]] for x in rb] for rb in r])


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _check_vjp(channels_b, env, shapes, carrier, grid, gs):
    """Host- and device-pointer calls agree bitwise, and so does a repeated call; every (b, k) matches the oracle VJP within
    the bounds of test_signals.test_synthesis_vjp_vs_oracle; unused slots and entries, and delta without DRAG, are exactly 0."""
    import torch

    t0, t1, awg_res, sim_res, _, _ = _grid(grid)
    host = sg.synthesize_signals_vjp(env, shapes, carrier, t0, t1, awg_res, sim_res, gs)
    dev = lambda x: torch.as_tensor(x, device="cuda:0")
    runs = [[x.cpu().numpy() for x in sg.synthesize_signals_vjp(dev(env), dev(shapes), dev(carrier), t0, t1, awg_res, sim_res, dev(gs))] for _ in range(2)]
    for h, d0, d1 in zip(host, *runs):
        assert np.array_equal(_bits(h), _bits(d0)), "host-pointer and device-pointer calls differ"
        assert np.array_equal(_bits(d0), _bits(d1)), "two identical calls differ"
    genv, gcar = host
    B, K, E = genv.shape[:3]
    for b in range(B):
        for k in range(K):
            comps = channels_b[b][k]
            want, wcar = o.generate_signal_vjp(_oracle_line(comps), carrier[b, k, 0], carrier[b, k, 1], t0, t1, awg_res, sim_res, gs[b, k])
            used = [e for e in range(E) if shapes[k, e] >= 0]
            assert len(used) == len(want) == len(comps)
            for e, wg, c in zip(used, want, comps):
                for key in ("amp", "xy_angle", "freq_offset", "delta"):
                    scale = max(abs(wg[key]), 1e-12 * np.abs(gs).max() * carrier[b, k, 1])
                    tol = 1e-10 * max(scale, max(abs(x) for x in wg.values()) * (1e-9 if key == "freq_offset" else 1.0))
                    assert abs(genv[b, k, e, sg.ENV_SLOTS[key]] - wg[key]) < tol, (grid, b, k, e, key)
                if not c["drag"]:
                    assert genv[b, k, e, sg.ENV_SLOTS["delta"]] == 0.0, (grid, b, k, e)
            assert abs(gcar[b, k, 0] - wcar["lo_freq"]) < 1e-10 * abs(wcar["lo_freq"]) + 1e-20, (grid, b, k)
            assert abs(gcar[b, k, 1] - wcar["v_to_hz"]) < 1e-10 * abs(wcar["v_to_hz"]) + 1e-20, (grid, b, k)
    assert np.all(genv[..., sg.ENV_SLOTS["delta"] + 1 :] == 0.0)
    assert np.all(genv[:, shapes < 0] == 0.0)


def test_grids_reach_what_they_are_named_for():
    for name in GRIDS:
        t0, t1, awg_res, sim_res, N, Na = _grid(name)
        assert (sg.slice_num(t0, t1, sim_res), sg.slice_num(t0, t1, awg_res)) == (N, Na), name
    _, _, _, _, N, Na = _grid("60ns_from_3ns")
    assert N // Na > 64 and Na > 64  # every AWG sample feeds two wavefront passes; two lane passes per line
    assert _grid("100ns")[5] > 3 * 64
    assert sorted(c for line in _all_combos() for c in line) == sorted(COMBOS) and len(set(COMBOS)) == 32


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("device_resident", [False, True])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_synthesis_on_grid(prop, grid, device_resident):
    """All 32 shape / flag combinations on 9 lines of 1 to 5 components, B = 3, against the oracle; with and without the
    I/Q output (without it the I/Q rows live in the library's workspace)."""
    t0, t1, awg_res, sim_res, N, Na = _grid(grid)
    rng = np.random.default_rng(100 + list(GRIDS).index(grid))
    channels_b, carrier = _problem(rng, 3, GRIDS[grid][0][1], _all_combos())
    env, shapes = _pack(channels_b, GAP)
    want, want_iq = _oracle(channels_b, carrier, t0, t1, awg_res, sim_res)
    device = "cuda:0" if device_resident else None
    sig, iq = sg.synthesize_signals(env, shapes, carrier, t0, t1, awg_res, sim_res, want_iq=True, device=device)
    sig_ws = sg.synthesize_signals(env, shapes, carrier, t0, t1, awg_res, sim_res, device=device)
    if device_resident:
        assert sig.is_cuda and iq.is_cuda and sig_ws.is_cuda
        sig, iq, sig_ws = (x.cpu().numpy() for x in (sig, iq, sig_ws))
    assert sig.shape == (3, len(COUNTS), N) and iq.shape == (3, len(COUNTS), 2, Na)
    assert np.abs(iq - want_iq).max() < 1e-13 * np.abs(want_iq).max()
    assert np.abs(sig - want).max() < 1e-12 * np.abs(want).max()
    assert np.array_equal(_bits(sig_ws), _bits(sig))


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_synthesis_vjp_on_grid(prop, grid):
    t0, t1, awg_res, sim_res, N, Na = _grid(grid)
    rng = np.random.default_rng(200 + list(GRIDS).index(grid))
    channels_b, carrier = _problem(rng, 2, GRIDS[grid][0][1], _all_combos())
    env, shapes = _pack(channels_b, GAP)
    _check_vjp(channels_b, env, shapes, carrier, grid, rng.normal(size=(2, len(COUNTS), N)))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 257])
def test_synthesis_batch_sizes(prop, B):
    """K = 2 lines of three and one components on the 60 ns grid: at B = 257 mix_kernel's B*K*N thread index spans 12 000
    blocks and mix_bwd_kernel runs 37 000 wavefronts."""
    grid = "60ns_from_3ns"
    t0, t1, awg_res, sim_res, N, Na = _grid(grid)
    rng = np.random.default_rng(300 + B)
    layout = [[("gaussian_nonorm", True, True), ("flattop", False, True), ("trapezoid", True, False)], [("cosine", False, True)]]
    channels_b, carrier = _problem(rng, B, GRIDS[grid][0][1], layout)
    env, shapes = _pack(channels_b)
    want, want_iq = _oracle(channels_b, carrier, t0, t1, awg_res, sim_res)
    sig, iq = (x.cpu().numpy() for x in sg.synthesize_signals(env, shapes, carrier, t0, t1, awg_res, sim_res, want_iq=True, device="cuda:0"))
    assert sig.shape == (B, 2, N) and iq.shape == (B, 2, 2, Na)
    assert np.abs(iq - want_iq).max() < 1e-13 * np.abs(want_iq).max()
    assert np.abs(sig - want).max() < 1e-12 * np.abs(want).max()
    _check_vjp(channels_b, env, shapes, carrier, grid, rng.normal(size=(B, 2, N)))


@pytest.mark.gpu
def test_goal_run_with_grad_long_offset_window(prop):
    """optimal_control.goal_run_with_grad, fused and as three calls, on the 60 ns window from t = 3 ns: the goal against the
    oracle pipeline (generate_signal -> propagate_batch -> unitary_infid), the gradient w.r.t. every component's amp,
    xy_angle, freq_offset and delta and both carrier entries of each line against central differences of that pipeline."""
    from c3_amd import optimal_control as oc
    from c3_amd.workloads import make_workload

    w = make_workload(2, B=1, N=8)  # operators only
    t0, t1, awg_res, sim_res, _, _ = _grid("60ns_from_3ns")
    B = 2
    rng = np.random.default_rng(6)
    channels_b = [
        [
            [dict(shape="gaussian_nonorm", amp=rng.uniform(0.04, 0.06), xy_angle=0.2, freq_offset=-53e6 * TWO_PI, delta=-0.6, t_final=40e-9, sigma=10e-9, delay=1.2e-9, use_t_before=True, drag=True),
             dict(shape="cosine", amp=0.02, xy_angle=1.1, freq_offset=31e6 * TWO_PI, delta=0.4, t_final=20e-9, delay=36e-9)],
            [dict(shape="flattop_risefall", amp=0.03, xy_angle=-0.4, freq_offset=10e6 * TWO_PI, delta=0.3, t_final=50e-9, risefall=4e-9, delay=3e-9, drag=True),
             dict(shape="trapezoid", amp=rng.uniform(0.01, 0.02), xy_angle=0.7, freq_offset=-20e6 * TWO_PI, delta=-0.5, t_final=30e-9, risefall=3e-9, delay=20e-9, use_t_before=True)],
        ]
        for _ in range(B)
    ]
    env, shapes = _pack(channels_b)
    carrier = np.tile(np.array([[5.05e9 * TWO_PI, 1e9 * TWO_PI], [5.65e9 * TWO_PI, 1e9 * TWO_PI]]), (B, 1, 1))
    phases = np.tile(w.fr_phase[:1] * (60e-9 / (8 * w.dt)), (B, 1))
    ideal = np.kron(np.array([[1, -1j], [-1j, 1]]) / np.sqrt(2), np.eye(2))
    runs = []
    for fused in (True, False):
        r = oc.goal_run_with_grad(w.h0, w.hks, env, shapes, carrier, t0, t1, awg_res, sim_res, ideal, [0, 1], [3, 3], fr_phase=phases, fused=fused)
        runs.append((fused, r["goal"].cpu().numpy(), r["grad_env"].cpu().numpy(), r["grad_carrier"].cpu().numpy()))
    ts = o.create_ts(t0, t1, sim_res)

    def goal(chans, car, b):
        sigs = np.stack([o.generate_signal(_oracle_line(comps), car[k, 0], car[k, 1], t0, t1, awg_res, sim_res)["values"] for k, comps in enumerate(chans)])
        U = o.propagate_batch(w.h0, w.hks, sigs[None], ts[1] - ts[0], fr_phase=phases[b : b + 1])[0]
        return o.unitary_infid(ideal, U, index=[0, 1], dims=[3, 3])

    def moved(chans, k, e, key, h):
        out = [[dict(c) for c in line] for line in chans]
        out[k][e][key] += h
        return out

    for b in range(B):
        chans = channels_b[b]
        g0 = goal(chans, carrier[b], b)
        for fused, gl, _, _ in runs:
            assert abs(gl[b] - g0) < 1e-11, (fused, b)
        for k, line in enumerate(chans):
            for e, c in enumerate(line):
                for key, h in (("amp", 1e-6), ("xy_angle", 1e-6), ("freq_offset", 1e3), ("delta", 1e-5)):
                    slot = sg.ENV_SLOTS[key]
                    if key == "delta" and not c.get("drag", False):
                        assert all(ge[b, k, e, slot] == 0.0 for _, _, ge, _ in runs)
                        continue
                    fd = (goal(moved(chans, k, e, key, h), carrier[b], b) - goal(moved(chans, k, e, key, -h), carrier[b], b)) / (2 * h)
                    for fused, _, ge, _ in runs:
                        assert abs(fd - ge[b, k, e, slot]) < 2e-6 * abs(fd) + 1e-16, (fused, b, k, e, key, fd, ge[b, k, e, slot])
            for i, h in ((0, 1e2), (1, 1e-6 * carrier[b, k, 1])):
                cp, cm = carrier[b].copy(), carrier[b].copy()
                cp[k, i] += h
                cm[k, i] -= h
                fd = (goal(chans, cp, b) - goal(chans, cm, b)) / (2 * h)
                for fused, _, _, gc in runs:
                    assert abs(fd - gc[b, k, i]) < 2e-6 * abs(fd) + 1e-16, (fused, b, k, i, fd, gc[b, k, i])
