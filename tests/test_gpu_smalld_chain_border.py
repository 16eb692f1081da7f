"""The chain step of the core + border real loop (c3p_smalld.hip, chain_step8: D = 5, 9) with its border in the direct form -- row
border, column border and corner as fma chains on the vector unit, each reduced over the lane's r index by one matrix instruction
against a tile of ones (the row border with the ones as the A operand) -- against the CPU oracle at the bar of
tests/test_gpu_round2.py and tests/test_gpu_smalld_fold_split.py: max |U - U_ref| < 1e-11.  tests/test_chain_border_model.py holds the
same step on a lane-level CPU model.

Cases (dense random real-symmetric operators, B = 3, random row phases):
* D in {5, 9} x K in {0, 2, 3}, 32 segments, N = 131: the workgroup-per-sample instance with uneven segments of 3 .. 5 slices -- a wave
  of short chains runs a masked slot, where the step is applied with E = I and must pass the border through;
* D in {5, 9}, K = 2, 4 segments, one-wave workgroups: N = 23 and N = 203 (50 dependent steps per chain);
* D = 9, K = 2 with the largest segment bound at 0.6 (degree-6 pair), 1.5 (degree-8 pair) and 3.0 (one squaring);
* the padded-tile form (no_split81 = 1) against the default: 1e-11;  equal segments (mw_skew = 500) against one-wave workgroups:
  array_equal;  two identical calls: array_equal.

Before every GPU call border_guard asserts on the CPU, from the oracle's per-slice propagators, why a wrong border cannot pass:
every element of the reference's last row and last column (the corner among them) has real and imaginary parts above 1e-2 in
magnitude, and replacing the last row, or the last column, of ANY single slice propagator by the identity's moves the reference by
more than 1e-6.  The seeds below were chosen so that this holds.  The oracle's results are computed once per case and shared."""
import functools

import numpy as np
import pytest

from norm_bound_model import MM6_THETA, MM8_THETA, bounds, segments
from oracle import c3_oracle as o

TOL = 1e-11
B = 3
KERNEL = "c3p_smalld.hip: smalld_chain_kernel<%d, false, false, false, %s, true>"  # workgroup per sample: true; one wave: false

# name -> D, K, N, S (segments per sample), target (largest column-wise segment bound), seed
CASES = {}
for _D in (5, 9):
    for _K in (0, 2, 3):
        CASES[f"d{_D}_k{_K}_s32_n131"] = dict(D=_D, K=_K, N=131, S=32, target=0.7)
    for _N in (23, 203):
        CASES[f"d{_D}_k2_s4_n{_N}"] = dict(D=_D, K=2, N=_N, S=4, target=0.7)
for _t in (0.6, 1.5, 3.0):
    CASES[f"d9_k2_s32_n131_norm{_t}"] = dict(D=9, K=2, N=131, S=32, target=_t)
# seeds for which border_guard holds (searched on the CPU; the margins are printed by test_inputs_tell_a_wrong_border)
SEEDS = {
    "d5_k0_s32_n131": 8101, "d5_k2_s32_n131": 9102, "d5_k3_s32_n131": 10103, "d5_k2_s4_n23": 11104, "d5_k2_s4_n203": 12100,
    "d9_k0_s32_n131": 13102, "d9_k2_s32_n131": 14160, "d9_k3_s32_n131": 15193, "d9_k2_s4_n23": 16128, "d9_k2_s4_n203": 17152,
    "d9_k2_s32_n131_norm0.6": 18183, "d9_k2_s32_n131_norm1.5": 19166, "d9_k2_s32_n131_norm3.0": 20164,
}


def sym(rng, D, s):
    m = rng.normal(size=(D, D))
    return (s * (m + m.T) / 2).astype(np.complex128)


def seg_edges(c):
    """the segments the launch cuts: 32 segments -- the default split of the workgroup-per-sample mode (704 per mille at D = 9, 700 at
    D = 5); 4 segments -- equal shares"""
    return segments(c["N"], c["S"], (704 if c["D"] == 9 else 700) if c["S"] == 32 else 500)


def problem(rng, D, K, N, S, target):
    """as problem() of tests/test_gpu_smalld_real_loop.py, with a dense drift: real symmetric operators, amplitudes of nearly constant
    magnitude (every segment's bound is close to the sample's), dt such that the largest column-wise segment bound is `target`"""
    h0 = np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.3)
    hks = np.stack([sym(rng, D, 0.4) for _ in range(K)]) if K else np.zeros((0, D, D), complex)
    sig = rng.choice([-1.0, 1.0], size=(B, K, N)) * rng.uniform(0.9, 1.0, size=(B, K, N))
    ph = rng.uniform(0, 6.28, size=(B, D))
    seg = seg_edges(dict(D=D, N=N, S=S))
    col = np.array([[bounds(h0, hks, sig[b], 1.0, n0, n1)[1] for n0, n1 in seg] for b in range(B)])
    dt = target / col.max()
    return h0, hks, sig, dt, ph, col * dt


def build_case(name, seed):
    kw = CASES[name]
    D, K, N = kw["D"], kw["K"], kw["N"]
    h0, hks, sig, dt, ph, col = problem(np.random.default_rng(seed), D, K, N, kw["S"], kw["target"])
    dU = np.stack([o.tf_propagation_vectorized(h0, hks, sig[b], dt) if K else np.stack([o.expm(-1j * dt * h0)] * N) for b in range(B)])
    ref = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    return dict(kw, name=name, h0=h0, hks=hks, sig=sig, dt=dt, ph=ph, col=col, dU=dU, ref=ref)


def border_margins(c):
    """(smallest |Re|, |Im| over the reference's last rows and columns, smallest move of the reference when the last row / the last
    column of one slice propagator is replaced by the identity's, largest distance of the folded slice propagators from the reference)"""
    D, N = c["D"], c["N"]
    small, moved, off = [], [], []
    for b in range(B):
        ref = c["ref"][b]
        edge = np.concatenate([ref[D - 1, :], ref[:, D - 1]])
        small.append(min(np.abs(edge.real).min(), np.abs(edge.imag).min()))
        dU = c["dU"][b]
        pre, suf = [np.eye(D, dtype=complex)], [np.eye(D, dtype=complex)]  # pre[n] = dU[n-1] .. dU[0], suf[n] = dU[N-1] .. dU[N-n]
        for n in range(N):
            pre.append(dU[n] @ pre[-1])
            suf.append(suf[-1] @ dU[N - 1 - n])
        U = pre[N]
        off.append(np.abs(np.exp(1j * c["ph"][b])[:, None] * U - ref).max())
        for n in range(N):
            for what in ("row", "column"):
                m = dU[n].copy()
                if what == "row":
                    m[D - 1, :] = np.eye(D)[D - 1]
                else:
                    m[:, D - 1] = np.eye(D)[D - 1]
                moved.append(np.abs(suf[N - 1 - n] @ m @ pre[n] - U).max())
    return min(small), min(moved), max(off)


@functools.lru_cache(maxsize=None)
def border_guard(name):
    """the case, after asserting that its inputs tell a wrong border (see the module docstring)"""
    c = build_case(name, SEEDS[name])
    small, moved, off = border_margins(c)
    print(f"{name}: smallest border part {small:.3e}, smallest move {moved:.3e}, fold against the oracle {off:.1e}")
    assert off < 1e-12, off
    assert small > 1e-2, small
    assert moved > 1e-6, moved
    # the pair of polynomials the target asks for, on every wave
    if c["target"] <= MM6_THETA:
        assert c["col"].max() <= MM6_THETA
    elif c["target"] <= MM8_THETA:
        assert c["col"].min() > MM6_THETA and c["col"].max() <= MM8_THETA
    else:
        assert c["col"].min() > MM8_THETA and c["col"].max() <= 2 * MM8_THETA
    return c


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_tell_a_wrong_border(name):
    border_guard(name)


def test_segments_leave_a_masked_slot():
    """N = 131 in 32 segments: a wave of short chains holds segments of unequal length, so one of its chains runs a masked last slot"""
    for D in (5, 9):
        lens = [n1 - n0 for n0, n1 in seg_edges(dict(D=D, N=131, S=32))]
        assert sum(lens) == 131 and min(lens) >= 3 and max(lens) <= 5
        assert any(min(lens[4 * w : 4 * w + 4]) < max(lens[4 * w : 4 * w + 4]) for w in range(8))


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


def run(prop, c, kernel=None, **opts):
    from c3_amd import _lib

    with _lib.options(smalld_segments=c["S"], **opts):
        U = np.asarray(prop.propagate_batch(c["h0"], c["hks"], c["sig"], c["dt"], fr_phase=c["ph"])["U"])
    if kernel is not None:
        assert _lib.last_kernel_detail() == KERNEL % (c["D"], kernel), _lib.last_kernel_detail()
    return U


def run_default(prop, c):
    """the case's own mode: 32 segments -- workgroup per sample; 4 segments -- one-wave workgroups"""
    return run(prop, c, "true") if c["S"] == 32 else run(prop, c, "false", no_mw=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_parity_against_the_oracle(prop, name):
    c = border_guard(name)
    U = run_default(prop, c)
    err = np.abs(U - c["ref"]).max()
    print(f"{name}: max |U - U_oracle| {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["d9_k2_s32_n131", "d5_k2_s32_n131"])
def test_padded_tiles_agree(prop, name):
    c = border_guard(name)
    U, Up = run(prop, c, "true"), run(prop, c, no_split81=1)
    err = np.abs(U - Up).max()
    print(f"{name}: max |U - U_padded| {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["d9_k2_s32_n131", "d5_k2_s32_n131", "d9_k2_s32_n131_norm1.5", "d9_k2_s32_n131_norm3.0"])
def test_modes_bit_for_bit(prop, name):
    """equal segments: the workgroup-per-sample instance and the one-wave instance share the step and give the same bits"""
    c = border_guard(name)
    Ue, U1 = run(prop, c, "true", mw_skew=500), run(prop, c, "false", no_mw=1)
    assert np.array_equal(Ue, U1)
    assert np.abs(Ue - c["ref"]).max() < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["d9_k2_s32_n131", "d5_k3_s32_n131", "d9_k2_s4_n203"])
def test_repeatable(prop, name):
    c = border_guard(name)
    assert np.array_equal(run_default(prop, c), run_default(prop, c))
