"""The forms of the core + border real slice loop (c3p_smalld.hip, D = 5, 9) against the CPU oracle at the bar of
tests/test_gpu_smalld_chain_border.py: max |U - U_ref| < 1e-11.  A segment's first slice is peeled out of the loop (it alone copies E
into the state); a segment without squarings then runs the slots that are real for all four chains of its wave in a body without a
drift weight and without squarings (compile-time K = 0, 1, 2), and a padded last slot in the weighted body; a segment with squarings,
or with K > 2, runs the weighted body throughout.

Cases (dense random real-symmetric operators, B = 3, random row phases; inputs as in tests/test_gpu_smalld_chain_border.py):
* D in {5, 9} x K in {0, 1, 2, 3}, 32 segments (workgroup per sample): N = 32 -- every chain is one slice, the peeled slice alone;
  N = 33 -- chains of one and two slices in one wave, so a padded slot right after the peeled one; N = 47 -- the same in every
  wave; N = 131 -- the uneven split, segments of 3 .. 5 slices;
* D in {5, 9}, K = 2, 4 segments, one-wave workgroups: N = 4, 5, 7, 23;
* D = 9, K = 2, N = 131 with the largest segment bound at 0.6 (degree 6, no squaring), 1.5 (degree 8, no squaring) and 3.0 (one
  squaring: the weighted body);
* one batch whose three samples have amplitudes scaled onto those three forms, in one launch.
For every case: the default against the padded tiles (no_split81 = 1) at 1e-11; equal segments (mw_skew = 500) against one-wave
workgroups array_equal; two identical calls array_equal; the launch log names the instance.

test_cases_are_what_they_are_named_for checks on the CPU, from tests/norm_bound_model.py, that every case's segments have the chain
lengths and every wave the squaring count and polynomial degree that the case is named for.  The oracle's results are computed once
per case and shared."""
import functools

import numpy as np
import pytest

from norm_bound_model import MM6_THETA, MM8_THETA, bounds, segments
from oracle import c3_oracle as o
from test_gpu_smalld_chain_border import B, KERNEL, TOL, sym

# name -> D, K, N, S (segments per sample), target: largest column-wise segment bound of each sample
CASES = {}
for _D in (5, 9):
    for _K in (0, 1, 2, 3):
        for _N in (32, 33, 47, 131):
            CASES[f"d{_D}_k{_K}_s32_n{_N}"] = dict(D=_D, K=_K, N=_N, S=32, target=(0.7,) * B)
    for _N in (4, 5, 7, 23):
        CASES[f"d{_D}_k2_s4_n{_N}"] = dict(D=_D, K=2, N=_N, S=4, target=(0.7,) * B)
for _t in (0.6, 1.5, 3.0):
    CASES[f"d9_k2_s32_n131_norm{_t}"] = dict(D=9, K=2, N=131, S=32, target=(_t,) * B)
CASES["d9_k2_s32_n131_mixed"] = dict(D=9, K=2, N=131, S=32, target=(0.6, 1.5, 3.0))
# what the chains of a case look like: (shortest, longest) segment, and whether some wave holds chains of unequal length
LENGTHS = {32: (1, 1, False), 33: (1, 2, True), 47: (1, 2, True), 131: (3, 5, True), 4: (1, 1, False), 5: (1, 2, True), 7: (1, 2, True),
           23: (5, 6, True)}


def seg_edges(c):
    """the segments the launch cuts: 32 segments of at least four slices on average -- the default split of the workgroup-per-sample
    mode (704 per mille at D = 9, 700 at D = 5); shorter samples, 4 segments and mw_skew = 500 -- equal shares"""
    uneven = c["S"] == 32 and c["N"] >= 4 * c["S"]
    return segments(c["N"], c["S"], (704 if c["D"] == 9 else 700) if uneven else 500)


def seg_bounds(h0, hks, sig, dt, seg):
    return np.array([[bounds(h0, hks, sig[b], dt, n0, n1)[1] for n0, n1 in seg] for b in range(B)])


def problem(rng, D, K, N, S, target):
    """as problem() of tests/test_gpu_smalld_chain_border.py (dense real-symmetric drift and controls, amplitudes of nearly constant
    magnitude), with one target per sample: dt puts the largest column-wise segment bound of the samples with the smallest target on
    it, and the amplitudes of the others are scaled up (bisection; the bound grows with the scale) until theirs are on their own"""
    h0 = np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.3)
    hks = np.stack([sym(rng, D, 0.4) for _ in range(K)]) if K else np.zeros((0, D, D), complex)
    sig = rng.choice([-1.0, 1.0], size=(B, K, N)) * rng.uniform(0.9, 1.0, size=(B, K, N))
    ph = rng.uniform(0, 6.28, size=(B, D))
    seg = seg_edges(dict(D=D, N=N, S=S))
    low = [b for b in range(B) if target[b] == min(target)]
    dt = min(target) / seg_bounds(h0, hks, sig, 1.0, seg)[low].max()
    for b in range(B):
        if b in low:
            continue
        top = lambda f: max(bounds(h0, hks, f * sig[b], dt, n0, n1)[1] for n0, n1 in seg)
        lo, hi = 1.0, 64.0
        assert top(lo) < target[b] < top(hi)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if top(mid) < target[b] else (lo, mid)
        sig[b] *= lo
    return h0, hks, sig, dt, ph, seg_bounds(h0, hks, sig, dt, seg)


@functools.lru_cache(maxsize=None)
def case(name):
    kw = CASES[name]
    seed = 31000 + 17 * list(CASES).index(name)
    h0, hks, sig, dt, ph, col = problem(np.random.default_rng(seed), kw["D"], kw["K"], kw["N"], kw["S"], kw["target"])
    ref = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    for a in (h0, hks, sig, ph, col, ref):
        a.setflags(write=False)
    return dict(kw, name=name, h0=h0, hks=hks, sig=sig, dt=dt, ph=ph, col=col, ref=ref)


def form(bound):
    """(squarings, degree) the loop takes at a wave's bound: c3p_squarings against the radius of the degree-8 pair, then the degree-6
    pair where the scaled bound is inside its radius"""
    s = 0
    while MM8_THETA * 2**s < bound:
        s += 1
    return s, (6 if bound * 2.0**-s <= MM6_THETA else 8)


@pytest.mark.parametrize("name", list(CASES))
def test_cases_are_what_they_are_named_for(name):
    c = case(name)
    seg = seg_edges(c)
    lens = np.array([n1 - n0 for n0, n1 in seg])
    lo, hi, padded = LENGTHS[c["N"]]
    assert lens.sum() == c["N"] and lens.min() == lo and lens.max() == hi
    waves = lens.reshape(-1, 4)
    assert (waves.max(axis=1) - waves.min(axis=1)).max() == (1 if padded else 0)  # at most the last slot of a wave is padding
    if c["N"] == 47:
        assert (waves.max(axis=1) - waves.min(axis=1)).min() == 1  # a padded slot in every wave
    if c["N"] in (33, 5):
        assert sorted(lens)[-2:] == [1, 2]  # one chain of two slices: its wave runs the peeled slice and one padded slot
    # the plan of every wave (the kernel takes the largest bound of a wave's four chains), per sample
    wave_col = c["col"].reshape(B, -1, 4).max(axis=2)
    for b, t in enumerate(c["target"]):
        want = {0.6: (0, 6), 0.7: (0, 6), 1.5: (0, 8), 3.0: (1, 8)}[t]
        assert {form(x) for x in wave_col[b]} == {want}, (b, sorted(wave_col[b]))
        assert wave_col[b].max() <= t * (1 + 1e-12)
    assert abs(max(wave_col[b].max() / t for b, t in enumerate(c["target"])) - 1) < 1e-12
    print(f"{name}: segments {lo}..{hi}, wave bounds {wave_col.min(axis=1).round(3)} .. {wave_col.max(axis=1).round(3)}")


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
    return run(prop, c, "true" if c["S"] == 32 else "false")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_parity_against_the_oracle(prop, name):
    c = case(name)
    U = run_default(prop, c)
    err = np.abs(U - c["ref"]).max()
    print(f"{name}: max |U - U_oracle| {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_padded_tiles_agree(prop, name):
    c = case(name)
    from c3_amd import _lib

    U, Up = run_default(prop, c), run(prop, c, no_split81=1)
    padded = _lib.last_kernel_detail()
    assert "smalld_chain_kernel<%d, " % c["D"] in padded and padded not in (KERNEL % (c["D"], "true"), KERNEL % (c["D"], "false")), padded
    err = np.abs(U - Up).max()
    print(f"{name}: max |U - U_padded| {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_modes_bit_for_bit(prop, name):
    """equal segments: the workgroup-per-sample instance and the one-wave instance run the same forms and give the same bits"""
    c = case(name)
    Ue, U1 = run(prop, c, "true" if c["S"] == 32 else "false", mw_skew=500), run(prop, c, "false", no_mw=1)
    assert np.array_equal(Ue, U1)
    assert np.abs(Ue - c["ref"]).max() < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_repeatable(prop, name):
    c = case(name)
    assert np.array_equal(run_default(prop, c), run_default(prop, c))
