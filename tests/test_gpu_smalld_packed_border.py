"""The chain step of the core + border real loop (c3p_smalld.hip, chain_step8: D = 5, 9) with the column border and the corner of the
state carried packed -- Re and Im dealt over the quad index of the lane, the rotation by DPP -- against the CPU oracle at the bar of
tests/test_gpu_smalld_chain_border.py: max |U - U_ref| < 1e-11.  tests/chain_packed_model.py holds the same step on a lane-level CPU
model, and tests/test_chain_packed_model.py asserts on these inputs that a wrong rotation, a dropped corner term or Re and Im swapped
at the store move the result by more than 1e-6.

Cases (dense random real-symmetric operators, B = 3, random row phases; inputs as in tests/test_gpu_smalld_chain_border.py):
* one-wave workgroups, 4 segments, K = 2, D in {5, 9}: N = 5 -- segments of 1, 1, 1, 2: the peeled slice alone and a single step;
  N = 23; N = 203 -- 50 dependent steps;
* D = 5, K = 3, N = 23: the run-time-K loop;
* D = 9, 32 segments, N = 131: the workgroup-per-sample instance at its default split, uneven segments and padded slots;
* D = 9, 6 segments, N = 23: 18 chains in five one-wave workgroups, the last wave with two invalid chains;
* D = 9, N = 40, 4 segments with the largest segment bound at 0.6 (degree-6 pair), 1.5 (degree-8 pair) and 3.0 (one squaring): each
  copy of the loop has its own register allocation.
For every case: the oracle at 1e-11; the default against the padded tiles (no_split81 = 1) at 1e-11; equal segments (mw_skew = 500)
against one-wave workgroups (no_mw = 1) array_equal; two identical calls array_equal.

Every case's reference has the real and imaginary parts of its whole border column above 1e-2 in magnitude (seeds searched on the
CPU; asserted by tests/test_chain_packed_model.py together with the guard above).  The oracle's results are computed once per case."""
import functools

import numpy as np
import pytest

from norm_bound_model import MM6_THETA, MM8_THETA, bounds, segments
from oracle import c3_oracle as o
from test_gpu_smalld_chain_border import B, KERNEL, TOL, problem

# name -> D, K, N, S (segments per sample), target (largest column-wise segment bound)
CASES = {}
for _D in (9, 5):
    for _N in (5, 23, 203):
        CASES[f"d{_D}_k2_s4_n{_N}"] = dict(D=_D, K=2, N=_N, S=4, target=0.7)
CASES["d5_k3_s4_n23"] = dict(D=5, K=3, N=23, S=4, target=0.7)
CASES["d9_k2_s32_n131"] = dict(D=9, K=2, N=131, S=32, target=0.7)
CASES["d9_k2_s6_n23"] = dict(D=9, K=2, N=23, S=6, target=0.7)
for _t in (0.6, 1.5, 3.0):
    CASES[f"d9_k2_s4_n40_norm{_t}"] = dict(D=9, K=2, N=40, S=4, target=_t)
# seeds for which the reference's border column is well away from zero in both parts
SEEDS = {
    "d9_k2_s4_n5": 45804, "d9_k2_s4_n23": 42023, "d9_k2_s4_n203": 43043, "d5_k2_s4_n5": 44080, "d5_k2_s4_n23": 45009,
    "d5_k2_s4_n203": 46000, "d5_k3_s4_n23": 47005, "d9_k2_s32_n131": 48009, "d9_k2_s6_n23": 49146,
    "d9_k2_s4_n40_norm0.6": 50031, "d9_k2_s4_n40_norm1.5": 51008, "d9_k2_s4_n40_norm3.0": 52006,
}


def seg_edges(c):
    """the segments the launch cuts: 32 segments -- the default split of the workgroup-per-sample mode (736 per mille at D = 9, 716 at
    D = 5); 4 and 6 segments -- equal shares"""
    return segments(c["N"], c["S"], (736 if c["D"] == 9 else 716) if c["S"] == 32 else 500)


@functools.lru_cache(maxsize=None)
def case(name):
    kw = CASES[name]
    h0, hks, sig, dt, ph, _ = problem(np.random.default_rng(SEEDS[name]), kw["D"], kw["K"], kw["N"], kw["S"], kw["target"])
    # (problem() scales dt on the cut of its own file; the bounds of the segments this launch cuts:)
    col = np.array([[bounds(h0, hks, sig[b], dt, n0, n1)[1] for n0, n1 in seg_edges(kw)] for b in range(B)])
    ref = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    for a in (h0, hks, sig, ph, col, ref):
        a.setflags(write=False)
    return dict(kw, name=name, h0=h0, hks=hks, sig=sig, dt=dt, ph=ph, col=col, ref=ref)


@pytest.mark.parametrize("name", list(CASES))
def test_cases_are_what_they_are_named_for(name):
    c = case(name)
    lens = [n1 - n0 for n0, n1 in seg_edges(c)]
    assert sum(lens) == c["N"] and len(lens) == c["S"]
    if c["N"] == 5:
        assert lens == [1, 1, 1, 2]
    if c["N"] == 203:
        assert min(lens) == 50  # 50 dependent steps behind the peeled slice, or 49
    if c["S"] == 32:
        assert min(lens) < max(lens) and any(min(lens[4 * w : 4 * w + 4]) < max(lens[4 * w : 4 * w + 4]) for w in range(8))
    if c["S"] == 6:
        assert (B * c["S"]) % 4 == 2
    # the pair of polynomials the target asks for, on every segment
    if c["target"] <= MM6_THETA:
        assert c["col"].max() <= MM6_THETA
    elif c["target"] <= MM8_THETA:
        assert c["col"].min() > MM6_THETA and c["col"].max() <= MM8_THETA
    else:
        assert c["col"].min() > MM8_THETA and c["col"].max() <= 2 * MM8_THETA


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
        # (6 segments: the chains' launch first, then the launch that folds the six segment products)
        log = _lib.last_kernel_detail().split("; ")
        assert log[0] == KERNEL % (c["D"], kernel) and len(log) == (2 if c["S"] == 6 else 1), log
    return U


def run_default(prop, c):
    """the case's own mode: 32 segments -- workgroup per sample at the default split; otherwise one-wave workgroups"""
    return run(prop, c, "true") if c["S"] == 32 else run(prop, c, "false", no_mw=1)


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
    """equal segments: the workgroup-per-sample instance and the one-wave instance share the step and give the same bits"""
    c = case(name)
    Ue, U1 = run(prop, c, "true" if c["S"] == 32 else "false", mw_skew=500), run(prop, c, "false", no_mw=1)
    assert np.array_equal(Ue, U1)
    assert np.abs(Ue - c["ref"]).max() < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_repeatable(prop, name):
    c = case(name)
    assert np.array_equal(run_default(prop, c), run_default(prop, c))
