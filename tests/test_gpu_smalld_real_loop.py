"""The real core + border slice loop of the small-D chain kernel (D = 5, 9; workgroup per sample): per-segment weights, the
trace shift formed once per segment, compile-time and run-time loops over the control tables -- against the CPU oracle at the
tolerance of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from oracle import c3_oracle as o

pytestmark = pytest.mark.gpu

TOL = 1e-10  # tests/test_gpu_parity.py: |U_gpu - U_ref|_F < 1e-10 per sample
S = 32  # eight waves of four chains: the workgroup-per-sample kernel
N = 131
B = 3
MM6_THETA, MM8_THETA = 0.81, 1.85  # radii of the degree-6 and degree-8 pairs (c3p_common.h)
MW_SPLIT = "c3p_smalld.hip: smalld_chain_kernel<%d, false, false, false, true, true>"


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


def segments(n, s=S, per_mille=700):
    """[n0, n1) of the s segments of a sample as launch_chain_t / split_segments deal them: the first s / 2 chains take the long
    segments, the others share the rest."""
    h = s // 2
    la = max(1, (n * per_mille) // (500 * s))
    if h * la > n - h:
        la = (n - h) // h
    rest = n - h * la
    edge = lambda g: g * la if g <= h else h * la + ((g - h) * rest) // h
    return [(edge(g), edge(g + 1)) for g in range(s)]


def segment_bounds(h0, hks, sig, dt):
    """the kernel's bound per segment: ||G0||_1 + sum_k max_t |c_k(t)| ||G_k||_1 of the trace-shifted generators"""
    D = h0.shape[-1]
    one = lambda h: np.abs(dt * (h - np.trace(h) / D * np.eye(D))).sum(axis=0).max()
    out = []
    for b in range(sig.shape[0]):
        for n0, n1 in segments(sig.shape[2]):
            out.append(one(h0) + sum(np.abs(sig[b, k, n0:n1]).max() * one(hks[k]) for k in range(sig.shape[1])))
    return np.array(out)


def sym(rng, D, s):
    m = rng.normal(size=(D, D))
    return (s * (m + m.T) / 2).astype(np.complex128)


def problem(rng, D, K, target, trace=0.0, mean=0.0):
    """real symmetric operators, amplitudes of nearly constant magnitude (so that every segment's bound is close to the sample's),
    dt such that the largest segment bound is `target`"""
    h0 = np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.05) + trace * np.eye(D)
    hks = np.stack([sym(rng, D, 0.4) + 0.5 * trace * np.eye(D) for _ in range(K)]) if K else np.zeros((0, D, D), complex)
    sig = rng.choice([-1.0, 1.0], size=(B, K, N)) * rng.uniform(0.9, 1.0, size=(B, K, N)) + mean
    dt = target / segment_bounds(h0, hks, sig, 1.0).max()
    return h0, hks, sig, dt


def run(prop, D, h0, hks, sig, dt, ph=None):
    from c3_amd import _lib

    with _lib.options(smalld_segments=S):
        U = np.asarray(prop.propagate_batch(h0, hks, sig, dt, fr_phase=ph)["U"])
    assert _lib.last_kernel_detail() == MW_SPLIT % D, _lib.last_kernel_detail()
    ref = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    err = max(np.linalg.norm(U[b] - ref[b]) for b in range(U.shape[0]))
    print(f"D={D} K={sig.shape[1]} max_b |U - U_ref|_F = {err:.3e}")
    return err


def test_segments_of_a_wave_are_unequal():
    """N = 131: the long segments take 5 slices, the short ones 3 or 4 -- a wave of short chains iterates 4 times and at least one of
    its chains runs a masked last slot (weight a_0 = 0)"""
    seg = segments(N)
    assert seg[0][0] == 0 and seg[-1][1] == N and all(a[1] == b[0] for a, b in zip(seg, seg[1:]))
    lens = [n1 - n0 for n0, n1 in seg]
    assert N >= 4 * S and min(lens) >= 1
    waves = [lens[4 * w : 4 * w + 4] for w in range(S // 4)]
    assert any(min(w) < max(w) for w in waves), waves


@pytest.mark.parametrize("D", [5, 9])
@pytest.mark.parametrize("K", [0, 1, 2, 3])
def test_table_loops_compile_time_and_run_time(prop, D, K):
    """K = 0, 1, 2: the loop over the tables unrolled at compile time; K = 3: the run-time loop"""
    rng = np.random.default_rng(7100 + 10 * D + K)
    h0, hks, sig, dt = problem(rng, D, K, 0.7)
    assert segment_bounds(h0, hks, sig, dt).max() <= MM6_THETA
    assert run(prop, D, h0, hks, sig, dt) < TOL


@pytest.mark.parametrize("D", [5, 9])
@pytest.mark.parametrize("with_phase", [False, True])
def test_trace_shift_once_per_segment(prop, D, with_phase):
    """h0 and the controls with non-zero trace, amplitudes with non-zero mean: the summed phase of a sample winds more than twenty
    times, a long segment's own phase leaves (-pi, pi] (the reduction inside the segment sum acts).  The trace is as large as the
    oracle allows: its expm (Pade 13, squarings rounded DOWN as the reference does) is accurate to 1e-14 only while
    ||dt H||_1 stays below theta_13 = 5.37 -- at four times this trace it is itself 1.3e-9 away from scipy's expm."""
    rng = np.random.default_rng(7200 + D)
    K = 2
    h0, hks, sig, dt = problem(rng, D, K, 0.7, trace=10.0, mean=0.3)
    H = h0[None, None] + np.einsum("bkn,kij->bnij", sig, hks)
    assert np.abs(dt * H).sum(axis=-2).max() < o.PADE_THETA[4]
    total = dt * (N * np.trace(h0).real / D + sum(sig[:, k, :].sum(axis=1) * np.trace(hks[k]).real / D for k in range(K)))
    assert np.abs(total).min() > 20 * 2 * np.pi, total
    n0, n1 = segments(N)[0]
    assert abs(dt * (n1 - n0) * np.trace(h0).real / D) > np.pi
    ph = rng.uniform(0, 6.28, size=(B, D)) if with_phase else None
    assert run(prop, D, h0, hks, sig, dt, ph) < TOL


@pytest.mark.parametrize("D", [5, 9])
def test_degree8_pair(prop, D):
    rng = np.random.default_rng(7300 + D)
    h0, hks, sig, dt = problem(rng, D, 2, 1.6)
    bd = segment_bounds(h0, hks, sig, dt)
    assert bd.min() > MM6_THETA and bd.max() <= MM8_THETA, (bd.min(), bd.max())
    assert run(prop, D, h0, hks, sig, dt) < TOL


@pytest.mark.parametrize("D", [5, 9])
def test_squarings_scale_the_weights(prop, D):
    """bound above 1.85: squarings, weights with rscale < 1 (one and two halvings)"""
    rng = np.random.default_rng(7400 + D)
    for target in (3.2, 6.5):
        h0, hks, sig, dt = problem(rng, D, 2, target, trace=0.5)
        assert segment_bounds(h0, hks, sig, dt).min() > MM8_THETA
        assert run(prop, D, h0, hks, sig, dt) < TOL


@pytest.mark.parametrize("D", [5, 9])
def test_complex_sample_in_the_same_launch(prop, D):
    """per-sample operators, one sample with a complex Hermitian control: it takes the complex loop of the same launch behind the
    shared prologue; its neighbours take the real loop"""
    rng = np.random.default_rng(7500 + D)
    h0, hks, sig, dt = problem(rng, D, 2, 0.7, trace=1.5, mean=0.2)
    h0b = np.stack([h0] * B)
    hksb = np.stack([hks] * B)
    a = rng.normal(size=(D, D))
    hksb[1, 0] = hksb[1, 0] + 0.2j * (a - a.T)
    ph = rng.uniform(0, 6.28, size=(B, D))
    from c3_amd import _lib

    with _lib.options(smalld_segments=S):
        U = np.asarray(prop.propagate_batch(h0b, hksb, sig, dt, fr_phase=ph)["U"])
    assert (MW_SPLIT % D) in _lib.last_kernel_detail(), _lib.last_kernel_detail()
    ref = np.stack([o.propagate_batch(h0b[b], hksb[b], sig[b : b + 1], dt, fr_phase=ph[b : b + 1])[0] for b in range(B)])
    err = [np.linalg.norm(U[b] - ref[b]) for b in range(B)]
    print("per-sample errors", err)
    assert max(err) < TOL
