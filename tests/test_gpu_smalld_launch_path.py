"""The serial path round the slice loop of smalld_chain_kernel (c3p_smalld.hip): the sample and segment indices and the segment
bounds n0 / n1 taken without a division in the workgroup-per-sample mode, the table build with its reductions on the register
path (one latency chain for the four maxima), the chains' max_t |c_k(t)| taken from the prefetched amplitudes in front of the
table barrier, the table flags read once, no second barrier in that mode, the fold's phase sums on the register path.  Every
GPU result is compared with oracle.c3_oracle at max |U - U_ref| < 1e-10.

* segment bounds: D = 9, 5 with 32 segments, N = 128 (the edge N >= 4 S of the uneven split), 129, 131, 257, 1000, 1600 (long
  segments of 73 slices: beyond the 48 the amplitude prefetch serves); the default split, equal segments (mw_skew = 500) and
  one-wave workgroups (no_mw = 1), the last two array_equal.  The signals differ in every slice: on the oracle, a dropped or a
  doubled slice moves U by more than 1e-6 (asserted first).
* sample index: per-sample drift and control operators that differ by O(1), B = 3.
* maxima: ONE slice carries an amplitude that lifts the segment's bound from below the radius of the degree-6 pair to 1.8; it
  stands in every slot of a long and of a short segment, in each of the four chains of an older and of a younger wave.  The
  control operator couples two levels and dominates the slice, so that the bound is nearly the spectral norm: on the CPU the
  degree-6 pair moves U by more than 1e-8 there.  And the heaviest column of a control operator at each j = 0 .. 8: with that
  column left out of the bound the plan is the degree-6 pair without squarings, which moves U by more than 1e-8 on the CPU.
* flags: a real symmetric drift; one complex Hermitian control; a lossy drift; a real drift asymmetric by 1e-6 of its norm
  (symmetrising it moves U by more than 1e-8 on the CPU: the real path would be wrong) and by 1e-17 (symmetric to rounding:
  either loop is right there, and the test cannot tell which one ran -- last_kernel_detail names the instance, not the loop).
* other instances of the shared prologue: D = 3, D = 12, K = 3.
* CPU: the shifts of the kernel's n0 / n1 against the divisions they replace, every N in 32 .. 2100, S in {8, 16, 32} and every
  long-segment length launch_chain_t derives from 501 .. 899 per mille."""
import functools
import os
import re

import numpy as np
import pytest

from norm_bound_model import MM6_THETA, MM8_THETA, bounds, segments
from oracle import c3_oracle as o

TOL = 1e-10
SKEW = {9: 736, 5: 716}  # default long share of the workgroup-per-sample mode, per mille (launch_chain_t)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sym(rng, D, s):
    m = rng.normal(size=(D, D))
    return (s * (m + m.T) / 2).astype(np.complex128)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def edges(D, N, S=32):
    return segments(N, S, SKEW.get(D, 640) if (S == 32 and N >= 4 * S) else 500)


def top_bound(h0, hks, sig, dt, seg):
    return max(bounds(h0, hks, sig[b], dt, n0, n1)[1] for b in range(sig.shape[0]) for n0, n1 in seg)


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


def gpu(prop, h0, hks, sig, dt, ph, S=32, **opts):
    from c3_amd import _lib

    with _lib.options(smalld_segments=S, **opts):
        U = np.asarray(prop.propagate_batch(h0, hks, sig, dt, fr_phase=ph)["U"])
    assert "smalld_chain_kernel<%d, " % h0.shape[-1] in _lib.last_kernel_detail(), _lib.last_kernel_detail()
    return U


def slice_props(h0, hks, sig1, dt):
    """[N, D, D] slice propagators of one sample"""
    return np.stack([o.expm(-1j * dt * (h0 + np.tensordot(sig1[:, n], hks, axes=1))) for n in range(sig1.shape[1])])


def chain(dU):
    U = np.eye(dU.shape[-1], dtype=complex)
    for E in dU:
        U = E @ U
    return U


# ---------------------------------------------------------------- CPU: the index arithmetic of the workgroup-per-sample mode
def test_shifts_give_the_segment_bounds_of_the_divisions():
    """kernel: sshift = 31 - clz(S); n = (seg N) >> sshift for equal segments; with long segments of La slices the chains seg >= h =
    S / 2 start at h La + ((seg - h) rest) >> (sshift - 1), rest = N - h La.  Before: the same products divided by S and by h."""
    checked = 0
    for S in (8, 16, 32):
        sshift = S.bit_length() - 1  # 31 - clz(S) of a 32-bit S
        assert 1 << sshift == S
        h = S >> 1
        Ns = np.arange(32, 2101, dtype=np.int64)[:, None]
        g = np.arange(S + 1, dtype=np.int64)[None, :]  # n0 of chain g and n1 of chain g - 1
        assert np.array_equal((g * Ns) >> sshift, (g * Ns) // S)
        done = set()
        for pm in range(501, 900):
            La = np.maximum((Ns * pm) // (500 * S), 1)  # launch_chain_t: split()
            La = np.where(h * La > Ns - h, (Ns - h) // h, La)
            key = La.tobytes()
            if key in done:
                continue
            done.add(key)
            rest = Ns - h * La
            assert (rest >= h).all()
            old = np.where(g <= h, g * La, h * La + ((g - h) * rest) // h)
            new = np.where(g <= h, g * La, h * La + (((g - h) * rest) >> (sshift - 1)))
            assert np.array_equal(old, new)
            assert (np.diff(new, axis=1) >= 1).all() and (new[:, -1] == Ns[:, 0]).all() and (new[:, 0] == 0).all()
            checked += new.size
    assert checked > 100000


# ---------------------------------------------------------------- segment bounds
BOUND_N = (128, 129, 131, 257, 1000, 1600)


@functools.lru_cache(maxsize=None)
def bounds_case(D, N):
    rng = np.random.default_rng(7000 + 10 * N + D)
    B, K = 2, 2
    h0 = np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.3)
    hks = np.stack([sym(rng, D, 0.4) for _ in range(K)])
    sig = rng.choice([-1.0, 1.0], size=(B, K, N)) * rng.uniform(0.5, 1.0, size=(B, K, N))  # different in every slice
    ph = rng.uniform(0, 6.28, size=(B, D))
    dt = 0.7 / max(top_bound(h0, hks, sig, 1.0, edges(D, N)), top_bound(h0, hks, sig, 1.0, segments(N, 32, 500)))
    dU = [slice_props(h0, hks, sig[b], dt) for b in range(B)]
    ref = np.stack([np.exp(1j * ph[b])[:, None] * chain(dU[b]) for b in range(B)])
    return frozen(h0, hks, sig, ph, ref) + (dt, dU)


@pytest.mark.parametrize("N", BOUND_N)
@pytest.mark.parametrize("D", (9, 5))
def test_a_dropped_or_doubled_slice_shows(D, N):
    h0, hks, sig, ph, ref, dt, dU = bounds_case(D, N)
    lens = [n1 - n0 for n0, n1 in edges(D, N)]
    assert sum(lens) == N and min(lens) >= 1
    if N >= 129:
        assert max(lens) > min(lens)
    if N == 1600:
        assert max(lens) > 48
    assert np.abs(ref - o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)).max() < 1e-12  # the folded slices ARE the oracle's result
    cut = sorted({n for n0, n1 in edges(D, N) for n in (n0, n1 - 1)})[:: max(1, N // 40)]  # first and last slices of segments
    for n in cut:
        for twice in (False, True):
            d = dU[0][np.r_[0 : n + 1, n:N]] if twice else np.delete(dU[0], n, axis=0)
            moved = np.abs(np.exp(1j * ph[0])[:, None] * chain(d) - ref[0]).max()
            assert moved > 1e-6, (n, twice, moved)


@pytest.mark.gpu
@pytest.mark.parametrize("N", BOUND_N)
@pytest.mark.parametrize("D", (9, 5))
def test_segment_bounds(prop, D, N):
    h0, hks, sig, ph, ref, dt, _ = bounds_case(D, N)
    U = gpu(prop, h0, hks, sig, dt, ph)
    Ue = gpu(prop, h0, hks, sig, dt, ph, mw_skew=500)
    U1 = gpu(prop, h0, hks, sig, dt, ph, no_mw=1)
    errs = [np.abs(x - ref).max() for x in (U, Ue, U1)]
    print(f"D={D} N={N}: max |U - U_oracle| default {errs[0]:.3e} equal segments {errs[1]:.3e} one wave {errs[2]:.3e}")
    assert max(errs) < TOL
    assert np.array_equal(Ue, U1)


# ---------------------------------------------------------------- sample index
@functools.lru_cache(maxsize=None)
def per_sample_case():
    rng = np.random.default_rng(8101)
    B, K, D, N = 3, 2, 9, 131
    h0 = np.stack([np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.3) for _ in range(B)])
    hks = np.stack([np.stack([sym(rng, D, 0.4) for _ in range(K)]) for _ in range(B)])
    sig = rng.choice([-1.0, 1.0], size=(B, K, N)) * rng.uniform(0.5, 1.0, size=(B, K, N))
    ph = rng.uniform(0, 6.28, size=(B, D))
    dt = 0.7 / max(top_bound(h0[b], hks[b], sig[b : b + 1], 1.0, edges(D, N)) for b in range(B))
    ref = np.stack([o.propagate_batch(h0[b], hks[b], sig[b : b + 1], dt, fr_phase=ph[b : b + 1])[0] for b in range(B)])
    # another sample's operators give another result
    for b in range(B):
        c = (b + 1) % B
        assert np.abs(o.propagate_batch(h0[c], hks[c], sig[b : b + 1], dt, fr_phase=ph[b : b + 1])[0] - ref[b]).max() > 1e-2
    return frozen(h0, hks, sig, ph, ref) + (dt,)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ({}, {"no_mw": 1}), ids=("workgroup_per_sample", "one_wave"))
def test_sample_index(prop, opts):
    h0, hks, sig, ph, ref, dt = per_sample_case()
    err = np.abs(gpu(prop, h0, hks, sig, dt, ph, **opts) - ref).max()
    print(f"per-sample operators {opts}: max |U - U_oracle| {err:.3e}")
    assert err < TOL


# ---------------------------------------------------------------- maxima
def header_coefficients(name):
    text = open(os.path.join(ROOT, "c3_amd", "csrc", "c3p_common.h")).read()
    body = re.search(r"\b%s\[\d+\] = \{([^}]*)\}" % name, text).group(1)
    return [float.fromhex(x.strip()) for x in body.split(",")]


def pair_exp(h, dt, deg, squarings=0):
    """exp(-i dt h) of a real symmetric h the way the real loop forms it: the trace shift apart, cos Y - i sin Y from the
    economised pair of degree `deg` in W = Y^2 at Y = dt (h - tr h / D) / 2^s, then s squarings"""
    D = h.shape[0]
    mu = np.trace(h).real / D
    Y = (dt * (h.real - mu * np.eye(D))) / 2.0**squarings
    W = Y @ Y
    cosc, sinc = header_coefficients("c3p_mm%d_cos" % deg), header_coefficients("c3p_mm%d_sinc" % deg)
    C = sum(c * np.linalg.matrix_power(W, p) for p, c in enumerate(cosc))
    Sn = sum(c * np.linalg.matrix_power(W, p) for p, c in enumerate(sinc)) @ Y
    E = C - 1j * Sn
    for _ in range(squarings):
        E = E @ E
    return np.exp(-1j * dt * mu) * E


def form(bound):
    """(squarings, degree) of the real loop at a wave's bound (c3p_squarings against the degree-8 radius, then the degree-6 test)"""
    s = 0
    while MM8_THETA * 2**s < bound:
        s += 1
    return s, (6 if bound * 2.0**-s <= MM6_THETA else 8)


SPIKE_N = 720  # long segments of 33 slices (three amplitude registers a lane), short ones of 12


@functools.lru_cache(maxsize=None)
def spike_base():
    rng = np.random.default_rng(9103)
    D, K, N = 9, 2, SPIKE_N
    # The bound is tight on the heavy slice -- the degree-6 pair's error falls with the 14th power of the true norm --: the first
    # control couples two levels (its 1-norm IS its spectral norm, and the error stays on four elements), everything else is 0.5 %
    h0 = 0.005 * (np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.3))
    pair = np.zeros((D, D), dtype=np.complex128)
    pair[2, 6] = pair[6, 2] = 1.0
    hks = np.stack([pair, 0.005 * sym(rng, D, 0.4)])
    sig = (rng.choice([-1.0, 1.0], size=(1, K, N)) * rng.uniform(0.5, 1.0, size=(1, K, N)))
    ph = rng.uniform(0, 6.28, size=(1, D))
    seg = edges(D, N)
    dt = 0.6 / top_bound(h0, hks, sig, 1.0, seg)
    dU = slice_props(h0, hks, sig[0], dt)
    pre = [np.eye(D, dtype=complex)]
    for E in dU:
        pre.append(E @ pre[-1])
    suf = [np.eye(D, dtype=complex)]
    for E in dU[::-1]:
        suf.append(suf[-1] @ E)
    suf = suf[::-1]  # suf[n] = E_{N-1} ... E_n
    return frozen(h0, hks, sig, ph) + (dt, seg, pre, suf)


def spike_case(n):
    """the base signals with slice n's first amplitude raised until its segment's bound is 1.8; (signals, reference, U with the
    degree-6 pair on that slice)"""
    h0, hks, sig, ph, dt, seg, pre, suf = spike_base()
    n0, n1 = next(s for s in seg if s[0] <= n < s[1])
    s2 = sig.copy()
    lo, hi = 1.0, 200.0
    top = lambda a: bounds(h0, hks, np.concatenate([sig[0, :, :n], [[a], [sig[0, 1, n]]], sig[0, :, n + 1 :]], axis=1), dt, n0, n1)[1]
    assert top(lo) < 1.8 < top(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if top(mid) < 1.8 else (lo, mid)
    s2[0, 0, n] = lo
    h = h0 + lo * hks[0] + sig[0, 1, n] * hks[1]
    rot = np.exp(1j * ph[0])[:, None]
    ref = rot * (suf[n + 1] @ o.expm(-1j * dt * h) @ pre[n])
    weak = rot * (suf[n + 1] @ pair_exp(h, dt, 6) @ pre[n])
    return s2, ref[None], weak[None], (n0, n1)


def spike_slots(wave, chain_):
    n0, n1 = edges(9, SPIKE_N)[4 * wave + chain_]
    return list(range(n0, n1))


def test_spike_cases_are_what_they_are_named_for():
    h0, hks, sig, ph, dt, seg, pre, suf = spike_base()
    lens = [n1 - n0 for n0, n1 in seg]
    assert lens[:16] == [33] * 16 and set(lens[16:]) == {12} and sum(lens) == SPIKE_N
    assert top_bound(h0, hks, sig, dt, seg) <= 0.6 * (1 + 1e-12) < MM6_THETA
    assert np.abs(np.exp(1j * ph[0])[:, None] * pre[-1] - o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)[0]).max() < 1e-12
    for wave, chain_ in ((1, 0), (1, 3), (5, 2)):
        for n in spike_slots(wave, chain_)[::11]:
            s2, ref, weak, (n0, n1) = spike_case(n)
            col = [bounds(h0, hks, s2[0], dt, a, b)[1] for a, b in seg]
            assert form(max(col)) == (0, 8) and abs(max(col) - 1.8) < 1e-9
            assert sum(c > MM6_THETA for c in col) == 1 and col[4 * wave + chain_] == max(col)
            moved = np.abs(weak - ref).max()
            assert moved > 1e-8, (n, moved)


@pytest.mark.gpu
@pytest.mark.parametrize("chain_", range(4))
@pytest.mark.parametrize("wave", (1, 5), ids=("older_wave", "younger_wave"))
def test_one_heavy_slice_in_every_slot(prop, wave, chain_):
    h0, hks, sig, ph, dt, _, _, _ = spike_base()
    worst = 0.0
    for n in spike_slots(wave, chain_):
        s2, ref, weak, _ = spike_case(n)
        assert np.abs(weak - ref).max() > 1e-8
        err = np.abs(gpu(prop, h0, hks, s2, dt, ph) - ref).max()
        assert err < TOL, (n, err)
        worst = max(worst, err)
    print(f"wave {wave} chain {chain_}: {len(spike_slots(wave, chain_))} slots, max |U - U_oracle| {worst:.3e}")


@functools.lru_cache(maxsize=None)
def column_case(j):
    """a control operator with one heavy row and column j: the bound with column j is 5.4 (two squarings), without it the degree-6
    pair without squarings -- at a spectral norm near 2"""
    rng = np.random.default_rng(9300 + j)
    D, K, N, B = 9, 2, 131, 2
    h0 = 0.05 * (np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.3))
    arrow = np.zeros((D, D))
    arrow[j, :] = arrow[:, j] = rng.uniform(0.9, 1.0, D)
    arrow[j, j] = 0.0
    hks = np.stack([arrow.astype(np.complex128), sym(rng, D, 0.01)])
    sig = rng.choice([-1.0, 1.0], size=(B, K, N)) * rng.uniform(0.9, 1.0, size=(B, K, N))
    ph = rng.uniform(0, 6.28, size=(B, D))
    seg = edges(D, N)
    dt = 5.4 / top_bound(h0, hks, sig, 1.0, seg)
    ref = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    return frozen(h0, hks, sig, ph, ref) + (dt, seg)


@pytest.mark.parametrize("j", range(9))
def test_leaving_out_the_heaviest_column_shows(j):
    h0, hks, sig, ph, ref, dt, seg = column_case(j)
    from norm_bound_model import column_sums

    cs = column_sums(h0, hks, dt)
    without = []
    for n0, n1 in seg:
        cmax = np.abs(sig[0][:, n0:n1]).max(axis=1)
        col = cs[0] + cmax @ cs[1:]
        assert np.argmax(col) == j
        without.append(np.delete(col, j).max())
    assert form(max(without)) == (0, 6) and form(5.4) == (2, 8)
    weak = np.exp(1j * ph[0])[:, None] * chain(np.stack([pair_exp(h0 + np.tensordot(sig[0][:, n], hks, axes=1), dt, 6) for n in range(sig.shape[2])]))
    moved = np.abs(weak - ref[0]).max()
    print(f"column {j}: the plan without it moves U by {moved:.3e}")
    assert moved > 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(9))
def test_heaviest_column_in_every_lane(prop, j):
    h0, hks, sig, ph, ref, dt, _ = column_case(j)
    err = np.abs(gpu(prop, h0, hks, sig, dt, ph) - ref).max()
    print(f"column {j}: max |U - U_oracle| {err:.3e}")
    assert err < TOL


# ---------------------------------------------------------------- flags
FLAG_CASES = ("real_symmetric", "complex_control", "lossy_drift", "asym_1e-6", "asym_1e-17")


@functools.lru_cache(maxsize=None)
def flag_case(name):
    rng = np.random.default_rng(9500)
    D, K, N, B = 9, 2, 131, 2
    h0 = np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.3)
    hks = np.stack([sym(rng, D, 0.4) for _ in range(K)])
    sig = rng.choice([-1.0, 1.0], size=(B, K, N)) * rng.uniform(0.5, 1.0, size=(B, K, N))
    ph = rng.uniform(0, 6.28, size=(B, D))
    if name == "complex_control":
        a = rng.normal(size=(D, D))
        hks[1] = hks[1] + 0.2j * (a - a.T)  # Hermitian
        assert np.array_equal(hks[1], hks[1].conj().T) and np.abs(hks[1].imag).max() > 0.1
    elif name == "lossy_drift":
        h0 = h0 - 0.05j * np.diag(rng.uniform(0, 1, D))
    elif name.startswith("asym"):
        a = rng.normal(size=(D, D))
        a = a - a.T
        h0 = h0 + float(name[5:]) * np.abs(h0).sum(axis=0).max() / np.abs(a).sum(axis=0).max() * a  # real, not symmetric
    dt = 0.7 / top_bound(h0, hks, sig, 1.0, edges(D, N))
    ref = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    return frozen(h0, hks, sig, ph, ref) + (dt,)


def test_the_asymmetric_drift_needs_the_complex_path():
    h0, hks, sig, ph, ref, dt = flag_case("asym_1e-6")
    hs = (h0 + h0.T) / 2
    assert np.abs(h0 - hs).max() > 0
    moved = np.abs(o.propagate_batch(hs, hks, sig, dt, fr_phase=ph) - ref).max()
    print(f"asymmetry 1e-6 of the norm: symmetrising moves U by {moved:.3e}")
    assert moved > 1e-8
    h0, hks, sig, ph, ref, dt = flag_case("asym_1e-17")
    assert np.abs(o.propagate_batch((h0 + h0.T) / 2, hks, sig, dt, fr_phase=ph) - ref).max() < 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("name", FLAG_CASES)
def test_flags(prop, name):
    h0, hks, sig, ph, ref, dt = flag_case(name)
    for opts in ({}, {"no_mw": 1}):
        err = np.abs(gpu(prop, h0, hks, sig, dt, ph, **opts) - ref).max()
        print(f"{name} {opts}: max |U - U_oracle| {err:.3e}")
        assert err < TOL


# ---------------------------------------------------------------- the other instances of the prologue
@functools.lru_cache(maxsize=None)
def other_case(D, K):
    rng = np.random.default_rng(9700 + 10 * D + K)
    N, B = 131, 2
    h0 = np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.3)
    hks = np.stack([sym(rng, D, 0.4) for _ in range(K)])
    sig = rng.choice([-1.0, 1.0], size=(B, K, N)) * rng.uniform(0.5, 1.0, size=(B, K, N))
    ph = rng.uniform(0, 6.28, size=(B, D))
    dt = 0.7 / top_bound(h0, hks, sig, 1.0, edges(D, N))
    return frozen(h0, hks, sig, ph, o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)) + (dt,)


@pytest.mark.gpu
@pytest.mark.parametrize("D,K", ((3, 2), (12, 2), (9, 3)))
def test_other_instances(prop, D, K):
    h0, hks, sig, ph, ref, dt = other_case(D, K)
    for opts in ({}, {"no_mw": 1}):
        err = np.abs(gpu(prop, h0, hks, sig, dt, ph, **opts) - ref).max()
        print(f"D={D} K={K} {opts}: max |U - U_oracle| {err:.3e}")
        assert err < TOL
