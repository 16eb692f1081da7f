"""The tail of smalld_chain_kernel in the workgroup-per-sample mode (c3p_smalld.hip): the waves' partial products P_0 .. P_{nW-1}
meet in LDS and are folded as the tree ((P7 P6)(P5 P4))((P3 P2)(P1 P0)), later segment on the left.  The instances that deal
the fold (D = 5 .. 9) form each level on as many waves as it has products, a workgroup barrier between the levels; D <= 4 and
D >= 10 and every one-wave instance keep the fold on one wave.  Every output tile is the same instructions on the same operands
in both forms, so with equal segments the two modes must agree bit for bit.

* D = 5 .. 9 with 8, 16 and 32 segments (nW = 2, 4, 8 waves): B = 3, K = 2, N = 131 (segments of 4 and 5 slices at S = 32, so
  every partial differs from the identity and from its neighbours), signals that differ in every slice, frame-rotation phases;
  real symmetric operators, one complex Hermitian control, a lossy drift.  Workgroup per sample with equal segments (mw_skew =
  500) array_equal with one-wave workgroups (no_mw = 1); both, and at S = 32 the default split, within 1e-10 (Frobenius norm
  per sample) of oracle.c3_oracle.propagate_batch.
* The shortest chains the launch layer admits (pick_segments takes a forced segment count only up to S = N, so a segment without a
  slice never reaches the kernel: N = 9 with 32 segments runs unfused with nine): N = 32 with 32 segments, one slice each, and
  N = 9 with 8 segments of one and two slices.
* D = 4 and D = 10 (not dealt) once each.
* CPU: on the oracle, swapping two adjacent partials of any of these inputs moves the result by more than 1e-6, so a wrong
  pairing of the tree cannot pass."""
import functools

import numpy as np
import pytest

from norm_bound_model import bounds, segments
from oracle import c3_oracle as o

TOL = 1e-10
SKEW = {9: 736, 5: 716}  # default long share of the workgroup-per-sample mode, per mille (launch_chain_t)
MW = "c3p_smalld.hip: smalld_chain_kernel<%d, false, false, false, true, "
KINDS = ("real_symmetric", "complex_control", "lossy_drift")
B, K = 3, 2


def sym(rng, D, s):
    m = rng.normal(size=(D, D))
    return (s * (m + m.T) / 2).astype(np.complex128)


def splits(D, N):
    """every split of the time axis the cases run with: equal segments at 8, 16, 32 and the default split of 32"""
    out = [segments(N, S, 500) for S in (8, 16, 32)]
    if N >= 4 * 32:
        out.append(segments(N, 32, SKEW.get(D, 640)))
    return out


@functools.lru_cache(maxsize=None)
def case(D, kind, N=131):
    rng = np.random.default_rng(17000 + 100 * D + 10 * KINDS.index(kind) + N)
    h0 = np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.3)
    hks = np.stack([sym(rng, D, 0.4) for _ in range(K)])
    sig = rng.choice([-1.0, 1.0], size=(B, K, N)) * rng.uniform(0.5, 1.0, size=(B, K, N))  # different in every slice
    ph = rng.uniform(0, 6.28, size=(B, D))
    if kind == "complex_control":
        a = rng.normal(size=(D, D))
        hks[1] = hks[1] + 0.2j * (a - a.T)  # Hermitian
        assert np.array_equal(hks[1], hks[1].conj().T) and np.abs(hks[1].imag).max() > 0.1
    elif kind == "lossy_drift":
        h0 = h0 - 0.05j * np.diag(rng.uniform(0, 1, D))
    top = max(bounds(h0, hks, sig[b], 1.0, n0, n1)[1] for seg in splits(D, N) for b in range(B) for n0, n1 in seg if n1 > n0)
    dt = 0.7 / top
    ref = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    for a in (h0, hks, sig, ph, ref):
        a.setflags(write=False)
    return h0, hks, sig, ph, ref, dt


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


def gpu(prop, c, S, mw, **opts):
    from c3_amd import _lib

    h0, hks, sig, ph, _, dt = c
    D = h0.shape[-1]
    with _lib.options(smalld_segments=S, **opts):
        U = np.asarray(prop.propagate_batch(h0, hks, sig, dt, fr_phase=ph)["U"])
    detail = _lib.last_kernel_detail()
    assert "smalld_chain_kernel<%d, " % D in detail and ((MW % D) in detail) == mw, detail
    return U


def fro(U, ref):
    return max(np.linalg.norm(U[b] - ref[b]) for b in range(ref.shape[0]))


def both_modes(prop, c, S, label, default_split=False):
    ref = c[4]
    Ue = gpu(prop, c, S, True, mw_skew=500)
    U1 = gpu(prop, c, S, False, no_mw=1)
    errs = [fro(Ue, ref), fro(U1, ref)]
    if default_split:
        errs.append(fro(gpu(prop, c, S, True), ref))
    print(f"{label} S={S}: max_b |U - U_oracle|_F equal segments {errs[0]:.3e} one wave {errs[1]:.3e}" + (f" default split {errs[2]:.3e}" if default_split else ""))
    assert max(errs) < TOL
    assert np.array_equal(Ue, U1)


# ---------------------------------------------------------------- CPU: the order of the partials shows
def wave_partials(c, S):
    """[B][nW] products of the slice propagators of each wave's four consecutive segments (equal segments)"""
    h0, hks, sig, ph, ref, dt = c
    seg = segments(sig.shape[2], S, 500)
    out = []
    for b in range(B):
        E = [o.expm(-1j * dt * (h0 + np.tensordot(sig[b][:, n], hks, axes=1))) for n in range(sig.shape[2])]
        row = []
        for w in range(S // 4):
            P = np.eye(h0.shape[-1], dtype=complex)
            for n in range(seg[4 * w][0], seg[4 * w + 3][1]):
                P = E[n] @ P
            row.append(P)
        out.append(row)
    return out


def fold(parts):
    U = np.eye(parts[0].shape[-1], dtype=complex)
    for P in parts:
        U = P @ U
    return U


def swaps_show(c, Ss=(8, 16, 32)):
    ph, ref = c[3], c[4]
    least = np.inf
    for S in Ss:
        parts = wave_partials(c, S)
        for b in range(B):
            rot = np.exp(1j * ph[b])[:, None]
            assert np.linalg.norm(rot * fold(parts[b]) - ref[b]) < 1e-12  # the folded partials ARE the oracle's result
            for w in range(S // 4 - 1):
                p = list(parts[b])
                p[w], p[w + 1] = p[w + 1], p[w]
                moved = np.linalg.norm(rot * fold(p) - ref[b])
                assert moved > 1e-6, (S, b, w, moved)
                least = min(least, moved)
    return least


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", (5, 6, 7, 8, 9))
def test_swapping_adjacent_partials_shows(D, kind):
    print(f"D={D} {kind}: the least a swap of two adjacent partials moves U: {swaps_show(case(D, kind)):.3e}")


SHORT = ((32, 32), (9, 8))  # (N, S)


@pytest.mark.parametrize("N,S", SHORT)
def test_swapping_adjacent_partials_shows_on_the_shortest_chains(N, S):
    lens = [n1 - n0 for n0, n1 in segments(N, S, 500)]
    assert sum(lens) == N and min(lens) == 1 and max(lens) == (N + S - 1) // S
    print(f"N={N} S={S}: the least a swap of two adjacent partials moves U: {swaps_show(case(9, 'real_symmetric', N), (S,)):.3e}")


def test_segments_of_the_cases():
    lens = [n1 - n0 for n0, n1 in segments(131, 32, 500)]
    assert set(lens) == {4, 5} and sum(lens) == 131


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("S", (8, 16, 32))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", (5, 6, 7, 8, 9))
def test_tree_equals_one_wave_fold(prop, D, kind, S):
    both_modes(prop, case(D, kind), S, f"D={D} {kind}", default_split=(S == 32))


@pytest.mark.gpu
@pytest.mark.parametrize("N,S", SHORT)
def test_tree_on_the_shortest_chains(prop, N, S):
    both_modes(prop, case(9, "real_symmetric", N), S, f"D=9 N={N}")


@pytest.mark.gpu
@pytest.mark.parametrize("D", (4, 10))
def test_instances_that_keep_the_one_wave_fold(prop, D):
    both_modes(prop, case(D, "real_symmetric"), 32, f"D={D}", default_split=True)
