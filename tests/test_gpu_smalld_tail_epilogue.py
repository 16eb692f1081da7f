"""The epilogues of the dealt fold products in the workgroup-per-sample mode of smalld_chain_kernel (c3p_smalld.hip, D = 5 .. 9).
The second product of a wave's own fold scales its tiles by the wave's factor e^{tr + i ti} in the block that formed them and
writes the partial once; the last product of the tree over the waves scales its tiles by the frame phases of their rows and
stores them to the result from all four blocks.  Both are the arithmetic of scale_rows / store_plain on the same operands, which
the one-wave mode keeps, so with equal segments the two modes must agree bit for bit.

* D = 5 .. 9 with 8, 16 and 32 segments (nW = 2, 4, 8 waves; one and two tree levels and three), B = 3, K = 2, N = 131, frame
  phases that are no multiples of 2 pi; real symmetric operators, one complex Hermitian control, a lossy drift whose trace has a
  real part (er != 1: the exp branch of the wave's factor).  Workgroup per sample with equal segments (mw_skew = 500) array_equal
  with one-wave workgroups (no_mw = 1); both, and at S = 32 the default split, within 1e-10 (Frobenius norm per sample, the
  project's bound) of oracle.c3_oracle.propagate_batch.
* The shortest chains the launch layer admits: N = 32 with 32 segments (one slice each) and N = 9 with 8 segments.
* D = 4 and D = 10 (not dealt: they keep scale_rows and store_plain) once each.
* CPU, on the oracle and the same inputs: dropping one wave's factor, dropping the row phases, and swapping Re and Im of one row
  at the store each move U by at least 1e-6, so an epilogue that does nothing, or pairs the halves wrongly, cannot pass.
* CPU: the deal of sd_split_deal<D>(4, blk, t), mirrored here, with the store's predicate row < D && col < D: every double of the
  D x D complex result is stored by exactly one (block, task, lane), and nothing of the padding."""
import functools

import numpy as np
import pytest

from norm_bound_model import bounds, segments
from oracle import c3_oracle as o

TOL = 1e-10
GUARD = 1e-6
SKEW = {9: 736, 5: 716}  # default long share of the workgroup-per-sample mode, per mille (launch_chain_t)
MW = "c3p_smalld.hip: smalld_chain_kernel<%d, false, false, false, true, "
KINDS = ("real_symmetric", "complex_control", "lossy_drift")
DS = (5, 6, 7, 8, 9)
B, K = 3, 2
SHORT = ((32, 32), (9, 8))  # (N, S)


def sym(rng, D, s):
    m = rng.normal(size=(D, D))
    return (s * (m + m.T) / 2).astype(np.complex128)


def splits(D, N):
    out = [segments(N, S, 500) for S in (8, 16, 32)]
    if N >= 4 * 32:
        out.append(segments(N, 32, SKEW.get(D, 640)))
    return out


@functools.lru_cache(maxsize=None)
def case(D, kind, N=131):
    rng = np.random.default_rng(18000 + 100 * D + 10 * KINDS.index(kind) + N)
    h0 = np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + sym(rng, D, 0.3)
    hks = np.stack([sym(rng, D, 0.4) for _ in range(K)])
    sig = rng.choice([-1.0, 1.0], size=(B, K, N)) * rng.uniform(0.5, 1.0, size=(B, K, N))  # different in every slice
    ph = rng.uniform(0.3, 6.0, size=(B, D))  # no multiple of 2 pi
    if kind == "complex_control":
        a = rng.normal(size=(D, D))
        hks[1] = hks[1] + 0.2j * (a - a.T)  # Hermitian
        assert np.array_equal(hks[1], hks[1].conj().T) and np.abs(hks[1].imag).max() > 0.1
    elif kind == "lossy_drift":
        h0 = h0 - 0.05j * np.diag(rng.uniform(0.2, 1, D))
        assert np.trace(h0).imag < -0.05  # the generator's trace -i dt tr(h) has a real part: er = e^{tr} != 1
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


# ---------------------------------------------------------------- CPU: what the epilogues apply shows in the result
@functools.lru_cache(maxsize=None)
def wave_partials(D, kind, N, S):
    """[B][nW] (traceless partial, factor): the product of exp(-i dt (H_n - tr H_n / D)) over the slices of each wave's four
    consecutive segments (equal segments) and the scalar e^{tr + i ti} = prod_n exp(-i dt tr H_n / D) the kernel carries beside it"""
    h0, hks, sig, ph, ref, dt = case(D, kind, N)
    seg = segments(N, S, 500)
    out = []
    for b in range(B):
        H = [h0 + np.tensordot(sig[b][:, n], hks, axes=1) for n in range(N)]
        mu = [-1j * dt * np.trace(h) / D for h in H]
        E = [o.expm(-1j * dt * h - m * np.eye(D)) for h, m in zip(H, mu)]
        row = []
        for w in range(S // 4):
            P, f = np.eye(D, dtype=complex), 1.0 + 0j
            for n in range(seg[4 * w][0], seg[4 * w + 3][1]):
                P, f = E[n] @ P, f * np.exp(mu[n])
            row.append((P, f))
        out.append(row)
    return out


def fold(parts, skip=None):
    """the scaled partials folded, later segment on the left; `skip`: the wave whose factor is dropped"""
    U = np.eye(parts[0][0].shape[-1], dtype=complex)
    for w, (P, f) in enumerate(parts):
        U = (P if w == skip else f * P) @ U
    return U


def guards(D, kind, N=131, Ss=(8, 16, 32)):
    """the least that (a) one wave's dropped factor, (b) dropped row phases, (c) Re and Im of one row swapped at the store move U"""
    ph, ref = case(D, kind, N)[3:5]
    least = [np.inf, np.inf, np.inf]
    for S in Ss:
        parts = wave_partials(D, kind, N, S)
        for b in range(B):
            rot = np.exp(1j * ph[b])[:, None]
            V = fold(parts[b])
            assert np.linalg.norm(rot * V - ref[b]) < 1e-12  # the scaled partials, folded and rotated, ARE the oracle's result
            if S == Ss[0]:
                least[1] = min(least[1], np.linalg.norm(V - ref[b]))
                for i in range(D):
                    sw = ref[b].copy()
                    sw[i] = ref[b][i].imag + 1j * ref[b][i].real
                    least[2] = min(least[2], np.linalg.norm(sw - ref[b]))
            for w in range(S // 4):
                least[0] = min(least[0], np.linalg.norm(rot * fold(parts[b], skip=w) - ref[b]))
    assert min(least) >= GUARD, least
    return least


@pytest.mark.parametrize("D", DS)
def test_lossy_drift_takes_the_exp_branch(D):
    """er = |e^{tr + i ti}| differs from 1 in every wave of the lossy cases and is 1 in the Hermitian ones"""
    for kind in KINDS:
        mod = [abs(f) for S in (8, 16, 32) for row in wave_partials(D, kind, 131, S) for _, f in row]
        if kind == "lossy_drift":
            assert max(mod) < 1 - 1e-4
        else:
            assert np.allclose(mod, 1.0, rtol=0, atol=1e-14)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", DS)
def test_dropped_factor_phases_or_swapped_halves_show(D, kind):
    a, b, c = guards(D, kind)
    print(f"D={D} {kind}: the least U moves: a wave's factor dropped {a:.3e}, row phases dropped {b:.3e}, Re/Im of a row swapped {c:.3e}")


@pytest.mark.parametrize("N,S", SHORT)
def test_dropped_factor_phases_or_swapped_halves_show_on_the_shortest_chains(N, S):
    lens = [n1 - n0 for n0, n1 in segments(N, S, 500)]
    assert sum(lens) == N and min(lens) == 1 and max(lens) == (N + S - 1) // S
    a, b, c = guards(9, "real_symmetric", N, (S,))
    print(f"N={N} S={S}: the least U moves: a wave's factor dropped {a:.3e}, row phases dropped {b:.3e}, Re/Im of a row swapped {c:.3e}")


# ---------------------------------------------------------------- CPU: the deal of the store
def split_deal(D, nb, blk, task):
    """sd_split_deal<D>(nb, blk, task) of c3p_smalld.hip: (I, J, on)"""
    NBI, NJ = (D + 1) // 2, (D + 3) // 4
    per = (NBI * NJ + nb - 1) // nb
    full, rem = NBI // per, NBI % per
    if blk < NJ * full:
        return (blk % full) * per + task, blk // full, True
    idx = (blk - NJ * full) * per + task
    if rem == 0 or idx >= NJ * rem:
        return 0, 0, False
    return full * per + idx % rem, idx // rem, True


@pytest.mark.parametrize("D", DS)
def test_dealt_store_writes_every_element_once_and_no_padding(D):
    NBI, NJ = (D + 1) // 2, (D + 3) // 4
    per = (NBI * NJ + 3) // 4
    stored = np.zeros((2 * NBI, 4 * NJ, 2), dtype=int)  # [row][col][Re, Im] of the padded result
    tiles = np.zeros((NBI, NJ), dtype=int)
    for blk in range(4):
        for t in range(per):
            I, J, on = split_deal(D, 4, blk, t)
            assert 0 <= I < NBI and 0 <= J < NJ
            tiles[I, J] += on
            for lane in range(64):
                r, b, c = lane >> 4, (lane >> 2) & 3, lane & 3
                if b != blk:
                    continue
                row, col = 2 * I + (r >> 1), 4 * J + c
                if on and row < D and col < D:  # the predicate of the store
                    stored[row, col, r & 1] += 1
    assert (tiles == 1).all()
    assert (stored[:D, :D] == 1).all()
    assert stored.sum() == 2 * D * D  # nothing of the padding


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("S", (8, 16, 32))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", DS)
def test_epilogues_equal_one_wave_fold(prop, D, kind, S):
    both_modes(prop, case(D, kind), S, f"D={D} {kind}", default_split=(S == 32))


@pytest.mark.gpu
@pytest.mark.parametrize("N,S", SHORT)
def test_epilogues_on_the_shortest_chains(prop, N, S):
    both_modes(prop, case(9, "real_symmetric", N), S, f"D=9 N={N}")


@pytest.mark.gpu
@pytest.mark.parametrize("D", (4, 10))
def test_instances_that_keep_scale_rows_and_store_plain(prop, D):
    both_modes(prop, case(D, "real_symmetric"), 32, f"D={D}", default_split=True)
