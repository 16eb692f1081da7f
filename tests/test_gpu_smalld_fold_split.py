"""The fold of the small-D chain kernel's fused tail on the split product (c3p_smalld.hip: mm_split, fold_slots): in the
workgroup-per-sample instances of D = 5 .. 9 the output tiles of the fold's products are dealt over the MFMA blocks of the slots that
have no product of their own; every other instance (one-wave workgroups, D <= 4, D >= 10) keeps one chain per block.

* test_modes_bit_for_bit: with equal segments the workgroup-per-sample mode and the one-wave ticket mode are array_equal, over
  D in {2, 3, 4, 5, 7, 9, 10, 12} (1, 2, 2, 6, 8, 15, 15, 18 output tiles: every remainder of the deal over two and four blocks),
  two, four and eight waves per sample, K in {0, 2}, real-symmetric and complex Hermitian control operators (both entries of
  fold_slots: the real loops leave their state as images, the complex loop in registers).  At D = 5, 7, 9 this pins the dealt fold
  bit for bit to the one-chain-per-block fold, which the one-wave mode runs: a wrong deal shows here, not only at the parity bar.
* test_parity_against_the_oracle: the same cases with the default split of the time axis, and S = 4 (one wave: the in-wave fold
  alone), a D = 3 Lindblad batch (Dm = 9) and per-sample drifts, max |U - U_oracle| < 1e-11 as in tests/test_gpu_round2.py.
* Every GPU case first asserts on the CPU (order_guard, also run alone as test_inputs_tell_the_order_of_the_partials), from the
  oracle's per-slice propagators, that exchanging any two neighbouring segment partials moves the result by more than 1e-6 -- at
  the balanced cuts and, for eight waves, at the uneven cuts of the default split.  A fold that multiplies in the wrong order cannot
  then pass the parity bar by luck.  ONLY THE K = 2 CASES GUARD THE ORDER: with K = 0 every slice of a sample is the same matrix, all
  partials are powers of it and commute whatever the input (the row phases are applied once, on the left of the whole product), so
  no K = 0 input can make the order visible.  For those cases the guard asserts that the partials do commute, and they are held to
  the parity bar and the bit-for-bit pin, which a dropped or repeated tile still fails.
* test_repeatable: two identical calls are array_equal.

The oracle's propagators are computed once per case and shared."""
import functools

import numpy as np
import pytest

from oracle import c3_oracle as o

TOL = 1e-11
DT = 1e-11
DIMS = (2, 3, 4, 5, 7, 9, 10, 12)
B = 3


def rsym(rng, D, scale):
    a = rng.normal(size=(D, D))
    return (scale * (a + a.T) / 2).astype(complex)


def with_imaginary_part(h):
    """as bench.py --complex: Hermitian, complex"""
    up = np.triu(h.real, 1)
    return h + 0.3j * (up - up.T)


def n_slices(S):
    return 4 * S + 3  # a little above 4 S (the uneven split of eight waves applies), odd: no multiple of S


CASES = {}
for _D in DIMS:
    for _S in (8, 16, 32):
        for _K in (0, 2):
            for _kind in ("real", "complex"):
                CASES[f"d{_D}_s{_S}_k{_K}_{_kind}"] = dict(D=_D, S=_S, K=_K, kind=_kind)
MODE_CASES = list(CASES)  # (half of them K = 0: no guard against a wrong order of the partials there, see the module docstring)
for _D in DIMS:
    CASES[f"d{_D}_s4_k2_real"] = dict(D=_D, S=4, K=2, kind="real")
CASES["d9_s4_k2_complex"] = dict(D=9, S=4, K=2, kind="complex")
for _S in (4, 8, 32):
    CASES[f"lindblad_d3_s{_S}"] = dict(D=3, S=_S, K=2, kind="lindblad")
    CASES[f"d9_s{_S}_per_sample_h0"] = dict(D=9, S=_S, K=2, kind="per_sample")
CASES["d7_s16_per_sample_h0"] = dict(D=7, S=16, K=2, kind="per_sample")


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs, the oracle's per-slice propagators dU [B, N, Dm, Dm] and the oracle's result"""
    kw = CASES[name]
    D, S, K, kind = kw["D"], kw["S"], kw["K"], kw["kind"]
    N = n_slices(S)
    rng = np.random.default_rng(sorted(CASES).index(name) + 77000)
    h0 = rsym(rng, D, 3e10)
    hks = np.stack([rsym(rng, D, 1.0) for _ in range(K)]) if K else np.zeros((0, D, D), complex)
    sig = rng.normal(size=(B, K, N)) * 1e10
    col = None
    ph = rng.uniform(0, 6, size=(B, D))
    if kind == "complex":
        if K:
            hks[min(1, K - 1)] = with_imaginary_part(hks[min(1, K - 1)])
        else:
            h0 = with_imaginary_part(h0)
    elif kind == "per_sample":
        h0 = np.stack([rsym(rng, D, 3e10) for _ in range(B)])
    elif kind == "lindblad":
        # (decay rates of 0.01 per slice: at 0.1 the propagator of 131 slices has shrunk to 1e-6 and no exchange could move it)
        col = (rng.normal(size=(2, D, D)) + 1j * rng.normal(size=(2, D, D))) * 1e4
        ph = None
    dU = []
    for b in range(B):
        h0b = h0[b] if h0.ndim == 3 else h0
        if kind == "lindblad":
            dU.append(o.tf_propagation_lind(h0b, hks, col, sig[b], DT))
        elif K:
            dU.append(o.tf_propagation_vectorized(h0b, hks, sig[b], DT))
        else:
            dU.append(np.stack([o.expm(-1j * DT * h0b)] * N))
    ref = o.propagate_batch(h0, hks, sig, DT, col_ops=col, lindbladian=kind == "lindblad", fr_phase=ph) if h0.ndim == 2 else \
        np.stack([o.propagate_batch(h0[b], hks, sig[b : b + 1], DT, fr_phase=ph[b : b + 1])[0] for b in range(B)])
    return dict(kw, N=N, h0=h0, hks=hks, sig=sig, col=col, ph=ph, dU=np.stack(dU), ref=ref)


def fold(parts):
    U = parts[0]
    for p in parts[1:]:
        U = p @ U  # the later segment on the left
    return U


def segment_edges(N, S, per_mille):
    """first slice of every chain as launch_chain_t / split_segments cut them (per_mille = 500: balanced)"""
    if S == 32 and N >= 4 * S and per_mille != 500:
        h = S // 2
        la = max(1, (N * per_mille) // (500 * S))
        if h * la > N - h:
            la = (N - h) // h
        rest = N - h * la
        return [g * la if g <= h else h * la + ((g - h) * rest) // h for g in range(S + 1)]
    return [(g * N) // S for g in range(S + 1)]


@functools.lru_cache(maxsize=None)
def order_guard(name):
    """asserts that the case's inputs tell the order of the segment partials (K > 0), at the cuts of every split a test uses"""
    c = case(name)
    S, N = c["S"], c["N"]
    cuts = {tuple(segment_edges(N, S, pm)) for pm in (500, 640, 700, 704)}  # equal shares; the defaults of the complex loop, D = 5, D = 9
    assert len(cuts) == (2 if S == 32 else 1)
    for edges in cuts:
        moved = []
        for b in range(B):
            parts = [fold(list(c["dU"][b, n0:n1])) for n0, n1 in zip(edges, edges[1:])]
            U = fold(parts)
            # the per-slice propagators reproduce the oracle's result (row phases apart)
            want = c["ref"][b] if c["ph"] is None else np.exp(-1j * c["ph"][b])[:, None] * c["ref"][b]
            assert np.abs(U - want).max() < 1e-12
            for j in range(S - 1):
                sw = list(parts)
                sw[j], sw[j + 1] = sw[j + 1], sw[j]
                moved.append(np.abs(fold(sw) - U).max())
        if c["K"] == 0:
            assert max(moved) < 1e-12  # powers of one matrix: the order cannot show (see the module docstring)
        else:
            assert min(moved) > 1e-6, min(moved)
    return c


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_tell_the_order_of_the_partials(name):
    order_guard(name)


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


def run(prop, c, **opts):
    from c3_amd import _lib

    more = dict(col_ops=c["col"], lindbladian=True) if c["kind"] == "lindblad" else {}
    with _lib.options(smalld_segments=c["S"], **opts):
        return np.asarray(prop.propagate_batch(c["h0"], c["hks"], c["sig"], DT, fr_phase=c["ph"], **more)["U"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODE_CASES)
def test_modes_bit_for_bit(prop, name):
    c = order_guard(name)
    Ue = run(prop, c, mw_skew=500)
    U0 = run(prop, c, no_mw=1)
    assert np.array_equal(Ue, U0)
    assert np.abs(Ue - c["ref"]).max() < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_parity_against_the_oracle(prop, name):
    c = order_guard(name)
    U = run(prop, c)
    err = np.abs(U - c["ref"]).max()
    print(f"{name}: max |U - U_oracle| {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["d9_s32_k2_real", "d9_s32_k2_complex", "d12_s16_k2_real", "d5_s8_k0_real", "d9_s4_k2_real", "lindblad_d3_s32"])
def test_repeatable(prop, name):
    c = order_guard(name)
    assert np.array_equal(run(prop, c), run(prop, c))
