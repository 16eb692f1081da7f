"""The small-D backward sweeps (smalld_grad_real_kernel, smalld_grad_kernel, smalld_grad_general_kernel, smallr_grad_kernel) on
long and uneven time segments.

The segment rules of c3p_api.hip (pick_segments, pick_segments_r, lind_small_segments) give every small test shape segments of ONE
slice: B S stays far below the slot count, so rounds = 1 and the cost (N / S + 8) is smallest at S = N.  At that length the
in-segment recursion of the sweeps (M_n = dU_n^+ M_{n+1} dU_n, the local prefixes of the general sweeps), the second pass of the
amplitude staging loop, the padding slices of uneven segments, the forward pass on 2 S segments and the per-wave hand-over between
the real and the general sweep are computed and never used, or never run.  Here the `smalld_segments` option pins S, so that one
sample of N = 67 slices is cut into segments of 67, 33/34, 22/23, 16/17, 13/14, 8/9 slices and of one slice (the control).

Every case compares with the CPU oracle (oracle/c3_oracle.py) at the bar of tests/test_gradient.py, max|g - want| < 1e-10 max|want|
per sample; 2e-9 where a slice is deliberately past three squarings (tests/test_gpu_round2.py,
test_vjp_real_hamiltonian_small_dims).  The inputs and references are checked without a GPU by the four CPU tests at the end:
finite differences of the oracle's propagator, the oracle's own error against an eigen-decomposition form of the same gradient,
a floor under the largest entry of every reference, and the bounds of the hand-over case.

Every comparison prints one line `SEGERR <family> S=<S> <max_b max|g - want| / max|want|>`; DESIGN.md 5.6 records the worst per
family and S of one run."""
import functools

import numpy as np
import pytest

from norm_bound_model import bounds, segments
from oracle import c3_oracle as o

B, N = 3, 67
S_SHARED = (1, 2, 3, 4, 5, 8, 67)  # segments of 67, 33/34, 22/23, 16/17, 13/14, 8/9 and 1 slices; B S = 3, 9, 15: invalid chains in the last wave
S_PER_SAMPLE = (4, 8, 16, 36)  # per-sample tables: a wave must stay within one sample
S_SMALLR = (1, 4, 15, 16, 17, 35, 70)  # N = 70: the plain scan below 16, the blocked scan at 16 and at 17 (no multiple of its 8 or 4 wavefronts)
BAR, BAR_SQ = 1e-10, 2e-9
MM8_THETA, T18_THETA, SDG_MAXS = 1.85, 1.13, 3  # c3p_common.h, c3p_smalld.hip
REAL_LIMIT = MM8_THETA * 2**SDG_MAXS  # column-wise bound above which a wave leaves the real sweep
# The general sweep squares without a cap (c3p_squarings stops at 40).  Every squaring doubles the relative error of the pair
# (T, dT); the 2e-9 bar of test_vjp_real_hamiltonian_small_dims was set at |H| dt ~ 10 rad, four to five squarings of
# theta_18 = 1.13.  The hand-over case stays within five.
GENERAL_LIMIT = T18_THETA * 2**5
# Floor of the largest reference entry.  |g[k, n]| = |Re <W_n, L(X_n; G_k)>| <= ||Ubar||_F dt ||h_k||_F for unitary slices (||L|| <=
# ||G_k||, ||W_n||_F = ||Ubar||_F), and the kernels' absolute error is a few hundred roundoffs of that product.  With
# max|want| >= 1e-3 of it, the relative bar 1e-10 sits at 1e-13 of the product: well above roundoff, seven orders below a wrong slice.
FLOOR = 1e-3


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import _lib, propagation

    _lib.require_gpu()
    return propagation


def _mat(rng, D, kind):
    a = rng.normal(size=(D, D))
    if kind != "real":
        a = a + 1j * rng.normal(size=(D, D))
    return ((a + a.conj().T) / 2).astype(np.complex128)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _hb(h0, b):
    return h0[b] if h0.ndim == 3 else h0


def col_bound(h0, hks, sig, dt, b, n0=0, n1=None):
    return bounds(_hb(h0, b), hks, sig[b], dt, n0, sig.shape[-1] if n1 is None else n1)[1]


# ------------------------------------------------------------------------------------------------------------------------------
# inputs (all cached: one draw and one reference per case, shared by the GPU tests and the CPU checks)
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unitary_case(D, kind, target, per_sample=False, nb=B, n=N, K=None, phase=None):
    """operators (real symmetric or complex Hermitian), signals of magnitude 2.4 .. 4 and random sign, and dt such that
    the largest column-wise bound of a whole sample is `target`: every segment's bound lies in (0.6 target, target].
    K = 3 for odd D, 1 for even D; frame phases in half the cases.  (K, phase: set by tests/test_gpu_tiled_sweep.py, which
    shares these operators; left at None they change nothing.)"""
    rng = np.random.default_rng(5000 + 97 * D + int(10 * target) + (1 if kind == "real" else 0) + (500 if per_sample else 0) + n
                                + (0 if K is None else 100000 * K + 1000 * nb))
    K = (3 if D % 2 else 1) if K is None else K
    # A multi-level system in the lab frame: a drift that is mostly diagonal (centred at zero) and drives without a diagonal, every
    # table trace-free with a set 1-norm, plus a small multiple of the identity (the trace shift mu_k of its table).  Why the
    # structure: the oracle restates TensorFlow's expm, which takes the trace along and does not scale a matrix of 1-norm below
    # 10.7, on the slice generators and on the 2 D x 2 D block matrix of every Frechet derivative.  Its own error grows with the
    # SPECTRAL radius of what it is given.  At D = 2 and a bound of 5, where the column-wise bound is the norm itself, operators
    # drawn as dense random matrices left it at 6e-10 (drift diag(U(0, 1)): mostly trace) and 4e-8 (centred) of the largest
    # entry, measured against spectral_signal_gradient below -- and both sweeps on the GPU, at every S, differed from the oracle
    # by that same 5.81e-10.  With a diagonal drift and off-diagonal drives the spectral radius at D = 2 stays near
    # bound / sqrt(2), and test_the_oracle_itself_is_two_orders_below_the_bar holds every reference of this module to 1e-12.
    off = lambda m: m - np.diag(np.diag(m))
    unit = lambda h: (lambda g: g / np.abs(g).sum(axis=0).max())(h - np.trace(h).real / D * np.eye(D))  # trace-free, 1-norm 1
    drift = lambda: unit(np.diag(rng.uniform(-0.5, 0.5, D)).astype(np.complex128) + 0.1 * off(_mat(rng, D, kind))) + 0.05 * rng.uniform(-1, 1) * np.eye(D)
    h0 = np.stack([drift() for _ in range(nb)]) if per_sample else drift()
    # (the direction of every derivative, dt h_k, adds to the norm of the oracle's block matrix: drives of norm 1 / 4, amplitudes of 4)
    hks = np.stack([0.25 * unit(off(_mat(rng, D, kind))) + 0.0125 * rng.uniform(-1, 1) * np.eye(D) for _ in range(K)])
    sig = 4.0 * rng.uniform(0.6, 1.0, size=(nb, K, n)) * rng.choice([-1.0, 1.0], size=(nb, K, n))
    dt = target / max(col_bound(h0, hks, sig, 1.0, b) for b in range(nb))
    Ubar = rng.normal(size=(nb, D, D)) + 1j * rng.normal(size=(nb, D, D))
    ph = rng.uniform(0, 6, size=(nb, D)) if ((D + int(10 * target) + int(per_sample)) % 2 if phase is None else phase) else None
    return tuple(_frozen(x) if isinstance(x, np.ndarray) else x for x in (h0, hks, sig, dt, Ubar, ph))


def _signal_gradients(h0, hks, sig, dt, Ubar, ph):
    return _frozen(np.stack([o.pwc_signal_gradient(_hb(h0, b), hks, sig[b], dt, Ubar[b], None if ph is None else ph[b]) for b in range(sig.shape[0])]))


@functools.lru_cache(maxsize=None)
def unitary_want(*key):
    return _signal_gradients(*unitary_case(*key))


@functools.lru_cache(maxsize=None)
def handover_case(per_sample):
    """D = 9, real operators, column-wise bound 1.5 everywhere except ONE slice in the middle of sample 0 (n = 33) whose amplitudes
    are raised until the column-wise bound of the segment that holds it is 16.5 > 8 x 1.85: the wave of that segment leaves the
    real sweep, every other wave stays.  per_sample: h0 [B,D,D] with sample 1 complex Hermitian (the whole sample goes to the
    general sweep) between two real samples."""
    D, K, n_strong = 9, 3, 33
    rng = np.random.default_rng(6100 + int(per_sample))
    drift = lambda kind: np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + 0.3 * _mat(rng, D, kind)
    h0 = np.stack([drift("real"), drift("complex"), drift("real")]) if per_sample else drift("real")
    hks = np.stack([0.5 * _mat(rng, D, "real") for _ in range(K)])
    sig = rng.uniform(0.6, 1.0, size=(B, K, N)) * rng.choice([-1.0, 1.0], size=(B, K, N))
    dt = 1.5 / max(col_bound(h0, hks, sig, 1.0, b) for b in range(B))
    base = sig[0, :, n_strong].copy()
    lo, hi = 1.0, 1e3
    for _ in range(60):  # the bound of the segment is monotonic in the factor
        f = 0.5 * (lo + hi)
        sig[0, :, n_strong] = f * base
        lo, hi = (f, hi) if col_bound(h0, hks, sig, dt, 0, n_strong, n_strong + 1) < 16.5 else (lo, f)
    sig[0, :, n_strong] = hi * base
    Ubar = rng.normal(size=(B, D, D)) + 1j * rng.normal(size=(B, D, D))
    ph = rng.uniform(0, 6, size=(B, D))
    return tuple(_frozen(x) if isinstance(x, np.ndarray) else x for x in (h0, hks, sig, dt, Ubar, ph))


@functools.lru_cache(maxsize=None)
def handover_want(per_sample):
    return _signal_gradients(*handover_case(per_sample))


def handover_waves(per_sample, S):
    """per wave of the launch (four consecutive chains of the flattened [B, S] index; S % 4 == 0: one sample per wave)
    (sample, first slice, last slice + 1, column-wise bound, sum of norms, real tables)"""
    h0, hks, sig, dt, _, _ = handover_case(per_sample)
    seg = segments(N, S, per_mille=500)  # [g N / S, (g + 1) N / S): the segments of the sweeps
    out = []
    for b in range(B):
        real = bool(np.abs(_hb(h0, b).imag).max() == 0.0)
        for w in range(S // 4):
            per = [bounds(_hb(h0, b), hks, sig[b], dt, *seg[4 * w + q]) for q in range(4)]
            out.append((b, seg[4 * w][0], seg[4 * w + 3][1], max(p[1] for p in per), max(p[2] for p in per), real))
    return out


def handed_over(per_sample, S):
    """[B, N] mask of the slices whose wave the real sweep leaves to the general one; asserts that every wave is well away from the
    threshold and that the general sweep's own bound (the sum of norms) stays within five squarings"""
    mask = np.zeros((B, N), dtype=bool)
    for b, n0, n1, col, son, real in handover_waves(per_sample, S):
        assert col <= son * (1 + 1e-14)
        assert col > 1.02 * REAL_LIMIT or col < 0.5 * REAL_LIMIT, (b, n0, col)
        if not real or col > REAL_LIMIT:
            assert son <= GENERAL_LIMIT, (b, n0, son)
            mask[b, n0:n1] = True
    return mask


@functools.lru_cache(maxsize=None)
def lindblad_case(D, C, hermitian, n=N, col_scale=0.1, per_sample_col=False, K=None, nb=B, phase=None):
    """the operators of test_lindblad_vjp_small_superoperators_general_sweep (dt = 0.3) with weaker collapse operators, so that 20
    time units of dissipation leave the gradient well above roundoff; non-Hermitian: h0 + 0.1 x complex Gaussian
    (nb, phase: set by tests/test_gpu_tiled_sweep.py; at their defaults they change nothing)"""
    rng = np.random.default_rng(7100 + 100 * D + 10 * C + int(hermitian) + n + (3 if per_sample_col else 0) + (0 if nb == B else 1000 * nb))
    herm = lambda s: s * _mat(rng, D, "complex")
    K = (3 if C == 1 else 1) if K is None else K
    h0 = herm(0.8)
    if not hermitian:
        h0 = h0 + 0.1 * (rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D)))
    hks = np.stack([herm(0.5) for _ in range(K)])
    shape = (nb, C, D, D) if per_sample_col else (C, D, D)
    col = col_scale * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    if per_sample_col:
        col = col * np.resize([0.5, 1.0, 2.0], nb)[:, None, None, None]  # a kernel that reads another sample's dissipator misses by O(1)
    sig = rng.uniform(-1, 1, size=(nb, K, n))
    Dm = D * D
    Ubar = rng.normal(size=(nb, Dm, Dm)) + 1j * rng.normal(size=(nb, Dm, Dm))
    ph = rng.uniform(0, 2 * np.pi, size=(nb, Dm)) if ((D + C) % 2 if phase is None else phase) else None
    return tuple(_frozen(x) if isinstance(x, np.ndarray) else x for x in (h0, hks, sig, 0.3, col, Ubar, ph))


@functools.lru_cache(maxsize=None)
def lindblad_want(*key):
    h0, hks, sig, dt, col, Ubar, ph = lindblad_case(*key)
    return _frozen(np.stack([o.pwc_lindblad_signal_gradient(h0, hks, col[b] if col.ndim == 4 else col, sig[b], dt, Ubar[b], None if ph is None else ph[b])
                             for b in range(sig.shape[0])]))


@functools.lru_cache(maxsize=None)
def per_slice_case(D, hermitian, nb=B, n=N, loss=0.05):
    """the slice Hamiltonians of test_per_slice_vjp_on_chip_sweeps: Hermitian, or lossy and non-normal (a sixth of the loss there: 67
    slices of it leave the cotangents at a fifth of their size, not at 1e-4; tests/test_gpu_tiled_sweep.py takes four slices at the
    full loss, 0.3)"""
    rng = np.random.default_rng(7300 + 10 * D + int(hermitian) + (0 if (nb, n) == (B, N) else 1000 * nb + n))
    s = 0.5 / np.sqrt(D)

    def mat():
        h = s * _mat(rng, D, "complex")
        if hermitian:
            return h
        g = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
        up = np.triu(rng.normal(size=(D, D)), 1) * (1.0 + np.arange(D)[:, None]) / D
        return h - 1j * loss * s * (g @ g.conj().T) / D + 0.5 * s * up

    Hs = np.stack([np.stack([mat() for _ in range(n)]) for _ in range(nb)])
    Ubar = rng.normal(size=(nb, D, D)) + 1j * rng.normal(size=(nb, D, D))
    ph = rng.uniform(0, 2 * np.pi, size=(nb, D))
    return _frozen(Hs), 1.1, _frozen(Ubar), _frozen(ph)


@functools.lru_cache(maxsize=None)
def per_slice_want(D, hermitian):
    Hs, dt, Ubar, ph = per_slice_case(D, hermitian)
    return _frozen(np.stack([o.pwc_per_slice_hamiltonian_cotangents(Hs[b], dt, Ubar[b], ph[b]) for b in range(B)]))


GOAL = {9: ([3, 3], [0, 1]), 3: ([3], [0])}  # D -> (dims, index)


@functools.lru_cache(maxsize=None)
def goal_case(D, key=None, goal=None):
    """(key, goal: the unitary_case key and the (dims, index) of a dimension GOAL does not list, set by
    tests/test_gpu_valu_grad_sweep.py; left at None they change nothing)"""
    h0, hks, sig, dt, _, _ = unitary_case(*((D, "real", 1.5, False) if key is None else key))
    rng = np.random.default_rng(7500 + D)
    L = 2 ** len((GOAL[D] if goal is None else goal)[1])
    q, _ = np.linalg.qr(rng.normal(size=(L, L)) + 1j * rng.normal(size=(L, L)))
    ph = rng.uniform(0, 6, size=(sig.shape[0], D))
    return h0, hks, sig, dt, _frozen(q), _frozen(ph)


@functools.lru_cache(maxsize=None)
def goal_want(D):
    """(goal [B], d goal / d signals [B,K,N], cotangents [B,D,D]) from the oracle alone"""
    h0, hks, sig, dt, q, ph = goal_case(D)
    dims, index = GOAL[D]
    U = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    Ubar = np.stack([o.unitary_infid_cotangent(q, U[b], index, dims) for b in range(B)])
    goal = np.array([o.unitary_infid(q, U[b], index=index, dims=dims) for b in range(B)])
    return _frozen(goal), _signal_gradients(h0, hks, sig, dt, Ubar, ph), _frozen(Ubar)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ------------------------------------------------------------------------------------------------------------------------------
def rel_err(g, want):
    g = np.asarray(g)
    assert g.shape == want.shape, (g.shape, want.shape)
    return max(np.abs(g[b] - want[b]).max() / np.abs(want[b]).max() for b in range(want.shape[0]))


def check(g, want, bar, family, S, what=()):
    err = rel_err(g, want)
    print(f"SEGERR {family} S={S} {err:.3e}")
    assert err < bar, (family, S, *what, err)
    return np.asarray(g)


def detail():
    from c3_amd import _lib

    return _lib.last_kernel_detail()


def vjp(prop, case, S, **opts):
    from c3_amd import _lib

    h0, hks, sig, dt, Ubar, ph = case
    with _lib.options(smalld_segments=S, **opts):
        return np.asarray(prop.propagate_batch_vjp(h0, hks, sig, dt, Ubar, fr_phase=ph))


def lind_vjp(prop, case, S, **opts):
    from c3_amd import _lib

    h0, hks, sig, dt, col, Ubar, ph = case
    with _lib.options(smalld_segments=S, **opts):
        return np.asarray(prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph))


REAL_CASES = [(D, t, False) for D in range(2, 13) for t in (0.6, 1.5, 5.0)] + [(D, 1.5, True) for D in range(2, 13)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,target,per_sample", REAL_CASES)
def test_real_sweep(prop, D, target, per_sample):
    """smalld_grad_real_kernel<D>: the degree-6 pair (0.6), the degree-8 pair (1.5) and one or two squarings (5), against the oracle
    and against the general sweep (no_real_grad) at the same S"""
    key = (D, "real", target, per_sample)
    case, want = unitary_case(*key), unitary_want(*key)
    for S in S_PER_SAMPLE if per_sample else S_SHARED:
        g = check(vjp(prop, case, S), want, BAR, "real" + ("/per-sample" if per_sample else ""), S, key)
        assert f"smalld_grad_real_kernel<{D}>" in detail(), detail()
        if S <= 4:
            assert np.array_equal(g, vjp(prop, case, S))
        gg = check(vjp(prop, case, S, no_real_grad=1), want, BAR, "complex(no_real_grad)", S, key)
        assert "smalld_grad_real_kernel" not in detail(), detail()
        assert np.abs(g - gg).max() < BAR * np.abs(gg).max(), (S, key)


COMPLEX_CASES = [(D, t, False) for D in (2, 3, 5, 8, 9, 12) for t in (0.9, 4.0)] + [(D, 0.9, True) for D in (2, 3, 5, 8, 9, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,target,per_sample", COMPLEX_CASES)
def test_complex_pair_sweep(prop, D, target, per_sample):
    """smalld_grad_kernel<D> on complex Hermitian operators (the real sweep declines every wave)"""
    key = (D, "complex", target, per_sample)
    case, want = unitary_case(*key), unitary_want(*key)
    for S in S_PER_SAMPLE if per_sample else S_SHARED:
        g = check(vjp(prop, case, S), want, BAR, "complex" + ("/per-sample" if per_sample else ""), S, key)
        assert f"smalld_grad_kernel<{D}>" in detail(), detail()
        if S <= 4:
            assert np.array_equal(g, vjp(prop, case, S))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("D", [9, 3])
def test_forward_products_on_twice_the_segments(prop, D, kind):
    """run_vjp_smalld forms the forward products on 2 S segments and multiplies them in pairs with the supplied-matrix mode of the
    chain kernel (its second template argument, GIVEN) while 2 S <= N / 8 = 8: present at S = 1, 2, 4, absent with
    grad_fwd_seg2 = 0 and at S = 5 -- which also shows that the segment override took effect.  Both forms against the oracle."""
    key = (D, kind, 1.5 if kind == "real" else 0.9, False)  # (inputs of the two sweeps' own tests)
    case, want = unitary_case(*key), unitary_want(*key)
    given = f"smalld_chain_kernel<{D}, true,"
    for S in (1, 2, 4):
        g = check(vjp(prop, case, S), want, BAR, "fwd-2S", S, key)
        assert given in detail(), detail()
        assert np.array_equal(g, vjp(prop, case, S))
        check(vjp(prop, case, S, grad_fwd_seg2=0), want, BAR, "fwd-S", S, key)
        assert "smalld_chain_kernel" in detail() and given not in detail(), detail()
    check(vjp(prop, case, 5), want, BAR, "fwd-S", 5, key)
    assert "smalld_chain_kernel" in detail() and given not in detail(), detail()


@pytest.mark.gpu
@pytest.mark.parametrize("per_sample", [False, True])
def test_mixed_hand_over(prop, per_sample):
    """one launch whose waves go both ways: the wave with the strong slice (and, per sample, the complex sample) is left to the
    general sweep, the others stay on the real one.  The bounds are asserted on the host first.  On the device the result of the
    handed-over slices must be bit for bit that of the general sweep run alone (no_real_grad: the same kernel on the same data),
    and differ from it in the last bits elsewhere."""
    case, want = handover_case(per_sample), handover_want(per_sample)
    for S in (4, 8):
        mask = handed_over(per_sample, S)
        assert mask.any() and not mask.all()
        g = check(vjp(prop, case, S), want, BAR_SQ, "hand-over" + ("/per-sample" if per_sample else ""), S)
        assert "smalld_grad_real_kernel<9>" in detail() and "smalld_grad_kernel<9>" in detail(), detail()
        assert np.array_equal(g, vjp(prop, case, S))
        gg = check(vjp(prop, case, S, no_real_grad=1), want, BAR_SQ, "hand-over(no_real_grad)", S)
        m = np.broadcast_to(mask[:, None, :], g.shape)
        assert np.array_equal(g[m], gg[m])
        assert not np.array_equal(g[~m], gg[~m])


@pytest.mark.gpu
@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("D", [2, 3])
def test_general_sweep_lindblad(prop, D, C, hermitian):
    """smalld_grad_general_kernel<D^2, false>: Hermitian Hamiltonians with no_smallr = 1, and a non-Hermitian h0 that the
    Hermitian-basis sweep declines"""
    key = (D, C, hermitian)
    case, want = lindblad_case(*key), lindblad_want(*key)
    opts = {"no_smallr": 1} if hermitian else {}
    got = {}
    for S in S_SHARED:
        g = got[S] = check(lind_vjp(prop, case, S, **opts), want, BAR, "general/lindblad", S, key)
        assert f"smalld_grad_general_kernel<{D * D}, false>" in detail() and "smallr_grad_kernel" not in detail(), detail()
        if S <= 4:
            assert np.array_equal(g, lind_vjp(prop, case, S, **opts))
    assert not np.array_equal(got[1], got[67])  # (another order of the same products: the override reached this path)


@pytest.mark.gpu
@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("D", [5, 12])
def test_general_sweep_per_slice_hamiltonians(prop, D, hermitian):
    """smalld_grad_general_kernel<D, true>: supplied per-slice Hamiltonians"""
    from c3_amd import _lib

    Hs, dt, Ubar, ph = per_slice_case(D, hermitian)
    want = per_slice_want(D, hermitian)
    got = {}
    for S in (1, 4, 67):
        run = lambda: np.asarray(prop.propagate_per_slice_vjp(Hs, dt, Ubar, fr_phase=ph))
        with _lib.options(smalld_segments=S):
            g = got[S] = check(run(), want, BAR, "general/per-slice", S, (D, hermitian))
            assert f"smalld_grad_general_kernel<{D}, true>" in detail(), detail()
            if S <= 4:
                assert np.array_equal(g, run())
    assert not np.array_equal(got[1], got[67])  # (the override reached this path)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [2, 3, 4])
def test_hermitian_basis_sweep(prop, D):
    """smallr_grad_kernel<4 | 9 | 16> next to the plain scan (S < 16), the blocked scan (S >= 16) and, at S = 16, the sequential
    scan again (no_fuse); collapse operators of the size of test_normal_generator_schemes_on_the_small_real_lindblad_kernel;
    per-sample collapse operators at S = 4, 16"""
    key = (D, 1, True, 70, 0.05, False, 2)
    case, want = lindblad_case(*key), lindblad_want(*key)
    name = f"smallr_grad_kernel<{D * D}>"
    for S in S_SMALLR:
        g = check(lind_vjp(prop, case, S), want, BAR, "hermitian-basis", S, key)
        assert name in detail() and ("smallr_scan_blocked_kernel" in detail()) == (S >= 16), detail()
        if S <= 4:
            assert np.array_equal(g, lind_vjp(prop, case, S))
        if S == 16:
            gs = check(lind_vjp(prop, case, S, no_fuse=1), want, BAR, "hermitian-basis(no_fuse)", S, key)
            assert name in detail() and "smallr_scan_blocked_kernel" not in detail(), detail()
            assert np.abs(g - gs).max() < BAR * np.abs(gs).max()
    key = (D, 2, True, 70, 0.05, True, 2)
    case, want = lindblad_case(*key), lindblad_want(*key)
    for S in (4, 16):
        g = check(lind_vjp(prop, case, S), want, BAR, "hermitian-basis/per-sample-col", S, key)
        assert name in detail(), detail()
        if S <= 4:
            assert np.array_equal(g, lind_vjp(prop, case, S))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [9, 3])
def test_fused_goal(prop, D):
    """propagate_batch_goal_vjp on long segments: against the three-call form at the same S (1e-11 of the largest entry, the bar of
    test_fused_goal_vjp_matches_three_call_form_and_oracle) and against the oracle"""
    from c3_amd import _lib, fidelities as fid

    h0, hks, sig, dt, q, ph = goal_case(D)
    dims, index = GOAL[D]
    goal, want, _ = goal_want(D)
    for S in (1, 4):
        with _lib.options(smalld_segments=S):
            r = prop.propagate_batch_goal_vjp(h0, hks, sig, dt, q, index, dims, fr_phase=ph)
            assert f"smalld_grad_real_kernel<{D}>" in detail(), detail()
            r2 = prop.propagate_batch_goal_vjp(h0, hks, sig, dt, q, index, dims, fr_phase=ph)
            U = np.asarray(prop.propagate_batch(h0, hks, sig, dt, fr_phase=ph)["U"])
            Ubar, goal3 = fid.unitary_infid_cotangent(q, U, index, dims)
            g3 = np.asarray(prop.propagate_batch_vjp(h0, hks, sig, dt, np.asarray(Ubar), fr_phase=ph))
        g = check(r["grad_signals"], want, BAR, "fused-goal", S, (D,))
        assert np.array_equal(g, np.asarray(r2["grad_signals"]))
        assert np.abs(np.asarray(r["goal"]) - goal).max() < 1e-11
        assert np.abs(np.asarray(r["goal"]) - np.asarray(goal3)).max() < 1e-12
        assert np.abs(g - g3).max() < 1e-11 * np.abs(g3).max()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("D", [13, 27, 36])
def test_mid_d_one_segment_of_seventy_slices(prop, D, kind):
    """addendum: the mid-D sweeps with grad_target = B (run_vjp_midd: S = 1, one segment of 70 slices) and with their default
    (S = N / 8 = 8)"""
    from c3_amd import _lib

    key = (D, kind, 1.5, False, 2, 70)
    (h0, hks, sig, dt, Ubar, ph), want = unitary_case(*key), unitary_want(*key)
    run = lambda: np.asarray(prop.propagate_batch_vjp(h0, hks, sig, dt, Ubar, fr_phase=ph))
    with _lib.options(grad_target=2):
        check(run(), want, BAR, "mid-D/" + kind, 1, key)
        assert _lib.last_kernel() == "mfma"
    check(run(), want, BAR, "mid-D/" + kind, 8, key)
    assert _lib.last_kernel() == "mfma"


# ------------------------------------------------------------------------------------------------------------------------------
# CPU part: the inputs and the references
# ------------------------------------------------------------------------------------------------------------------------------
def _unitary_keys():
    keys = [(D, "real", t, ps) for D, t, ps in REAL_CASES] + [(D, "complex", t, ps) for D, t, ps in COMPLEX_CASES]
    return keys + [(D, kind, 1.5, False, 2, 70) for D in (13, 27, 36) for kind in ("real", "complex")]


def _lindblad_keys():
    keys = [(D, C, h) for D in (2, 3) for C in (1, 2) for h in (True, False)]
    return keys + [(D, C, True, 70, 0.05, ps, 2) for D in (2, 3, 4) for C, ps in ((1, False), (2, True))]


def _fro(a):
    return float(np.sqrt((np.abs(a) ** 2).sum()))


def _floor_ok(want, ubar_norms, gen_norm):
    """max|want[b]| >= FLOOR ||Ubar[b]||_F max_k ||G_k||_F for every sample"""
    return min(np.abs(want[b]).max() / (ubar_norms[b] * gen_norm) for b in range(want.shape[0])) >= FLOOR


def test_reference_gradients_are_not_at_roundoff_level():
    """every reference of this module: its largest entry per sample is at least FLOOR x ||Ubar||_F dt max_k ||h_k||_F (for the
    Lindblad cases ||G_k||_F = dt ||h_k (x) 1 - 1 (x) h_k^T||_F; for the per-slice cotangents the factor is ||Ubar||_F dt), the scale of
    a gradient entry whose cotangent and generator are aligned.  The relative bar of the GPU tests then means something."""
    for key in _unitary_keys():
        h0, hks, sig, dt, Ubar, ph = unitary_case(*key)
        assert _floor_ok(unitary_want(*key), [_fro(u) for u in Ubar], dt * max(_fro(h) for h in hks)), key
    for ps in (False, True):
        h0, hks, sig, dt, Ubar, ph = handover_case(ps)
        assert _floor_ok(handover_want(ps), [_fro(u) for u in Ubar], dt * max(_fro(h) for h in hks)), ps
    for key in _lindblad_keys():
        h0, hks, sig, dt, col, Ubar, ph = lindblad_case(*key)
        I = np.eye(h0.shape[-1])
        gen = dt * max(_fro(np.kron(h, I) - np.kron(I, h.T)) for h in hks)
        assert _floor_ok(lindblad_want(*key), [_fro(u) for u in Ubar], gen), key
    for D in (5, 12):
        for h in (True, False):
            Hs, dt, Ubar, ph = per_slice_case(D, h)
            assert _floor_ok(per_slice_want(D, h), [_fro(u) for u in Ubar], dt), (D, h)
    for D in GOAL:
        h0, hks, sig, dt, q, ph = goal_case(D)
        goal, want, Ubar = goal_want(D)
        assert _floor_ok(want, [_fro(u) for u in Ubar], dt * max(_fro(h) for h in hks)), D
        assert goal.min() > 1e-3  # (a goal at its minimum has no gradient)


def spectral_signal_gradient(h0, hks, sig, dt, Ubar, ph=None):
    """pwc_signal_gradient for Hermitian Hamiltonians from their eigen-decompositions: dU_n = V e^{-i dt w} V^+ and the Frechet
    derivative by divided differences (Daleckii-Krein), Phi_ij = e^{(x_i + x_j) / 2} sin(y_ij) / y_ij, y = dt (w_j - w_i) / 2 --
    no Pade approximant, no scaling and squaring, no 2 D x 2 D block matrix: an independent measure of the oracle's own error"""
    K, n_sl = sig.shape
    D = h0.shape[-1]
    lam = Ubar.astype(np.complex128)
    if ph is not None:
        lam = np.exp(-1j * ph)[:, None] * lam
    ev, P = [], [np.eye(D, dtype=np.complex128)]
    for n in range(n_sl):
        w, V = np.linalg.eigh(h0 + np.einsum("k,kij->ij", sig[:, n], hks))
        ev.append((w, V))
        P.append((V * np.exp(-1j * dt * w)) @ V.conj().T @ P[-1])
    g = np.zeros((K, n_sl))
    for n in range(n_sl - 1, -1, -1):
        w, V = ev[n]
        Wt = V.conj().T @ (lam @ P[n].conj().T) @ V
        Phi = np.exp(-1j * dt * (w[:, None] + w[None, :]) / 2) * np.sinc(dt * (w[None, :] - w[:, None]) / (2 * np.pi))
        for k in range(K):
            g[k, n] = np.real(np.vdot(Wt, Phi * (V.conj().T @ (-1j * dt * hks[k]) @ V)))
        lam = (V * np.exp(1j * dt * w)) @ V.conj().T @ lam
    return g


def test_the_oracle_itself_is_two_orders_below_the_bar():
    """every unitary reference of this module against spectral_signal_gradient: 1e-12 of the largest entry per sample"""
    cases = [(unitary_case(*key), unitary_want(*key), key) for key in _unitary_keys()]
    cases += [(handover_case(ps), handover_want(ps), ("hand-over", ps)) for ps in (False, True)]
    for D in GOAL:
        h0, hks, sig, dt, q, ph = goal_case(D)
        cases.append(((h0, hks, sig, dt, goal_want(D)[2], ph), goal_want(D)[1], ("goal", D)))
    for (h0, hks, sig, dt, Ubar, ph), want, key in cases:
        for b in range(want.shape[0]):
            g = spectral_signal_gradient(_hb(h0, b), hks, sig[b], dt, Ubar[b], None if ph is None else ph[b])
            assert np.abs(g - want[b]).max() < 1e-12 * np.abs(want[b]).max(), (key, b)


def _fd_check(want_b, loss, sig_b, rng, h):
    """six random entries against central differences, within 1e-6 of the largest entry (test_oracle_gradient_matches_finite_differences)"""
    K, n = sig_b.shape
    for _ in range(6):
        k, t = int(rng.integers(K)), int(rng.integers(n))
        sp, sm = sig_b.copy(), sig_b.copy()
        sp[k, t] += h
        sm[k, t] -= h
        fd = (loss(sp) - loss(sm)) / (2 * h)
        assert abs(fd - want_b[k, t]) < 1e-6 * np.abs(want_b).max(), (k, t, fd, want_b[k, t])


def test_references_match_finite_differences_of_the_oracle_propagator():
    """one sample per case family"""
    rng = np.random.default_rng(1)
    unitary = [((9, "real", 5.0, False), 0), ((5, "complex", 4.0, False), 1), ((12, "real", 1.5, True), 2), ((13, "complex", 1.5, False, 2, 70), 1)]
    for key, b in unitary:
        h0, hks, sig, dt, Ubar, ph = unitary_case(*key)
        loss = lambda s: np.real(np.vdot(Ubar[b], o.propagate_batch(_hb(h0, b), hks, s[None], dt, fr_phase=None if ph is None else ph[b : b + 1])[0]))
        _fd_check(unitary_want(*key)[b], loss, sig[b], rng, 1e-5)
    for ps in (False, True):  # sample 0: the strong slice is one of the entries
        h0, hks, sig, dt, Ubar, ph = handover_case(ps)
        loss = lambda s: np.real(np.vdot(Ubar[0], o.propagate_batch(_hb(h0, 0), hks, s[None], dt, fr_phase=ph[:1])[0]))
        want = handover_want(ps)[0]
        _fd_check(want, loss, sig[0], rng, 1e-5)
        sp, sm = sig[0].copy(), sig[0].copy()
        sp[1, 33] += 1e-5
        sm[1, 33] -= 1e-5
        assert abs((loss(sp) - loss(sm)) / 2e-5 - want[1, 33]) < 1e-6 * np.abs(want).max()
    for key, b in [((3, 2, False), 1), ((2, 1, True), 0), ((4, 2, True, 70, 0.05, True, 2), 2)]:
        h0, hks, sig, dt, col, Ubar, ph = lindblad_case(*key)
        cb = col[b] if col.ndim == 4 else col
        rows = np.ones(Ubar.shape[-1]) if ph is None else np.exp(1j * ph[b])
        loss = lambda s: np.real(np.vdot(Ubar[b], rows[:, None] * o.propagate_batch(h0, hks, s[None], dt, col_ops=cb, lindbladian=True)[0]))
        _fd_check(lindblad_want(*key)[b], loss, sig[b], rng, 1e-5)
    for D, herm in [(5, False), (12, True)]:  # (the rule of test_oracle_per_slice_cotangents_match_finite_differences)
        Hs, dt, Ubar, ph = per_slice_case(D, herm)
        want = per_slice_want(D, herm)[1]

        def loss(H):
            U = np.eye(D, dtype=complex)
            for n in range(N):
                U = o.expm(-1j * dt * H[n]) @ U
            return np.real(np.vdot(Ubar[1], np.exp(1j * ph[1])[:, None] * U))

        for _ in range(2):
            dH = rng.normal(size=Hs[1].shape) + 1j * rng.normal(size=Hs[1].shape)
            fd = (loss(Hs[1] + 1e-6 * dH) - loss(Hs[1] - 1e-6 * dH)) / 2e-6
            assert abs(fd - np.real(np.sum(np.conj(want) * dH))) < 1e-8 * max(1.0, abs(fd))
    for D in GOAL:
        h0, hks, sig, dt, q, ph = goal_case(D)
        dims, index = GOAL[D]
        loss = lambda s: o.unitary_infid(q, o.propagate_batch(h0, hks, s[None], dt, fr_phase=ph[:1])[0], index=index, dims=dims)
        _fd_check(goal_want(D)[1][0], loss, sig[0], rng, 1e-5)


def test_bounds_of_the_inputs_land_where_intended():
    """case 1 / 2: every segment of every S has its column-wise bound in (0.55 target, target]; case 4: the strong wave is beyond
    the real sweep's limit and within the general sweep's five squarings, all other waves far below; with S = 8 only the second of
    sample 0's two waves leaves, with S = 4 the whole of sample 0; per sample, the complex sample 1 leaves as a whole"""
    for D, kind, target, ps in [(9, "real", 0.6, False), (12, "real", 1.5, False), (4, "real", 5.0, False), (5, "complex", 4.0, False), (8, "real", 1.5, True)]:
        h0, hks, sig, dt, _, _ = unitary_case(D, kind, target, ps)
        for S in S_PER_SAMPLE if ps else S_SHARED:
            cols = [col_bound(h0, hks, sig, dt, b, n0, n1) for b in range(B) for n0, n1 in segments(N, S, per_mille=500)]
            assert 0.55 * target < min(cols) and max(cols) <= target * (1 + 1e-12), (D, kind, target, S)
        assert abs(max(col_bound(h0, hks, sig, dt, b) for b in range(B)) - target) < 1e-12 * target
    lens = lambda S: sorted({n1 - n0 for n0, n1 in segments(N, S, per_mille=500)})
    assert [lens(S) for S in S_SHARED] == [[67], [33, 34], [22, 23], [16, 17], [13, 14], [8, 9], [1]]
    for ps in (False, True):
        for S in (4, 8):
            waves = handover_waves(ps, S)
            strong = [w for w in waves if w[3] > REAL_LIMIT]
            assert len(strong) == 1 and strong[0][0] == 0 and strong[0][1] <= 33 < strong[0][2]
            assert abs(strong[0][3] - 16.5) < 1e-9 and strong[0][4] <= GENERAL_LIMIT
            assert all(w[3] <= 1.5 * (1 + 1e-12) for w in waves if w is not strong[0])
            mask = handed_over(ps, S)
            want0 = np.zeros(N, dtype=bool)
            want0[strong[0][1] : strong[0][2]] = True
            assert np.array_equal(mask[0], want0) and (S == 4) == bool(mask[0].all())
            assert bool(mask[1].all()) == ps and bool(mask[1].any()) == ps and not mask[2].any()
