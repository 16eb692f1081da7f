"""CPU tests of the extended-precision references (tests/extended_ref.py) and of their checkers.

* the long-double `expm_ld` / `chain_ld` against 40-digit mpmath;
* scipy's and the oracle's double-precision `expm` through `check_expm` over the case list of the GPU test: their worst
  ratios per class are the recorded `R_CPU_EXPM`, and must stay within them;
* the oracle's folds through `check_chain` over the chain case list;
* the long-double gradient references (`pwc_signal_gradient_ld`, `pwc_per_slice_cotangents_ld`) against a forward-mode 40-digit
  mpmath gradient and against central differences in long double;
* sensitivity: every checker passes on a double-precision result and FAILS on a subtly wrong one -- the proof that the
  GPU tests (tests/test_gpu_matrix_routines.py, tests/test_gpu_fidelity_epilogue.py) would notice a wrong kernel.
"""
import numpy as np
import pytest
import scipy.linalg

import extended_ref as x
from oracle import c3_oracle as o


# --------------------------------------------------------------------------
# the references against 40-digit arithmetic
# --------------------------------------------------------------------------


def _mp_matrix(mp, A):
    return mp.matrix([[mp.mpc(complex(v).real, complex(v).imag) for v in row] for row in np.asarray(A)])


def _ld_to_mp(mp, v):
    """A long double exactly as an mpf: its double part plus the remainder (both doubles)."""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))


def _max_diff_mp(mp, E_ld, M):
    D = E_ld.shape[0]
    worst = mp.mpf(0)
    for i in range(D):
        for j in range(D):
            z = mp.mpc(_ld_to_mp(mp, E_ld[i, j].real), _ld_to_mp(mp, E_ld[i, j].imag))
            worst = max(worst, abs(z - M[i, j]))
    return float(worst)


# norms of the GPU test (extended_ref.NORMS_*): the whole list where 40-digit arithmetic is cheap
MP_CASES = [(1, x.NORMS_FULL), (2, x.NORMS_FULL), (5, x.NORMS_SHORT), (8, x.NORMS_FEW + (40.0,)), (12, x.NORMS_FEW + (40.0,))]


@pytest.mark.parametrize("D,norms", MP_CASES, ids=[f"D{d}" for d, _ in MP_CASES])
def test_expm_ld_against_mpmath(D, norms):
    """|expm_ld - mpmath.expm| <= 4 eps_ld max(1, ||A||_1) ||E||_max: general (non-normal) matrices over the norm list,
    and the large-trace kinds (50i 1 + X, -4 1 + X) and a nilpotent one."""
    mp = pytest.importorskip("mpmath")
    rng = np.random.default_rng(D)
    mats = [x.expm_matrix("general", D, nrm, rng) for nrm in norms]
    mats += [x.expm_matrix(kind, D, 1.0, rng) for kind in ("phase50", "shift_m4", "nilpotent", "skewherm")]
    worst = 0.0
    with mp.workdps(40):
        for A in mats:
            E = x.expm_ld(A)
            M = mp.expm(_mp_matrix(mp, A))
            ref_max = max(abs(complex(M[i, j])) for i in range(D) for j in range(D))
            r = _max_diff_mp(mp, E, M) / (x.EPS_LD * max(1.0, x.norm1(A)) * ref_max)
            worst = max(worst, r)
    print(f"expm_ld vs mpmath D={D}: worst error / (eps_ld max(1,||A||) ||E||max) = {worst:.3g}")
    assert worst <= 4.0


@pytest.mark.parametrize("D", [1, 2, 5, 8, 12])
@pytest.mark.parametrize("right", [False, True])
def test_chain_ld_against_mpmath(D, right):
    """||chain_ld - exact||_F <= 4 eps_ld (N - 1) D sqrt(D) prod ||M_k||_2: every rounded product adds at most
    gamma_D (complex: x 2 sqrt 2) ||running product||_F ||M_k||_2, and ||running product||_F <= sqrt(D) prod ||M_k||_2."""
    mp = pytest.importorskip("mpmath")
    N = 9
    M = x.chain_inputs(D, N, 1).M[0]
    with mp.workdps(40):
        acc = _mp_matrix(mp, M[0] if right else M[-1])
        for k in (range(1, N) if right else range(N - 2, -1, -1)):
            acc = acc * _mp_matrix(mp, M[k])
        P = x.chain_ld(M, right=right)
        err = float(mp.sqrt(sum(abs(mp.mpc(_ld_to_mp(mp, P[i, j].real), _ld_to_mp(mp, P[i, j].imag)) - acc[i, j]) ** 2 for i in range(D) for j in range(D))))
    bar = 4 * x.EPS_LD * (N - 1) * D * np.sqrt(D) * float(np.prod([np.linalg.norm(m, 2) for m in M]))
    print(f"chain_ld vs mpmath D={D} right={right}: {err:.3g} (bar {bar:.3g})")
    assert err <= bar


def test_kron_overlap_infid_ld_against_mpmath():
    """The element-wise references on one small case each (they are single formulas)."""
    mp = pytest.importorskip("mpmath")
    rng = np.random.default_rng(3)
    A, B = rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2)), rng.normal(size=(3, 3)) + 1j * rng.normal(size=(3, 3))
    K = x.kron_ld(A, B)
    with mp.workdps(40):
        for (i, p, j, q) in [(0, 1, 1, 2), (1, 2, 0, 0)]:
            z = mp.mpc(A[i, j].real, A[i, j].imag) * mp.mpc(B[p, q].real, B[p, q].imag)
            got = K[i * 3 + p, j * 3 + q]
            assert abs(mp.mpc(_ld_to_mp(mp, got.real), _ld_to_mp(mp, got.imag)) - z) <= 4 * x.EPS_LD * abs(z)
        Umat = rng.normal(size=(5, 5)) + 1j * rng.normal(size=(5, 5))
        G = rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2))
        rows = [3, 1]
        s, T = x.overlap_ld(Umat, rows, G)
        z = sum(mp.mpc(Umat[rows[a], rows[c]].real, Umat[rows[a], rows[c]].imag) * mp.mpc(G[a, c].real, -G[a, c].imag) for a in range(2) for c in range(2))
        assert abs(mp.mpc(_ld_to_mp(mp, s.real), _ld_to_mp(mp, s.imag)) - z) <= 8 * x.EPS_LD * float(T)
        f = x.infid_ld(s, 2, "unitary")
        assert abs(_ld_to_mp(mp, f) - (1 - abs(z) ** 2 / 4)) <= 8 * x.EPS_LD * (1 + float(abs(z)) ** 2)
        f = x.infid_ld(s, 2, "average")
        assert abs(_ld_to_mp(mp, f) - (1 - (abs(z) ** 2 / 2 + 1) / 3)) <= 8 * x.EPS_LD * (1 + float(abs(z)) ** 2)


# --------------------------------------------------------------------------
# the CPU double-precision routines through the checkers
# --------------------------------------------------------------------------

RANGES = ("D<=2", "D3-12", "D13-40", "D>=41")


@pytest.mark.parametrize("rng_name", RANGES)
def test_cpu_expm_ratios_within_recorded_constants(rng_name):
    """scipy.linalg.expm and the oracle's expm over the case list of the GPU test: the worst ratio per class IS the
    recorded R_CPU_EXPM (printed here in the form it is recorded in), and must not exceed it."""
    measured = {}
    for c in x.expm_cases():
        if x.dim_range(c.D) != rng_name:
            continue
        A, E = x.expm_inputs(c)
        Es = np.stack([scipy.linalg.expm(a) for a in A])
        Eo = o.expm(A)
        for i in range(A.shape[0]):
            k = x.expm_class(c, A[i])
            r = max(x.expm_ratio(Es[i], A[i], E[i]), x.expm_ratio(Eo[i], A[i], E[i]))
            measured[k] = max(measured.get(k, 0.0), r)
    for k in sorted(measured):
        print(f"    {k!r}: measured {measured[k]:.4g}, recorded {x.R_CPU_EXPM.get(k)}")
    assert set(measured) == {k for k in x.R_CPU_EXPM if k[0] == rng_name}
    for k, r in measured.items():
        assert r <= x.R_CPU_EXPM[k], (k, r)


@pytest.mark.parametrize("D", x.CHAIN_DIMS)
def test_cpu_chain_through_checker(D):
    """The oracle's folds through `check_chain` over the chain case list: the left and right folds define e_cpu (ratio 1 at
    the worst sample); the pairwise tree tf_matmul_n, another order of association, obeys the same bar."""
    for N in x.chain_lengths(D):
        for B in x.chain_batches(D, N):
            ref = x.chain_inputs(D, N, B)
            left = np.stack([o.tf_matmul_left(ref.M[b]) for b in range(B)])
            right = np.stack([o.tf_matmul_right(ref.M[b]) for b in range(B)])
            tree = np.stack([o.tf_matmul_n(ref.M[b]) for b in range(B)])
            assert x.check_chain(left, ref.left, ref.e_left) <= 1.0
            assert x.check_chain(right, ref.right, ref.e_right) <= 1.0
            r = x.check_chain(tree, ref.left, ref.e_left)
            if N == 1:
                assert ref.e_left == 0.0 and ref.e_right == 0.0 and r == 0.0  # one factor: returned bit for bit
    print(f"D={D}: oracle folds within their own bar at N = {x.chain_lengths(D)}")


# --------------------------------------------------------------------------
# sensitivity of the checkers
# --------------------------------------------------------------------------


def _fails(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


@pytest.mark.parametrize("D,kind", [(9, "general"), (9, "skewherm"), (27, "general"), (41, "skewherm")])
def test_check_expm_sensitivity(D, kind):
    rng = np.random.default_rng(D)
    A = x.expm_matrix(kind, D, 1.0, rng)
    E_ref = x.expm_ld(A)
    c = x.ExpmCase(D, kind, (1.0,), 1, False)
    bar = x.expm_bar(c, A)
    E = scipy.linalg.expm(A)
    assert x.check_expm(E, A, E_ref, bar) <= x.R_CPU_EXPM[x.expm_class(c, A)]
    _fails(x.check_expm, E * (1 + 1e-13), A, E_ref, bar)
    _fails(x.check_expm, np.linalg.matrix_power(scipy.linalg.expm(A / 4), 2), A, E_ref, bar)  # one squaring too few
    _fails(x.check_expm, E * np.exp(1e-13j), A, E_ref, bar)  # a phase off by 1e-13
    _fails(x.check_expm, E.T, A, E_ref, bar)


@pytest.mark.parametrize("D,N", [(2, 9), (9, 8), (9, 33), (27, 9), (41, 17)])
def test_check_chain_sensitivity(D, N):
    B = 5
    ref = x.chain_inputs(D, N, B)
    M = ref.M
    left = np.stack([o.tf_matmul_left(M[b]) for b in range(B)])
    assert x.check_chain(left, ref.left, ref.e_left) <= 1.0
    _fails(x.check_chain, left * (1 + 1e-13), ref.left, ref.e_left)
    _fails(x.check_chain, left, ref.right, ref.e_right)  # the other order

    def variant(idx):
        return np.stack([o.tf_matmul_left(M[b][idx]) for b in range(B)])

    k = N // 2
    order = list(range(N))
    swapped = order[:k] + [order[k + 1], order[k]] + order[k + 2 :]
    _fails(x.check_chain, variant(swapped), ref.left, ref.e_left)  # two neighbouring factors swapped
    _fails(x.check_chain, variant(order[:k] + order[k + 1 :]), ref.left, ref.e_left)  # one factor dropped
    _fails(x.check_chain, variant(order[: k + 1] + order[k:]), ref.left, ref.e_left)  # one factor duplicated
    _fails(x.check_chain, variant(order[1:]), ref.left, ref.e_left)  # first factor (a segment edge) dropped
    one = left.copy()
    one[B - 1] = left[0]
    _fails(x.check_chain, one, ref.left, ref.e_left)  # a sample written from another sample's chain


def test_check_kron_sensitivity():
    rng = np.random.default_rng(7)
    A = rng.normal(size=(3, 2, 2)) + 1j * rng.normal(size=(3, 2, 2))
    Bm = rng.normal(size=(3, 3, 3)) + 1j * rng.normal(size=(3, 3, 3))
    assert x.check_kron(o.tf_kron(A, Bm), A, Bm) <= 1.0
    _fails(x.check_kron, o.tf_kron(A, Bm) * (1 + 1e-13), A, Bm)
    _fails(x.check_kron, o.tf_kron(Bm, A), A, Bm)  # p / q and i / j swapped
    _fails(x.check_kron, o.tf_kron(A, np.swapaxes(Bm, -1, -2)), A, Bm)
    _fails(x.check_kron, o.tf_kron(A, Bm)[::-1], A, Bm)  # batch index
    # tf_super = A (x) conj(A)
    sup = o.tf_kron(A, np.conj(A))
    assert x.check_kron(sup, A, np.conj(A)) <= 1.0
    assert x.check_kron(o.tf_super(A), A, np.conj(A)) <= 1.0
    _fails(x.check_kron, o.tf_kron(A, A), A, np.conj(A))  # A (x) A
    _fails(x.check_kron, o.tf_kron(A, np.conj(np.swapaxes(A, -1, -2))), A, np.conj(A))  # A (x) A^+
    # spre / spost: bit-exact, zeros included
    assert np.array_equal(x.spre_ref(A), o.tf_spre(A)) and np.array_equal(x.spost_ref(A), o.tf_spost(A))
    assert x.check_exact(x.spre_ref(A), x.spre_ref(A.copy())) == 0
    _fails(x.check_exact, x.spre_ref(A) * (1 + 1e-15), x.spre_ref(A))
    _fails(x.check_exact, x.spre_ref(A) + 1e-300, x.spre_ref(A))
    _fails(x.check_exact, np.where(x.spre_ref(A) == 0, -0.0, x.spre_ref(A)), x.spre_ref(A))  # a zero with the wrong sign
    _fails(x.check_exact, x.spost_ref(np.swapaxes(A, -1, -2)), x.spost_ref(A))
    _fails(x.check_exact, x.spre_ref(A), x.spost_ref(A))


@pytest.mark.parametrize("kind", ["unitary", "average"])
def test_check_overlap_and_infid_sensitivity(kind):
    rng = np.random.default_rng(11)
    D, L, B = 9, 4, 5
    rows = np.array([0, 1, 3, 4])
    Umat = np.stack([x.haar_unitary(rng, D) for _ in range(B)])
    G = x.haar_unitary(rng, L)
    blk = Umat[:, rows[:, None], rows[None, :]]
    s = (blk * np.conj(G)).sum(axis=(-2, -1))
    assert x.check_overlap(s, Umat, rows, G) <= 1.0
    _fails(x.check_overlap, s * (1 + 1e-13), Umat, rows, G)
    _fails(x.check_overlap, np.conj(s), Umat, rows, G)
    wrong = rows.copy()
    wrong[2] = 2  # one row index replaced
    blk_w = Umat[:, wrong[:, None], wrong[None, :]]
    _fails(x.check_overlap, (blk_w * np.conj(G)).sum(axis=(-2, -1)), Umat, rows, G)
    _fails(x.check_overlap, (blk * np.conj(G.T)).sum(axis=(-2, -1)), Umat, rows, G)  # transposed ideal
    _fails(x.check_overlap, (blk * G).sum(axis=(-2, -1)), Umat, rows, G)  # conjugate missing
    _fails(x.check_overlap, s[::-1], Umat, rows, G)  # samples in another order

    def infid(sv):
        return 1 - np.abs(sv / L) ** 2 if kind == "unitary" else 1 - (np.abs(sv) ** 2 / L + 1) / (L + 1)

    f = infid(s)
    assert x.check_infid(f, Umat, rows, G, kind) <= 1.0
    _fails(x.check_infid, f * (1 + 1e-13), Umat, rows, G, kind)
    _fails(x.check_infid, f, Umat, rows, G, "average" if kind == "unitary" else "unitary")
    _fails(x.check_infid, infid((blk_w * np.conj(G)).sum(axis=(-2, -1))), Umat, rows, G, kind)
    nan = f.copy()
    nan[3] = np.nan  # an entry never written
    _fails(x.check_infid, nan, Umat, rows, G, kind)
    assert x.check_infid_sum(f.sum(), Umat, rows, G, kind) <= 1.0
    _fails(x.check_infid_sum, f.sum() * (1 + 1e-13), Umat, rows, G, kind)
    _fails(x.check_infid_sum, f[:-1].sum(), Umat, rows, G, kind)  # one sample missing from the sum
    _fails(x.check_infid_sum, f.sum() + f[0], Umat, rows, G, kind)  # one sample counted twice


def test_check_infid_lindbladian_sensitivity():
    rng = np.random.default_rng(13)
    D, L = 3, 2
    rows = np.array([0, 1])
    srows = (rows[:, None] * D + rows[None, :]).reshape(-1)
    G = x.haar_unitary(rng, L)
    Gs = np.kron(G, np.conj(G))
    Umat = np.stack([x.haar_unitary(rng, D) for _ in range(3)])
    S = o.tf_super(Umat) * 0.999
    t = (S[:, srows[:, None], srows[None, :]] * np.conj(Gs)).sum(axis=(-2, -1))
    f = 1 - np.abs(t) / L**2
    assert x.check_infid(f, S, srows, Gs, "lindbladian", L=L) <= 1.0
    _fails(x.check_infid, f * (1 + 1e-13), S, srows, Gs, "lindbladian", L=L)
    _fails(x.check_infid, 1 - np.abs(t) ** 2 / L**4, S, srows, Gs, "lindbladian", L=L)
    bad = srows.copy()
    bad[1] = rows[0] * D + 2
    tb = (S[:, bad[:, None], bad[None, :]] * np.conj(Gs)).sum(axis=(-2, -1))
    _fails(x.check_infid, 1 - np.abs(tb) / L**2, S, srows, Gs, "lindbladian", L=L)


# --------------------------------------------------------------------------
# the gradient references (pwc_signal_gradient_ld, pwc_per_slice_cotangents_ld)
# --------------------------------------------------------------------------


def _mp_kron(mp, A, B):
    n, m = A.rows, B.rows
    out = mp.matrix(n * m, n * m)
    for i in range(n):
        for j in range(n):
            for p in range(m):
                for q in range(m):
                    out[i * m + p, j * m + q] = A[i, j] * B[p, q]
    return out


def _mp_sup(mp, H, one):
    return mp.mpc(0, -1) * (_mp_kron(mp, H, one) - _mp_kron(mp, one, H.T))


def _mp_signal_gradient(mp, h0, hks, sig, dt, col, ph, Ubar):
    """One sample in 40 digits, FORWARD mode (nothing shared with the adjoint form under test): dU / dc_k(n) = post_n L(X_n; G_k) pre_n
    with L the (0, 1) block of mp.expm([[X, G], [0, X]]); g[k, n] = Re sum conj(Ubar) FR dU.  Returns (g, sum_n ||X_n||_1,
    max_k ||G_k||_F) with g a K x N list of mpf."""
    D = h0.shape[-1]
    K, N = sig.shape
    one = mp.eye(D)
    Hk = [_mp_matrix(mp, hks[k]) for k in range(K)]
    if col is None:
        Gk = [mp.mpc(0, -1) * mp.mpf(dt) * h for h in Hk]
        diss = None
    else:
        Gk = [mp.mpf(dt) * _mp_sup(mp, h, one) for h in Hk]
        diss = mp.zeros(D * D)
        for C in col:
            C = _mp_matrix(mp, C)
            CC = C.H * C
            diss = diss + _mp_kron(mp, C, C.conjugate()) - (_mp_kron(mp, CC, one) + _mp_kron(mp, one, CC.T)) / 2
    Dm = Gk[0].rows
    Xs = []
    for n in range(N):
        H = _mp_matrix(mp, h0)
        for k in range(K):
            H = H + mp.mpf(float(sig[k, n])) * Hk[k]
        Xs.append(mp.mpc(0, -1) * mp.mpf(dt) * H if col is None else mp.mpf(dt) * (_mp_sup(mp, H, one) + diss))
    Es = [mp.expm(X) for X in Xs]
    pre = [mp.eye(Dm)]
    for n in range(N):
        pre.append(Es[n] * pre[-1])
    post = [None] * N
    acc = mp.eye(Dm)
    for n in range(N - 1, -1, -1):
        post[n] = acc
        acc = acc * Es[n]
    rows = [mp.expj(mp.mpf(float(p))) for p in ph] if ph is not None else [mp.mpf(1)] * Dm
    Ub = _mp_matrix(mp, Ubar)
    g = [[None] * N for _ in range(K)]
    for n in range(N):
        for k in range(K):
            blk = mp.zeros(2 * Dm)
            for i in range(Dm):
                for j in range(Dm):
                    blk[i, j] = blk[Dm + i, Dm + j] = Xs[n][i, j]
                    blk[i, Dm + j] = Gk[k][i, j]
            Eb = mp.expm(blk)
            dU = post[n] * Eb[0:Dm, Dm : 2 * Dm] * pre[n]
            g[k][n] = sum(mp.re(mp.conj(Ub[i, j]) * rows[i] * dU[i, j]) for i in range(Dm) for j in range(Dm))
    nsum = sum(max(sum(abs(X[i, j]) for i in range(Dm)) for j in range(Dm)) for X in Xs)
    gmax = max(mp.sqrt(sum(abs(G[i, j]) ** 2 for i in range(Dm) for j in range(Dm))) for G in Gk)
    return g, float(nsum), float(gmax)


def _grad_pin_problem(D, lind, phase, seed=0):
    rng = np.random.default_rng([D, int(lind), int(phase), seed])
    B, K, N = 2, 2, 3
    h0 = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    h0 = (h0 + h0.conj().T) / 2 + 0.7 * np.eye(D)
    hks = rng.normal(size=(K, D, D)) + 1j * rng.normal(size=(K, D, D))  # not Hermitian: nothing is assumed of the operators
    sig = rng.uniform(-1, 1, size=(B, K, N))
    col = 0.3 * (rng.normal(size=(2, D, D)) + 1j * rng.normal(size=(2, D, D))) if lind else None
    Dm = D * D if lind else D
    ph = rng.uniform(0, 6.28, size=(B, Dm)) if phase else None
    Ubar = rng.normal(size=(B, Dm, Dm)) + 1j * rng.normal(size=(B, Dm, Dm))
    return h0, hks, sig, 0.37, col, ph, Ubar


GRAD_PINS = [(D, lind, phase) for D in (2, 3, 4) for lind in (False, True) for phase in (False, True)]


@pytest.mark.parametrize("D,lind,phase", GRAD_PINS, ids=[f"D{d}-{'lindblad' if l else 'unitary'}{'-phase' if p else ''}" for d, l, p in GRAD_PINS])
def test_pwc_signal_gradient_ld_against_mpmath(D, lind, phase):
    """The form of the `pwc_ld` pin with the scale of a gradient entry (|g| <= ||U_bar||_F ||G_k||_F for unitary slices):
    |g_ld - exact| <= 4 eps_ld max(1, sum_n ||X_n||_1) ||U_bar||_F max_k ||G_k||_F.  Measured: at most 0.48 of that bar over these
    twelve cases (D = 4 Lindblad: one sample, 40-digit exponentials of 32 x 32 block matrices are slow)."""
    mp = pytest.importorskip("mpmath")
    h0, hks, sig, dt, col, ph, Ubar = _grad_pin_problem(D, lind, phase)
    g = x.pwc_signal_gradient_ld(h0, hks, sig, dt, Ubar, col_ops=col, fr_phase=ph)
    assert g.dtype == np.longdouble and g.shape == sig.shape
    worst = 0.0
    with mp.workdps(40):
        for b in range(1 if (lind and D == 4) else sig.shape[0]):
            gm, nsum, gmax = _mp_signal_gradient(mp, h0, hks, sig[b], dt, col, None if ph is None else ph[b], Ubar[b])
            diff = max(abs(_ld_to_mp(mp, g[b, k, n]) - gm[k][n]) for k in range(sig.shape[1]) for n in range(sig.shape[2]))
            worst = max(worst, float(diff) / (x.EPS_LD * max(1.0, nsum) * float(np.linalg.norm(Ubar[b])) * gmax))
    print(f"pwc_signal_gradient_ld vs mpmath D={D} lindblad={lind} phase={phase}: worst error / (eps_ld max(1, sum ||X_n||) ||Ubar||_F max ||G_k||_F) = {worst:.3g}")
    assert worst <= 4.0


def test_per_slice_cotangents_ld_are_the_signal_gradient_contracted():
    """Branch B: Re <H_bar_n, h_k> of the per-slice cotangents is the signal gradient of the same problem (two evaluations of the same
    long-double sweep on differently assembled inputs), and the cotangents follow the oracle's convention."""
    h0, hks, sig, dt, _, ph, Ubar = _grad_pin_problem(3, False, True, seed=1)
    hks = (hks + hks.conj().transpose(0, 2, 1)) / 2
    g = x.pwc_signal_gradient_ld(h0, hks, sig, dt, Ubar, fr_phase=ph)
    Hs = np.stack([o.sum_h0_hks(h0, hks, sig[b]) for b in range(sig.shape[0])])
    Hbar = x.pwc_per_slice_cotangents_ld(Hs, dt, Ubar, fr_phase=ph)
    assert Hbar.dtype == np.clongdouble and Hbar.shape == Hs.shape
    gc = np.einsum("bnij,kij->bkn", np.conj(Hbar), x.to_ld(hks)).real
    # (the slice Hamiltonians handed over are the DOUBLE sums h0 + sum_k c_k h_k: the two problems differ by their rounding, u ||H||)
    assert np.abs(gc - g).max() <= 1e-15 * np.abs(g).max()
    for b in range(sig.shape[0]):
        want = o.pwc_per_slice_hamiltonian_cotangents(Hs[b], dt, Ubar[b], ph[b])
        assert np.abs(Hbar[b].astype(np.complex128) - want).max() <= 1e-13 * np.abs(want).max()


def test_pwc_signal_gradient_ld_against_central_differences():
    """One mid-size case (D = 9, N = 12, Lindblad D = 3 likewise): central differences of `pwc_ld`'s steps in long double with
    h = 2^-20 (truncation h^2 |g'''| / 6 ~ 1e-13, rounding eps_ld / h = 1e-13): 1e-10 of the largest entry."""
    for D, lind in ((9, False), (3, True)):
        rng = np.random.default_rng([77, D])
        B, K, N = 1, 2, 12
        herm = lambda s: (lambda m: s * (m + m.conj().T) / 2)(rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D)))
        h0, hks = herm(0.5), np.stack([herm(0.3) for _ in range(K)])
        col = 0.2 * (rng.normal(size=(1, D, D)) + 1j * rng.normal(size=(1, D, D))) if lind else None
        Dm = D * D if lind else D
        sig = rng.uniform(-1, 1, size=(B, K, N))
        ph = rng.uniform(0, 6.28, size=(B, Dm))
        Ubar = rng.normal(size=(B, Dm, Dm)) + 1j * rng.normal(size=(B, Dm, Dm))
        g = x.pwc_signal_gradient_ld(h0, hks, sig, 0.4, Ubar, col_ops=col, fr_phase=ph)
        # the step is a double: s + h and s - h are formed in long double so that the difference is exactly 2 h
        h = np.longdouble(2.0**-20)
        worst = 0.0
        for k, n in ((0, 0), (1, 5), (0, N - 1), (1, 7)):
            e = np.zeros(sig.shape, dtype=np.longdouble)
            e[0, k, n] = h
            fd = (_loss_ld(h0, hks, sig.astype(np.longdouble) + e, 0.4, col, ph, Ubar) - _loss_ld(h0, hks, sig.astype(np.longdouble) - e, 0.4, col, ph, Ubar)) / (2 * h)
            worst = max(worst, float(abs(fd - g[0, k, n]) / np.abs(g[0]).max()))
        print(f"pwc_signal_gradient_ld vs central differences D={D} lindblad={lind}: {worst:.3g}")
        assert worst <= 1e-10


def _loss_ld(h0, hks, sig_ld, dt, col, ph, Ubar):
    """Re sum conj(Ubar) U of `pwc_ld`'s own steps with amplitudes that are long doubles already (`pwc_generators_ld` converts its
    amplitudes from double: a step of 2^-20 on an amplitude of order 1 would be exact there too, but the sum is formed here without
    the detour)."""
    D = h0.shape[-1]
    H = x.to_ld(h0)[None, None] + (sig_ld[:, :, :, None, None] * x.to_ld(hks)[None, :, None]).sum(axis=1)
    if col is None:
        X = np.clongdouble(-1j) * np.longdouble(dt) * H
    else:
        X = np.stack([np.longdouble(dt) * x.lindblad_generator_ld(H[b], col) for b in range(H.shape[0])])
    dUs = x.expm_ld(X)
    U = np.stack([x.chain_ld(dUs[b]) for b in range(X.shape[0])])
    phl = np.asarray(ph).astype(np.longdouble)
    U = (np.cos(phl) + np.clongdouble(1j) * np.sin(phl))[:, :, None] * U
    return (np.conj(x.to_ld(Ubar)) * U).sum().real
