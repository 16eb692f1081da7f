"""Extended-precision references for the matrix routines and the fidelity epilogue (numpy only).

Everything here is computed in x87 long double (64-bit mantissa, eps = 1.08e-19): 2^11 finer than the double
precision of the kernels under test, so an error of a few units of 2^-53 is measured, not guessed.  The module holds

* the references: `expm_ld`, `chain_ld`, `kron_ld`, `overlap_ld`, `infid_ld`, and `pwc_ld` (the assembled piecewise-constant
  propagators of `propagate_batch`, unitary and Lindblad; cases in tests/pwc_cases.py, GPU tests in tests/test_gpu_pwc_extended.py);
  `expm_frechet_ld`, `pwc_signal_gradient_ld`, `pwc_per_slice_cotangents_ld` (the signal gradients of the `*_vjp` entries and the
  Hamiltonian cotangents of branch B; cases in tests/grad_cases.py, GPU tests in tests/test_gpu_grad_extended.py);
* the checkers shared by the CPU tests (tests/test_extended_ref.py) and the GPU tests
  (tests/test_gpu_matrix_routines.py, tests/test_gpu_fidelity_epilogue.py): each asserts its bar and RETURNS the
  ratio it asserted on, so it can be printed and recorded;
* the case lists (inputs are a pure function of the case: the CPU tests that record `R_CPU_EXPM` and the GPU tests see
  the same matrices);
* `R_CPU_EXPM`: the worst ratio of scipy's and the oracle's double-precision `expm` per class, measured by
  tests/test_extended_ref.py::test_cpu_expm_ratios_within_recorded_constants, which also keeps them from rotting.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
EPS_LD = float(np.finfo(LD).eps)
# not a skip: every host this suite runs on is x86-64, where long double is the 80-bit format
assert EPS_LD < 1.1e-19, f"numpy.longdouble is not an extended format here (eps = {EPS_LD})"

U = 2.0**-53  # unit roundoff of the kernels' arithmetic


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------


def to_ld(a):
    """complex128 / float64 -> complex long double (exact)."""
    return np.asarray(a).astype(CLD)


def norm1(A) -> float:
    """Largest column sum of |a_ij| of one matrix."""
    return float(np.abs(np.asarray(A)).sum(axis=-2).max())


def device_norm(A) -> float:
    """The norm the device plans with (hmeta kernels): 1-norm of A - i Im(tr A) / D."""
    A = np.asarray(A, dtype=np.complex128)
    D = A.shape[-1]
    return norm1(A - 1j * (np.trace(A).imag / D) * np.eye(D))


def expm_ld(A):
    """exp(A) of one matrix or a stack [..., D, D]: scaled to ||X||_1 <= 1/8, 25 Taylor terms (remainder 8^-26 / 26! =
    8e-51 relative), squared back; all in complex long double.  Agrees with 40-digit mpmath to a few eps_ld
    (tests/test_extended_ref.py)."""
    A = to_ld(A)
    if A.ndim > 2:
        out = np.empty_like(A)
        flat, oflat = A.reshape((-1,) + A.shape[-2:]), out.reshape((-1,) + A.shape[-2:])
        for i in range(flat.shape[0]):
            oflat[i] = expm_ld(flat[i])
        return out
    D = A.shape[-1]
    nrm = norm1(A)
    s = 0
    while nrm > 0.125 * 2.0**s:
        s += 1
    X = A / LD(2) ** s
    # F = exp(X) - 1, squared back as (1 + F)^2 - 1 = 2F + F^2: the roundings stay relative to ||F|| ~ ||A|| / 2^(s-k), not
    # to the 1 of the diagonal, so the squarings amplify an error of ~eps ||A|| / 2^s to ~eps ||A|| instead of eps to 2^s eps;
    # once F is of order 1 (exp of a large negative number: F -> -1 cancels) the plain squarings E^2 take over
    T = X.copy()
    F = X.copy()
    for k in range(2, 26):
        T = (T @ X) / LD(k)
        F = F + T
    k = 0
    while k < s and norm1(F) < 0.5:
        F = 2 * F + F @ F
        k += 1
    E = F + np.eye(D, dtype=CLD)
    for _ in range(k, s):
        E = E @ E
    return E


def chain_ld(M, right: bool = False):
    """Ordered product of M[N, D, D] in complex long double: M[N-1] ... M[0] (left, tf.foldr), M[0] ... M[N-1] (right)."""
    M = to_ld(M)
    acc = M[0] if right else M[-1]
    idx = range(1, M.shape[0]) if right else range(M.shape[0] - 2, -1, -1)
    for k in idx:
        acc = acc @ M[k]
    return acc


def lindblad_generator_ld(H, col_ops):
    """L(H) = -i (H (x) 1 - 1 (x) H^T) + sum_c [ C (x) conj(C) - (C^+C (x) 1 + 1 (x) (C^+C)^T) / 2 ] of H[..., D, D] in complex
    long double: the row-major vectorisation of `oracle.lindblad_generator` / `lindblad_dissipator` (rho_ij at row i D + j)."""
    H, col = to_ld(H), to_ld(col_ops)
    D = H.shape[-1]
    one = np.eye(D, dtype=CLD)
    clp = np.zeros((D * D, D * D), dtype=CLD)
    for C in col:
        CC = np.conj(C.T) @ C
        clp = clp + kron_ld(C, np.conj(C)) - (kron_ld(CC, one) + kron_ld(one, CC.T)) / LD(2)
    return CLD(-1j) * (kron_ld(H, one) - kron_ld(one, np.swapaxes(H, -1, -2))) + clp


def pwc_generators_ld(h0, hks, signals, dt, *, col_ops=None):
    """X[B, N, Dm, Dm] of the piecewise-constant problem in complex long double: X_n = -i dt H_n, or dt L(H_n) with collapse
    operators; H_n = h0 + sum_k c_k(n) hk, or (hks = signals = None: branch B) the per-slice Hamiltonians h0[N, D, D] /
    [B, N, D, D] themselves.  Operators shared ([D,D], [K,D,D], [C,D,D]) or per sample ([B,..]).  The inputs are doubles:
    their conversion is exact, every operation after it rounds at eps_ld."""
    h0 = to_ld(h0)
    if hks is None or signals is None:
        H = h0 if h0.ndim == 4 else h0[None]
    else:
        sig = np.asarray(signals, dtype=np.float64).astype(LD)
        B, K, N = sig.shape
        hks = to_ld(hks)
        H = np.empty((B, N) + h0.shape[-2:], dtype=CLD)
        for b in range(B):
            hb = h0[b] if h0.ndim == 3 else h0
            kb = hks[b] if hks.ndim == 4 else hks
            H[b] = hb[None]
            for k in range(K):
                H[b] = H[b] + sig[b, k][:, None, None] * kb[k][None]
    if col_ops is None:
        return CLD(-1j) * LD(dt) * H
    col = np.asarray(col_ops)
    return np.stack([LD(dt) * lindblad_generator_ld(H[b], col[b] if col.ndim == 4 else col) for b in range(H.shape[0])])


def pwc_ld(h0, hks, signals, dt, *, col_ops=None, fr_phase=None, want_dUs=False):
    """U[B, Dm, Dm] of `propagate_batch` in complex long double: `expm_ld` of every slice generator (`pwc_generators_ld`),
    `chain_ld` (later slice on the left), then the row phases diag(exp(i fr_phase[b])), fr_phase [B, Dm].  With `want_dUs`
    returns (U, dUs[B, N, Dm, Dm])."""
    X = pwc_generators_ld(h0, hks, signals, dt, col_ops=col_ops)
    dUs = expm_ld(X)
    U = np.stack([chain_ld(dUs[b]) for b in range(X.shape[0])])
    if fr_phase is not None:
        ph = np.asarray(fr_phase, dtype=np.float64).astype(LD)
        assert ph.shape == U.shape[:2], (ph.shape, U.shape)
        U = (np.cos(ph) + CLD(1j) * np.sin(ph))[:, :, None] * U
    return (U, dUs) if want_dUs else U


def expm_frechet_ld(A, E):
    """L(A; E), the Frechet derivative of exp at A in the direction E (one matrix each), in complex long double: the
    (value, derivative) pair of `expm_ld`'s own scheme.  A scaled to ||X||_1 <= 1/8, 25 Taylor terms of both (T_k = T_{k-1} X / k,
    dT_k = (dT_{k-1} X + T_{k-1} Y) / k, Y = E / 2^s), then s squarings of the pair, F = exp - 1 carried as in `expm_ld`:
    (F, L) <- (2 F + F^2, 2 L + F L + L F), then (E, L) <- (E^2, E L + L E).  The derivative is linear in E: the direction is scaled
    to 1-norm 1 and the result scaled back, so that the roundings stay relative to ||L|| whatever the size of the cotangent.  Agrees
    with the (0, 1) block of 40-digit mpmath's exp of [[A, E], [0, A]] to a few eps_ld (tests/test_extended_ref.py)."""
    A, E = to_ld(A), to_ld(E)
    assert A.ndim == 2 and A.shape == E.shape, (A.shape, E.shape)
    D = A.shape[-1]
    ne = norm1(E)
    if ne == 0.0:
        return np.zeros_like(A)
    nrm = norm1(A)
    s = 0
    while nrm > 0.125 * 2.0**s:
        s += 1
    X = A / LD(2) ** s
    Y = E / (LD(ne) * LD(2) ** s)
    T, dT = X.copy(), Y.copy()
    F, L = X.copy(), Y.copy()
    for k in range(2, 26):
        dT = (dT @ X + T @ Y) / LD(k)
        T = (T @ X) / LD(k)
        F = F + T
        L = L + dT
    k = 0
    while k < s and norm1(F) < 0.5:
        L = 2 * L + F @ L + L @ F
        F = 2 * F + F @ F
        k += 1
    Ex = F + np.eye(D, dtype=CLD)
    for _ in range(k, s):
        L = Ex @ L + L @ Ex
        Ex = Ex @ Ex
    return L * LD(ne)


def _adjoint_sweep_ld(X, dUs, lam):
    """Z[N, Dm, Dm] of one sample: Z_n = L(X_n^H; W_n), W_n = lam_n P_n^H the cotangent of slice n, P_n = dU_{n-1} ... dU_0 the
    prefix product and lam_n = (dU_{N-1} ... dU_{n+1})^H lam the running adjoint, all in long double.  d loss = Re sum conj(lam) dU
    for U = dU_{N-1} ... dU_0 then gives d loss = sum_n Re <Z_n, dX_n>."""
    N, Dm = X.shape[0], X.shape[-1]
    H = lambda m: np.conj(np.swapaxes(m, -1, -2))
    P = [np.eye(Dm, dtype=CLD)]
    for n in range(N - 1):
        P.append(dUs[n] @ P[-1])
    Z = np.empty_like(X)
    for n in range(N - 1, -1, -1):
        Z[n] = expm_frechet_ld(H(X[n]), lam @ H(P[n]))
        lam = H(dUs[n]) @ lam
    return Z


def _row_phases_adjoint(U_bar, fr_phase):
    """FR^H U_bar[B, Dm, Dm] in long double: the cotangent of the chain product when U = diag(exp(i fr_phase)) x product."""
    lam = to_ld(U_bar)
    if fr_phase is not None:
        ph = np.asarray(fr_phase, dtype=np.float64).astype(LD)
        assert ph.shape == lam.shape[:2], (ph.shape, lam.shape)
        lam = (np.cos(ph) - CLD(1j) * np.sin(ph))[:, :, None] * lam
    return lam


def pwc_signal_gradient_ld(h0, hks, signals, dt, U_bar, *, col_ops=None, fr_phase=None):
    """g[B, K, N] in long double, d loss / d signals of `propagate_batch_vjp` / `propagate_batch_lindblad_vjp` for
    d loss = Re sum conj(U_bar) dU.  Generators and slices are those of `pwc_ld` (`pwc_generators_ld`, `expm_ld`); prefix products
    and the running adjoint in long double; per slice ONE adjoint Frechet derivative Z_n = L(X_n^H; W_n) (`expm_frechet_ld`) and
    g[k, n] = Re <Z_n, G_k>, G_k = -i dt h_k or dt (-i)(h_k (x) 1 - 1 (x) h_k^T) with collapse operators.  Operators shared or per
    sample, row phases as in `pwc_ld`."""
    X = pwc_generators_ld(h0, hks, signals, dt, col_ops=col_ops)
    dUs = expm_ld(X)
    B, N = X.shape[:2]
    K = np.asarray(signals).shape[1]
    lam = _row_phases_adjoint(U_bar, fr_phase)
    hks = to_ld(hks)
    g = np.zeros((B, K, N), dtype=LD)
    for b in range(B):
        kb = hks[b] if hks.ndim == 4 else hks
        if col_ops is None:
            Gk = CLD(-1j) * LD(dt) * kb
        else:
            one = np.eye(kb.shape[-1], dtype=CLD)
            Gk = CLD(-1j) * LD(dt) * (kron_ld(kb, one) - kron_ld(one, np.swapaxes(kb, -1, -2)))
        Z = _adjoint_sweep_ld(X[b], dUs[b], lam[b])
        for k in range(K):
            g[b, k] = (np.conj(Z) * Gk[k][None]).sum(axis=(-2, -1)).real
    return g


def pwc_per_slice_cotangents_ld(hs, dt, U_bar, *, fr_phase=None):
    """H_bar[B, N, D, D] in complex long double of branch B (`propagate_per_slice_vjp`, `oracle.pwc_per_slice_hamiltonian_cotangents`):
    d loss = Re sum conj(H_bar) dH for d loss = Re sum conj(U_bar) dU; the slice generator is -i dt H_n, so H_bar_n = i dt Z_n."""
    hs = to_ld(hs)
    X = pwc_generators_ld(hs if hs.ndim == 4 else hs[None], None, None, dt)
    dUs = expm_ld(X)
    lam = _row_phases_adjoint(np.asarray(U_bar).reshape((X.shape[0],) + X.shape[-2:]), fr_phase)
    return np.stack([CLD(1j) * LD(dt) * _adjoint_sweep_ld(X[b], dUs[b], lam[b]) for b in range(X.shape[0])])


def grad_err(g, ref) -> float:
    """Worst max|g_b - ref_b| / max|ref_b| over the samples (first axis), in long double."""
    g = np.asarray(g)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    assert np.all(np.isfinite(g)), "non-finite gradient"
    return max(float(np.abs(g[b].astype(ref.dtype) - ref[b]).max() / np.abs(ref[b]).max()) for b in range(ref.shape[0]))


def check_grad(g, ref, e_cpu: float, factor: float = None) -> float:
    """Every sample of a gradient within factor x e_cpu of the long-double one, e_cpu the worst `grad_err` of the double-precision
    CPU routes.  Returns the ratio."""
    factor = CHAIN_FACTOR if factor is None else factor
    e = grad_err(g, ref)
    ratio = 0.0 if e == 0.0 else (np.inf if e_cpu == 0.0 else e / e_cpu)
    assert ratio <= factor, f"gradient error {e:.3g} is {ratio:.3g} x the double-precision routes' {e_cpu:.3g} (bar {factor:g})"
    return ratio


def kron_ld(A, B):
    """Batched Kronecker product out[.., i Db + p, j Db + q] = A[.., i, j] B[.., p, q] in complex long double."""
    A, B = to_ld(A), to_ld(B)
    r = A[..., :, None, :, None] * B[..., None, :, None, :]
    return r.reshape(r.shape[:-4] + (A.shape[-2] * B.shape[-2], A.shape[-1] * B.shape[-1]))


def overlap_ld(Umat, rows, G):
    """(s, T): s = tr(P^T U P G^+) = sum_ac U[rows[a], rows[c]] conj(G[a, c]) for one U or a stack, in complex long double,
    and T = sum |U_ac| |G_ac|, the scale of its rounding-error bound."""
    rows = np.asarray(rows, dtype=np.int64)
    blk = to_ld(Umat)[..., rows[:, None], rows[None, :]]
    G = to_ld(G)
    s = (blk * np.conj(G)).sum(axis=(-2, -1))
    T = (np.abs(blk) * np.abs(G)).sum(axis=(-2, -1))
    return s, T


def infid_ld(s, L: int, kind: str):
    """The goal value of an overlap in long double: unitary 1 - |s / L|^2, average 1 - (|s|^2 / L + 1) / (L + 1),
    lindbladian 1 - |t| / L^2 (t the overlap of the projected superoperators)."""
    s2 = np.abs(s) ** 2
    L = LD(L)
    if kind == "unitary":
        return 1 - s2 / (L * L)
    if kind == "average":
        return 1 - (s2 / L + 1) / (L + 1)
    if kind == "lindbladian":
        return 1 - np.abs(s) / (L * L)
    raise ValueError(kind)


# --------------------------------------------------------------------------
# checkers: assert, and return the ratio asserted on
# --------------------------------------------------------------------------


def _maxabs(x) -> float:
    return float(np.abs(x).max()) if np.size(x) else 0.0


def expm_ratio(E, A, E_ref) -> float:
    """r = ||E - E_ref||_max / (u max(1, ||A||_1) ||E_ref||_max) of one matrix."""
    assert np.all(np.isfinite(np.asarray(E))), "non-finite exponential"
    return _maxabs(to_ld(E) - E_ref) / (U * max(1.0, norm1(A)) * _maxabs(E_ref))


def check_expm(E, A, E_ref, bar: float) -> float:
    """Worst `expm_ratio` over a stack (or of one matrix); asserts it is within `bar`."""
    E, A = np.asarray(E), np.asarray(A)
    assert E.shape == A.shape == E_ref.shape, (E.shape, A.shape, E_ref.shape)
    if A.ndim == 2:
        E, A, E_ref = E[None], A[None], E_ref[None]
    rs = [expm_ratio(E[i], A[i], E_ref[i]) for i in range(A.shape[0])]
    worst = max(rs) if rs else 0.0
    assert worst <= bar, f"expm error ratio {worst:.3g} (matrix {int(np.argmax(rs))} of {len(rs)}) exceeds {bar:.3g}"
    return worst


def unitarity_ratio(E, A) -> float:
    """||E^+ E - 1||_max / (u max(1, ||A||_1)) -- for skew-Hermitian generators, held to the bar of the error itself."""
    E = to_ld(E)
    D = E.shape[-1]
    return _maxabs(np.conj(np.swapaxes(E, -1, -2)) @ E - np.eye(D, dtype=CLD)) / (U * max(1.0, norm1(A)))


def chain_err(P, ref) -> float:
    """||P - ref||_F of one product, in long double."""
    assert np.all(np.isfinite(np.asarray(P))), "non-finite product"
    d = to_ld(P) - ref
    return float(np.sqrt((np.abs(d) ** 2).sum()))


CHAIN_FACTOR = 8.0
EXPM_SLICE_FACTOR = 8.0  # (= EXPM_FACTOR: the 8 R_CPU of the expm bars, per slice)


def check_chain(P, ref, e_cpu: float, factor: float = CHAIN_FACTOR) -> float:
    """Every sample of P[B, D, D] (or one product) must stay within factor x e_cpu of the long-double product, e_cpu the
    error of the double-precision fold (maximum over the samples).  Returns worst error / e_cpu (0 / 0 = 0: bit-exact
    where the double fold is)."""
    P = np.asarray(P)
    assert P.shape == ref.shape, (P.shape, ref.shape)
    if P.ndim == 2:
        P, ref = P[None], ref[None]
    e = max(chain_err(P[b], ref[b]) for b in range(P.shape[0]))
    ratio = 0.0 if e == 0.0 else (np.inf if e_cpu == 0.0 else e / e_cpu)
    assert ratio <= factor, f"chain error {e:.3g} is {ratio:.3g} x the double-precision fold's {e_cpu:.3g} (bar {factor:g})"
    return ratio


def pwc_err(U, ref) -> float:
    """Worst ||U_b - ref_b||_F over the samples of one propagator stack, in long double."""
    U = np.asarray(U)
    assert U.shape == ref.shape, (U.shape, ref.shape)
    return max(chain_err(U[b], ref[b]) for b in range(U.shape[0]))


def check_pwc(U, ref, e_cpu: float, factor: float = CHAIN_FACTOR) -> float:
    """Every sample of the assembled propagators U[B, Dm, Dm] must stay within factor x e_cpu of `pwc_ld`'s, e_cpu the worst
    error over the samples of the double-precision CPU routes.  Returns worst error / e_cpu."""
    U = np.asarray(U)
    assert U.ndim == 3 and U.dtype == np.complex128, (U.shape, U.dtype)
    return check_chain(U, ref, e_cpu, factor)


def slices_ratio(dUs, X, dUs_ref) -> float:
    """Worst `expm_ratio` over the slice propagators dUs[B, N, Dm, Dm] of generators X (long double) against `expm_ld`'s."""
    dUs = np.asarray(dUs)
    assert dUs.shape == X.shape == dUs_ref.shape, (dUs.shape, X.shape, dUs_ref.shape)
    return max(expm_ratio(dUs[b, n], X[b, n], dUs_ref[b, n]) for b in range(X.shape[0]) for n in range(X.shape[1]))


def check_pwc_slices(dUs, X, dUs_ref, r_cpu: float, factor: float = EXPM_SLICE_FACTOR) -> float:
    """The `dUs` route: every slice's `expm_ratio` within factor x r_cpu, r_cpu the worst ratio of scipy and the oracle over
    the same slices.  Returns worst ratio / r_cpu."""
    r = slices_ratio(dUs, X, dUs_ref)
    ratio = 0.0 if r == 0.0 else (np.inf if r_cpu == 0.0 else r / r_cpu)
    assert ratio <= factor, f"slice error ratio {r:.3g} is {ratio:.3g} x the CPU routes' {r_cpu:.3g} (bar {factor:g})"
    return ratio


def check_kron(K, A, B) -> float:
    """Entrywise |K - a b| <= 4 u |a| |b| (one rounded complex product: four products and two sums, each correctly
    rounded, Higham 3.6 gives sqrt(2) gamma_2 < 4u).  Returns the worst |K - ab| / (4 u |a||b|); a zero product must be
    an exact zero."""
    ref = kron_ld(A, B)
    K = np.asarray(K)
    assert K.shape == ref.shape, (K.shape, ref.shape)
    assert np.all(np.isfinite(K)), "non-finite Kronecker product"
    err = np.abs(to_ld(K) - ref)
    scale = 4 * U * np.abs(ref)
    ratio = float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    assert ratio <= 1.0, f"Kronecker entry off by {ratio:.3g} x (4 u |a||b|)"
    return ratio


def check_exact(X, ref) -> float:
    """Bit-for-bit equality with a reference that needs no arithmetic (spre / spost: copies and zeros); returns the
    number of differing entries."""
    X, ref = np.asarray(X), np.asarray(ref, dtype=np.complex128)
    assert X.shape == ref.shape, (X.shape, ref.shape)
    bad = int(np.count_nonzero(X.view(np.uint64) != np.ascontiguousarray(ref).view(np.uint64)))
    assert bad == 0, f"{bad} entries differ bit for bit"
    return float(bad)


def overlap_bar(T, nterms: int):
    """delta_s = 2 (n + 4) u T for a sum of n complex products in ANY order: each product carries 2u-odd (gamma_2 sqrt 2),
    each of at most n - 1 additions u; 2 (n + 4) u covers both with the second-order terms."""
    return 2.0 * (nterms + 4) * U * np.asarray(T, dtype=np.float64)


def infid_bar(s, T, L: int, kind: str):
    """Bar of the goal value from the bar of its overlap: d|s|^2 <= 2|s| delta + delta^2, divided as the formula divides,
    + 4u for the roundings of the epilogue itself (square, divide, add, subtract: four operations on numbers of order 1;
    the non-unitary test inputs keep |s|^2 / L^2 below 2, so that this term holds for them too)."""
    a = np.abs(np.asarray(s)).astype(np.float64)
    if kind == "lindbladian":
        return overlap_bar(T, L**4) / L**2 + 4 * U
    d = overlap_bar(T, L * L)
    den = L * L if kind == "unitary" else L * (L + 1)
    return (2 * a * d + d * d) / den + 4 * U


def check_overlap(s_hat, Umat, rows, G) -> float:
    """|s_hat - s| <= delta_s for every sample; returns the worst |s_hat - s| / delta_s."""
    s, T = overlap_ld(Umat, rows, G)
    L = len(rows)
    s_hat = np.asarray(s_hat)
    assert s_hat.shape == np.shape(s), (s_hat.shape, np.shape(s))
    assert np.all(np.isfinite(s_hat)), "non-finite overlap"
    err = np.abs(to_ld(s_hat) - s).astype(np.float64)
    bar = overlap_bar(T, L * L)
    # (T = 0, a block of zeros: the sum must be an exact zero)
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    assert ratio <= 1.0, f"overlap off by {ratio:.3g} x delta_s"
    return ratio


def check_infid(f_hat, Umat, rows, G, kind: str, L: int = None) -> float:
    """|f_hat - f| <= bar for every sample; returns the worst ratio.  kind "lindbladian": Umat is a stack of
    superoperators, rows the L^2 pair rows, G = ideal (x) conj(ideal), and `L` the size of the ideal gate."""
    s, T = overlap_ld(Umat, rows, G)
    if L is None:
        L = len(rows)
    f = infid_ld(s, L, kind)
    f_hat = np.asarray(f_hat)
    assert f_hat.shape == np.shape(f), (f_hat.shape, np.shape(f))
    assert np.all(np.isfinite(f_hat)), "non-finite infidelity (an entry never written?)"
    err = np.abs(f_hat.astype(LD) - f).astype(np.float64)
    bar = infid_bar(s, T, L, kind)
    ratio = float(np.max(err / bar)) if err.size else 0.0
    assert ratio <= 1.0, f"{kind} infidelity off by {ratio:.3g} x its bar"
    return ratio


def check_infid_sum(sum_hat, Umat, rows, G, kind: str) -> float:
    """|sum_hat - sum_b f_b| <= sum_b bar_b + B u sum_b |f_b| (any summation order); returns the ratio."""
    s, T = overlap_ld(Umat, rows, G)
    L = len(rows)
    f = np.atleast_1d(infid_ld(s, L, kind))
    B = f.shape[0]
    bar = float(np.sum(infid_bar(s, T, L, kind))) + B * U * float(np.abs(f).sum())
    err = float(abs(LD(float(sum_hat)) - f.sum()))
    assert np.isfinite(float(sum_hat))
    ratio = err / bar
    assert ratio <= 1.0, f"{kind} infidelity sum off by {ratio:.3g} x its bar"
    return ratio


# --------------------------------------------------------------------------
# expm cases
# --------------------------------------------------------------------------

# the radii of c3_amd/csrc/c3p_common.h: theta_m of the Paterson-Stockmeyer plans (generic kernel; q = 4 plans of the
# matrix-core kernels), C3P_T18_THETA, C3P_E4N_THETA, C3P_T18N_THETA
PS_THETA = (2.58e-8, 3.40e-4, 9.07e-3, 8.96e-2, 3.00e-1, 7.81e-1, 1.44)
Q4_THETA = (4.0e-4, 5.45e-2, 3.18e-1, 8.16e-1, 1.49)
RADII = PS_THETA + Q4_THETA + (1.13, 1.35, 2.0)
EDGE = 1e-3  # "just below / just above": far outside the rounding of the norm itself, well inside every plan's band


def _edges(radii, mults=(1, 2, 4)):
    return tuple(r * m * side for r in radii for m in mults for side in (1 - EDGE, 1 + EDGE))


NORMS_FULL = (0.0, 1e-9, 0.01) + _edges(RADII) + (6.0, 40.0)
# the larger dimensions (a long-double exponential costs D^3): the radii of the polynomial every kernel takes above
# norm 1 (T18 and its economised variants) at zero, one and two squarings, and the ends
NORMS_SHORT = (0.0, 1e-9, 0.01) + _edges((1.13, 2.0), (1,)) + _edges((1.13,), (2, 4)) + (6.0, 40.0)
NORMS_FEW = (0.01, 1.13 * (1 + EDGE), 6.0)

KINDS = ("general", "skewherm", "realskew", "nilpotent", "diagonal", "shift_m4", "phase50", "nearherm_1e-13", "nearherm_1e-15")

ExpmCase = namedtuple("ExpmCase", "D kind norms chunk force_generic")


def _tile(norms, n):
    """n norms from the list (repeated in turn if n is larger), ASCENDING: the matrix-core kernels take the plan of a wave
    from the largest norm among the (up to four) matrices that share it, so neighbours in a batch should be of like norm
    for a case to reach the plan of its own norm; `EXPM_MIXED_CASES` is the opposite arrangement."""
    return tuple(sorted(norms[i % len(norms)] for i in range(n)))


def expm_cases():
    """The (D, kind) list of the GPU expm test; `norms` holds one entry per matrix, `chunk` is the batch size n of one
    device call (the matrices of a case are handed over `chunk` at a time: n = 260 / 7 / 1 at D <= 12, n = 3 and a last
    call of n = 1 above)."""
    cases = []
    for D in (1, 2, 3, 9, 12):
        for kind in ("general", "skewherm"):
            cases.append(ExpmCase(D, kind, _tile(NORMS_FULL, 260), 260, False))
        for kind in KINDS[2:]:
            cases.append(ExpmCase(D, kind, (1.0,) * 7 if kind == "phase50" else _tile(NORMS_SHORT[1:] + (0.5,), 7), 7, False))
        cases.append(ExpmCase(D, "general", (1.0,), 1, False))
    for D in (13, 16, 17):
        for kind in ("general", "skewherm"):
            cases.append(ExpmCase(D, kind, _tile(NORMS_FULL, 97), 3, False))
        for kind in KINDS[2:]:
            cases.append(ExpmCase(D, kind, (1.0,) * 4 if kind == "phase50" else _tile(NORMS_FEW, 4), 3, False))
    for D in (27, 32, 33, 40, 41):
        for kind in ("general", "skewherm"):
            cases.append(ExpmCase(D, kind, _tile(NORMS_SHORT, 13), 3, False))
        for kind in KINDS[2:]:
            cases.append(ExpmCase(D, kind, (1.0,) if kind == "phase50" else NORMS_FEW[1:2], 1, False))
    for D in (64, 65):
        cases.append(ExpmCase(D, "general", _tile(NORMS_FEW + (40.0,), 4), 3, False))
        cases.append(ExpmCase(D, "skewherm", NORMS_FEW[1:], 3, False))
    cases.append(ExpmCase(128, "general", (2.5,), 1, False))
    cases.append(ExpmCase(256, "general", (2.5,), 1, False))
    # the generic kernel at the dimensions of the other two, across its LDS / global scratch boundary (37 | 38)
    cases.append(ExpmCase(9, "general", _tile(NORMS_FULL, 97), 3, True))
    cases.append(ExpmCase(9, "skewherm", _tile(NORMS_SHORT, 7), 7, True))
    for D in (27, 37, 38):
        cases.append(ExpmCase(D, "general", _tile(NORMS_SHORT, 13), 3, True))
        cases.append(ExpmCase(D, "phase50", (1.0,), 1, True))
    return cases


def case_id(c) -> str:
    return f"D{c.D}-{c.kind}-n{len(c.norms)}x{c.chunk}" + ("-generic" if c.force_generic else "")


def dim_range(D: int) -> str:
    """The dimension range of the kernel that serves D without force_generic.  D <= 2 stands alone: the oracle's Pade quotient
    loses e^|a| digits to cancellation on a (nearly) scalar argument with a large negative real part, and that ratio would
    widen the bar of every dimension of the small-D kernel (D = 1 itself runs the generic kernel)."""
    return "D<=2" if D <= 2 else ("D3-12" if D <= 12 else ("D13-40" if D <= 40 else "D>=41"))


PADE13_THETA = 5.371920351148152


def norm_band(nrm: float) -> str:
    """Part of the class, by the plain 1-norm (what the CPU references plan with): above the radius of Pade-13 the oracle (floor(log2) squaring count of the framework it restates)
    is accurate to ~1e-9 only, and its ratio would widen the bar of every smaller norm of the class."""
    return "n<=5.37" if nrm <= PADE13_THETA else "n>5.37"


def expm_class(c, A):
    """(dimension range, kind, band of ||A||_1) of one matrix A of case c."""
    return (dim_range(c.D), c.kind, norm_band(norm1(A)))


def _rand_c(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _scaled(A, nrm):
    d = device_norm(A)
    return A * (nrm / d) if d > 0 else A * 0.0


def expm_matrix(kind: str, D: int, nrm: float, rng):
    """One generator of `kind` whose device norm (`device_norm`) is `nrm` (shift_m4, phase50: the norm of X)."""
    X = _rand_c(rng, (D, D))
    H = (X + X.conj().T) / 2
    if kind == "general":
        return _scaled(X, nrm)
    if kind == "skewherm":
        return _scaled(-1j * H, nrm)
    if kind == "realskew":
        return _scaled((X.real - X.real.T) + 0j, nrm)
    if kind == "nilpotent":
        return _scaled(np.triu(X, 1), nrm)
    if kind == "diagonal":
        return _scaled(np.diag(np.diag(X)), nrm)
    if kind == "shift_m4":
        return -4.0 * np.eye(D) + _scaled(X, nrm)
    if kind == "phase50":
        return 50j * np.eye(D) + _scaled(X, nrm)
    if kind.startswith("nearherm_"):
        # skew-Hermitian up to a Hermitian defect of relative size eps: on either side of the device's 1e-14 flag
        eps = float(kind.split("_")[1])
        A = -1j * H
        S = _rand_c(rng, (D, D))
        S = S + S.conj().T
        A = A + eps * norm1(A) / norm1(S) * S
        return _scaled(A, nrm)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def expm_inputs(c):
    """(A[n, D, D] complex128, E_ref[n, D, D] complex long double) of a case; computed once per process."""
    seed = [c.D, KINDS.index(c.kind), len(c.norms), int(c.force_generic)]
    rng = np.random.default_rng(seed)
    A = np.stack([expm_matrix(c.kind, c.D, nrm, rng) for nrm in c.norms]).astype(np.complex128)
    A.setflags(write=False)
    E = expm_ld(A)
    E.setflags(write=False)
    return A, E


EXPM_FACTOR = 8.0

# Worst expm_ratio of scipy.linalg.expm and oracle.c3_oracle.expm per class over `expm_cases()`, rounded up to two digits
# (tests/test_extended_ref.py::test_cpu_expm_ratios_within_recorded_constants prints the measured table and asserts it
# stays within these).  The device bar of a class is EXPM_FACTOR x its entry.
R_CPU_EXPM = {
    ('D13-40', 'diagonal', 'n<=5.37'): 3.1,
    ('D13-40', 'diagonal', 'n>5.37'): 16,
    ('D13-40', 'general', 'n<=5.37'): 6.5,
    ('D13-40', 'general', 'n>5.37'): 0.81,
    ('D13-40', 'nearherm_1e-13', 'n<=5.37'): 5.3,
    ('D13-40', 'nearherm_1e-13', 'n>5.37'): 0.78,
    ('D13-40', 'nearherm_1e-15', 'n<=5.37'): 3.8,
    ('D13-40', 'nearherm_1e-15', 'n>5.37'): 0.73,
    ('D13-40', 'nilpotent', 'n<=5.37'): 0.39,
    ('D13-40', 'nilpotent', 'n>5.37'): 0.52,
    ('D13-40', 'phase50', 'n>5.37'): 29,
    ('D13-40', 'realskew', 'n<=5.37'): 4.3,
    ('D13-40', 'realskew', 'n>5.37'): 0.69,
    ('D13-40', 'shift_m4', 'n<=5.37'): 37,
    ('D13-40', 'shift_m4', 'n>5.37'): 11,
    ('D13-40', 'skewherm', 'n<=5.37'): 6.1,
    ('D13-40', 'skewherm', 'n>5.37'): 1.1,
    ('D3-12', 'diagonal', 'n<=5.37'): 3.2,
    ('D3-12', 'general', 'n<=5.37'): 5.9,
    ('D3-12', 'general', 'n>5.37'): 12,
    ('D3-12', 'nearherm_1e-13', 'n<=5.37'): 3.8,
    ('D3-12', 'nearherm_1e-15', 'n<=5.37'): 4.2,
    ('D3-12', 'nilpotent', 'n<=5.37'): 0.9,
    ('D3-12', 'phase50', 'n>5.37'): 30,
    ('D3-12', 'realskew', 'n<=5.37'): 1.9,
    ('D3-12', 'shift_m4', 'n<=5.37'): 47,
    ('D3-12', 'shift_m4', 'n>5.37'): 16,
    ('D3-12', 'skewherm', 'n<=5.37'): 6.0,
    ('D3-12', 'skewherm', 'n>5.37'): 1500,
    ('D<=2', 'diagonal', 'n<=5.37'): 1.9,
    ('D<=2', 'diagonal', 'n>5.37'): 2100,
    ('D<=2', 'general', 'n<=5.37'): 10.0,
    ('D<=2', 'general', 'n>5.37'): 33000000,
    ('D<=2', 'nearherm_1e-13', 'n<=5.37'): 1.5,
    ('D<=2', 'nearherm_1e-13', 'n>5.37'): 1800000,
    ('D<=2', 'nearherm_1e-15', 'n<=5.37'): 1.4,
    ('D<=2', 'nearherm_1e-15', 'n>5.37'): 4100,
    ('D<=2', 'nilpotent', 'n<=5.37'): 1.6,
    ('D<=2', 'phase50', 'n>5.37'): 290,
    ('D<=2', 'realskew', 'n<=5.37'): 1.3,
    ('D<=2', 'shift_m4', 'n<=5.37'): 19,
    ('D<=2', 'shift_m4', 'n>5.37'): 4300000,
    ('D<=2', 'skewherm', 'n<=5.37'): 2.9,
    ('D<=2', 'skewherm', 'n>5.37'): 330000,
    ('D>=41', 'diagonal', 'n<=5.37'): 2.2,
    ('D>=41', 'general', 'n<=5.37'): 6.4,
    ('D>=41', 'general', 'n>5.37'): 0.66,
    ('D>=41', 'nearherm_1e-13', 'n<=5.37'): 4.1,
    ('D>=41', 'nearherm_1e-15', 'n<=5.37'): 4.3,
    ('D>=41', 'nilpotent', 'n<=5.37'): 0.2,
    ('D>=41', 'phase50', 'n>5.37'): 30,
    ('D>=41', 'realskew', 'n<=5.37'): 2.6,
    ('D>=41', 'shift_m4', 'n<=5.37'): 25,
    ('D>=41', 'skewherm', 'n<=5.37'): 5.3,
    ('D>=41', 'skewherm', 'n>5.37'): 0.61,
}


def class_bar(k) -> float:
    """The device bar of a class.  The constant of a (dimension range, kind) is the worst of both bands; the matrices within the
    radius of Pade-13 are held to the constant of their own band, which the oracle's ratios above the radius do not reach."""
    lo = R_CPU_EXPM.get((k[0], k[1], "n<=5.37"), 0.0)
    return EXPM_FACTOR * (lo if k[2] == "n<=5.37" else max(lo, R_CPU_EXPM[k]))


def expm_bar(c, A) -> float:
    return class_bar(expm_class(c, A))


# A matrix of small norm in one wave with one of large norm: it is scaled and squared by the plan of the large one
EXPM_MIXED_CASES = [ExpmCase(D, "general", (1e-9, 40.0, 1e-9, 40.0), 4, False) for D in (3, 9, 12, 16, 41)]


# --------------------------------------------------------------------------
# chain cases
# --------------------------------------------------------------------------

CHAIN_DIMS = (1, 2, 9, 10, 12, 13, 27, 40, 41, 64)
# fold edges of combine_chain (<= 8 in one launch, else ceil(count / 4) segments: 129 -> 33 -> 9 -> 3) ...
CHAIN_N_TABLE = (1, 2, 8, 9, 32, 33, 129)
# ... and of the generic plan (S <= N / 8, groups of 8 until <= 16 remain: N = 136 at B = 1 gives S = 17)
CHAIN_N_GENERIC = (1, 7, 8, 16, 17, 136, 137)


def chain_generic(D: int) -> bool:
    return D < 2 or D > 40


def chain_lengths(D: int):
    return CHAIN_N_GENERIC if chain_generic(D) else CHAIN_N_TABLE


def chain_batches(D: int, N: int):
    """B of a chain case: 1 and 5; the long chains at D = 64 at B = 1 only (their long-double reference costs seconds per
    sample; D = 41 runs the same kernel and plan on both)."""
    return (1,) if D >= 64 and N > 100 else (1, 5)


def haar_unitary(rng, D):
    q, r = np.linalg.qr(_rand_c(rng, (D, D)))
    d = np.diag(r)
    return q * (d / np.abs(d))


ChainRef = namedtuple("ChainRef", "M left right e_left e_right")


@functools.lru_cache(maxsize=None)
def chain_inputs(D: int, N: int, B: int, general: bool = False) -> ChainRef:
    """Factors M[B, N, D, D] (distinct Haar unitaries times (1 + 0.01 g); `general`: N(0,1)/sqrt(D) entries), both ordered
    products in long double, and e_cpu of both orders: the worst error over the samples of the oracle's double fold."""
    from oracle import c3_oracle as o

    rng = np.random.default_rng([D, N, B, int(general)])
    if general:
        M = _rand_c(rng, (B, N, D, D)) / np.sqrt(2.0 * D)
    else:
        M = np.stack([np.stack([haar_unitary(rng, D) * (1 + 0.01 * rng.normal()) for _ in range(N)]) for _ in range(B)])
    M = np.ascontiguousarray(M, dtype=np.complex128)
    M.setflags(write=False)
    left = np.stack([chain_ld(M[b]) for b in range(B)])
    right = np.stack([chain_ld(M[b], right=True) for b in range(B)])
    e_left = max(chain_err(o.tf_matmul_left(M[b]), left[b]) for b in range(B))
    e_right = max(chain_err(o.tf_matmul_right(M[b]), right[b]) for b in range(B))
    for a in (left, right):
        a.setflags(write=False)
    return ChainRef(M, left, right, e_left, e_right)


# --------------------------------------------------------------------------
# plumbing of the GPU tests: both pointer routes, exact references that need no arithmetic
# --------------------------------------------------------------------------

ROUTES = ("host", "device")


def on_route(route: str, a):
    """The argument as the route hands it over: a numpy array (host pointers, staged by the library) or a CUDA tensor
    (device pointers)."""
    if route == "host":
        return np.ascontiguousarray(a)
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def to_np(r):
    return r.detach().cpu().numpy() if hasattr(r, "detach") else np.asarray(r)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(to_np(a)), np.ascontiguousarray(to_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def spre_ref(A):
    """A (x) 1 by copying: out[.., i D + p, j D + p] = A[.., i, j], every other entry +0."""
    A = np.asarray(A, dtype=np.complex128)
    D = A.shape[-1]
    out = np.zeros(A.shape[:-2] + (D, D, D, D), dtype=np.complex128)
    for p in range(D):
        out[..., :, p, :, p] = A
    return out.reshape(A.shape[:-2] + (D * D, D * D))


def spost_ref(A):
    """1 (x) A^T by copying: out[.., i D + p, i D + q] = A[.., q, p]."""
    A = np.asarray(A, dtype=np.complex128)
    D = A.shape[-1]
    out = np.zeros(A.shape[:-2] + (D, D, D, D), dtype=np.complex128)
    for i in range(D):
        out[..., i, :, i, :] = np.swapaxes(A, -1, -2)
    return out.reshape(A.shape[:-2] + (D * D, D * D))
