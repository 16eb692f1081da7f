"""Cotangents of the model operators through the piecewise-constant Lindblad propagator, in numpy (complex128), with ONE Frechet
derivative per slice: fast enough for D = 7, 8, 9 (tests/lindblad_model_grad_ref.py takes one per matrix entry and slice).

For one sample, U = diag(e^{i phase}) E_{N-1} ... E_0, E_n = exp(X_n), X_n = dt G_n, and a direction dG_n of the generators

    d loss = Re sum conj(U_bar) dU = Re sum_n < post_n^+ (e^{-i phase} U_bar) pre_n^+ , L(X_n; dt dG_n) >,     <A, B> = tr(A^+ B).

The adjoint of L(X; .) under that inner product is L(X^+; .)  (L(X)^* = L(X^+), the only identity used), so with

    Z_n = dt L(X_n^+; post_n^+ (e^{-i phase} U_bar) pre_n^+),     W_0 = sum_n Z_n,     W_k = sum_n c_k(n) Z_n,

d loss = Re <W_0, dG> for a direction of the drift generator and Re <W_k, dG> for one of control line k.  Every entry of the
cotangents is then the inner product of W with the SAME oracle directions the slow reference uses: o.lindblad_generator(E_ab, 0)
for the Hamiltonians, the central difference of o.lindblad_dissipator (exact: the dissipator is quadratic) for col_ops."""
import numpy as np

from oracle import c3_oracle as o

from lindblad_model_grad_ref import _slices


def generator_cotangents(h0, hks, col_ops, signals, dt, U_bar, fr_phase=None):
    """W [1 + K, D^2, D^2]: W[0] = sum_n Z_n, W[k] = sum_n c_{k-1}(n) Z_n of one sample."""
    signals = np.asarray(signals, dtype=np.float64)
    K, N = signals.shape
    Xs, pre, post = _slices(h0, hks, col_ops, signals, dt)
    Dm = Xs[0].shape[-1]
    ph = np.exp(1j * np.asarray(fr_phase)) if fr_phase is not None else np.ones(Dm)
    Ub = np.conj(ph)[:, None] * np.asarray(U_bar, dtype=np.complex128)
    W = np.zeros((1 + K, Dm, Dm), dtype=np.complex128)
    for n in range(N):
        Z = dt * o.expm_frechet(Xs[n].conj().T, post[n].conj().T @ Ub @ pre[n].conj().T)
        W[0] += Z
        for k in range(K):
            W[1 + k] += signals[k, n] * Z
    return W


def lindblad_model_cotangents(h0, hks, col_ops, signals, dt, U_bar, fr_phase=None):
    """(grad_h0 [D,D], grad_hks [K,D,D], grad_col_ops [C,D,D]) of one sample, the results of
    lindblad_model_grad_ref.lindblad_model_cotangents: signals [K,N], U_bar [D^2,D^2], fr_phase [D^2] row phases or None."""
    h0 = np.asarray(h0, dtype=np.complex128)
    hks = np.asarray(hks, dtype=np.complex128)
    col_ops = np.asarray(col_ops, dtype=np.complex128)
    K = hks.shape[0]
    C, D = col_ops.shape[0], h0.shape[-1]
    W = generator_cotangents(h0, hks, col_ops, signals, dt, U_bar, fr_phase)
    zero_col = np.zeros((1, D, D), dtype=np.complex128)
    g0 = np.zeros((D, D), dtype=np.complex128)
    gk = np.zeros((K, D, D), dtype=np.complex128)
    gc = np.zeros((C, D, D), dtype=np.complex128)
    for a in range(D):
        for b in range(D):
            E = np.zeros((D, D), dtype=np.complex128)
            E[a, b] = 1.0
            dG = o.lindblad_generator(E, zero_col)[0]  # complex-linear in the Hamiltonian
            # the slow reference: conj(sum conj(U_bar) dU) = conj(<W, dG>)
            g0[a, b] = np.conj(np.vdot(W[0], dG))
            for k in range(K):
                gk[k, a, b] = np.conj(np.vdot(W[1 + k], dG))
            for c in range(C):
                part = []
                for v in (1.0, 1.0j):
                    cp, cm = col_ops.copy(), col_ops.copy()
                    cp[c, a, b] += v
                    cm[c, a, b] -= v
                    dGc = (o.lindblad_dissipator(cp) - o.lindblad_dissipator(cm)) / 2
                    part.append(np.real(np.vdot(W[0], dGc)))
                gc[c, a, b] = part[0] + 1j * part[1]
    return g0, gk, gc


def hermitian_part(g):
    """(g + g^+) / 2 over the last two axes: what a real (Hermiticity-preserving) generator sees of a Hamiltonian cotangent"""
    g = np.asarray(g)
    return (g + np.conj(np.swapaxes(g, -1, -2))) / 2
