"""Cotangents of the model operators through the piecewise-constant Lindblad propagator, in numpy (complex128).

For one sample, U = diag(e^{i phase}) E_{N-1} ... E_0 with E_n = exp(X_n), X_n = dt G_n and
G_n = o.lindblad_generator(h0 + sum_k c_k(n) hk, col_ops) (propagation.py:551-585).  For a parameter theta of the operators

    dU/dtheta = diag(e^{i phase}) sum_n post_n L(X_n; dt dG_n/dtheta) pre_n,      L = o.expm_frechet (exact),

with pre_n = E_{n-1} ... E_0 and post_n = E_{N-1} ... E_{n+1}.  The directions are exact as well:
  * an entry of h0 / hks[k]: the generator is complex-linear in the Hamiltonian, dG = o.lindblad_generator(E_ab, 0), times
    c_k(n) for hks[k];
  * an entry of a collapse operator: the dissipator is QUADRATIC in col_ops, so (diss(C + E) - diss(C - E)) / 2 is its exact
    derivative along E; it is not complex-linear, real and imaginary directions are taken separately.
With d loss = Re sum conj(U_bar) dU the cotangent of an entry is (d loss along 1) + i (d loss along i): d loss = Re sum
conj(grad) d(operator), every entry an independent complex number, nothing assumed Hermitian."""
import numpy as np

from oracle import c3_oracle as o


def _slices(h0, hks, col_ops, signals, dt):
    K, N = signals.shape
    Xs = [o.lindblad_generator(h0 + sum(signals[k, n] * hks[k] for k in range(K)), col_ops)[0] * dt for n in range(N)]
    Es = [o.expm(X) for X in Xs]
    Dm = Xs[0].shape[-1]
    pre = [np.eye(Dm, dtype=np.complex128)]
    for n in range(N):
        pre.append(Es[n] @ pre[-1])
    post = [None] * N
    acc = np.eye(Dm, dtype=np.complex128)
    for n in range(N - 1, -1, -1):
        post[n] = acc
        acc = acc @ Es[n]
    return Xs, pre, post


def lindblad_model_cotangents(h0, hks, col_ops, signals, dt, U_bar, fr_phase=None):
    """(grad_h0 [D,D], grad_hks [K,D,D], grad_col_ops [C,D,D]) of one sample: signals [K,N], U_bar [D^2,D^2], fr_phase [D^2]
    row phases or None."""
    h0 = np.asarray(h0, dtype=np.complex128)
    hks = np.asarray(hks, dtype=np.complex128)
    col_ops = np.asarray(col_ops, dtype=np.complex128)
    signals = np.asarray(signals, dtype=np.float64)
    K, N = signals.shape
    C, D = col_ops.shape[0], h0.shape[-1]
    Dm = D * D
    Xs, pre, post = _slices(h0, hks, col_ops, signals, dt)
    ph = np.exp(1j * np.asarray(fr_phase)) if fr_phase is not None else np.ones(Dm)
    Ub = np.asarray(U_bar, dtype=np.complex128)
    dloss = lambda dU: np.sum(np.conj(Ub) * (ph[:, None] * dU))  # complex: its real part is d loss
    zero_col = np.zeros((1, D, D), dtype=np.complex128)

    def unit(a, b, v=1.0):
        E = np.zeros((D, D), dtype=np.complex128)
        E[a, b] = v
        return E

    g0 = np.zeros((D, D), dtype=np.complex128)
    gk = np.zeros((K, D, D), dtype=np.complex128)
    gc = np.zeros((C, D, D), dtype=np.complex128)
    for a in range(D):
        for b in range(D):
            dG = o.lindblad_generator(unit(a, b), zero_col)[0]  # complex-linear in the Hamiltonian
            dU0 = np.zeros((Dm, Dm), dtype=np.complex128)
            dUk = np.zeros((K, Dm, Dm), dtype=np.complex128)
            for n in range(N):
                T = post[n] @ o.expm_frechet(Xs[n], dt * dG) @ pre[n]
                dU0 += T
                for k in range(K):
                    dUk[k] += signals[k, n] * T
            # along 1: Re s, along i: Re(i s) = -Im s
            g0[a, b] = np.conj(dloss(dU0))
            for k in range(K):
                gk[k, a, b] = np.conj(dloss(dUk[k]))
            for c in range(C):
                part = []
                for v in (1.0, 1.0j):
                    cp, cm = col_ops.copy(), col_ops.copy()
                    cp[c, a, b] += v
                    cm[c, a, b] -= v
                    dGc = (o.lindblad_dissipator(cp) - o.lindblad_dissipator(cm)) / 2  # exact: the dissipator is quadratic
                    dU = sum(post[n] @ o.expm_frechet(Xs[n], dt * dGc) @ pre[n] for n in range(N))
                    part.append(np.real(dloss(dU)))
                gc[c, a, b] = part[0] + 1j * part[1]
    return g0, gk, gc


def loss(h0, hks, col_ops, signals, dt, U_bar, fr_phase=None):
    """Re sum conj(U_bar) U of the pinned oracle propagator, the row phases applied to U (for finite differences)."""
    U = o.propagate_batch(h0, hks, np.asarray(signals)[None], dt, col_ops=col_ops, lindbladian=True)[0]
    if fr_phase is not None:
        U = np.exp(1j * np.asarray(fr_phase))[:, None] * U
    return np.real(np.vdot(U_bar, U))
