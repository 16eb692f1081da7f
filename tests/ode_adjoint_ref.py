"""Discrete adjoint of the oracle's ODE state solvers, in numpy (complex128).

One step is y_{n+1} = y_n + sum_s b_s k_s with k_s = dt F(H(t_{n,s}))[y_n + sum_{j<s} a_sj k_j] and
H(t) = h0 + sum_k c_k(t) hk, c_k the linear interpolation (extrapolation past the last sample) of the signal samples.
Given ybar_{n+1}: kbar_s = b_s ybar_{n+1}, ybar_n = ybar_{n+1}, and for s = S-1 .. 0

    zbar = dt F^+(H)[kbar_s];  cbar_k += Re<kbar_s, dt dF/dc_k[y_s]>;  ybar_n += zbar;  kbar_j += a_sj zbar (j < s)

with adjoints under Re tr(a^+ b) -- nothing is assumed Hermitian.  The rk5 / tsit5 tableaux and stage nodes are the oracle's
data (oracle.c3_oracle.RK5_A ...); rk4 / rk38 are the coefficients of its rk4 / rk38 functions."""
import numpy as np

from oracle import c3_oracle as o

# solver -> (a rows, b, stage nodes as fractions of dt)
TABLEAUX = {
    "rk4": (((), (0.5,), (0.0, 0.5), (0.0, 0.0, 1.0)), (1 / 6, 2 / 6, 2 / 6, 1 / 6), (0.0, 0.5, 0.5, 1.0)),
    "rk38": (((), (1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (1 / 8, 3 / 8, 3 / 8, 1 / 8), (0.0, 1 / 3, 2 / 3, 1.0)),
    "rk5": (o.RK5_A, o.RK5_B, tuple(o.RK5_NODES[i] for i in o.RK5_H)),
    "tsit5": (o.TSIT5_A, o.TSIT5_B, tuple(o.TSIT5_NODES[i] for i in o.TSIT5_H)),
}


def interp_weights(n, node, N):
    """(lo, tau): c = (1 - tau) s[lo] + tau s[lo + 1] at u = n + node; tau in (1, 2] in the last step (extrapolation)."""
    u = n + node
    lo = min(int(np.floor(u)), N - 2)
    return lo, u - lo


def _dag(a):
    return np.conj(np.swapaxes(a, -1, -2))


def _F(step, H, y, col):
    if step == "schrodinger":
        return -1j * (H @ y)
    d = -1j * (H @ y - y @ H)
    if step == "lindblad":
        for c in col:
            g = _dag(c) @ c
            d = d + c @ y @ _dag(c) - 0.5 * (g @ y + y @ g)
    return d


def _Fadj(step, H, x, col):
    Hd = _dag(H)
    if step == "schrodinger":
        return 1j * (Hd @ x)
    d = 1j * (Hd @ x - x @ Hd)
    if step == "lindblad":
        for c in col:
            g = _dag(c) @ c
            d = d + _dag(c) @ x @ c - 0.5 * (g @ x + x @ g)
    return d


def _dF(step, hk, y):
    if step == "schrodinger":
        return -1j * (hk @ y)
    return -1j * (hk @ y - y @ hk)


def forward(h0, hks, sig, dt, y0, solver, step, col=None):
    """Trajectory [N, D, M] (state after every step) of one sample, sig [K, N]."""
    A, Bw, nodes = TABLEAUX[solver]
    K, N = sig.shape
    y = np.asarray(y0, dtype=np.complex128)
    out = []
    for n in range(N):
        ks = []
        for s in range(len(Bw)):
            lo, tau = interp_weights(n, nodes[s], N)
            c = (1 - tau) * sig[:, lo] + tau * sig[:, lo + 1]
            H = h0 + np.tensordot(c, hks, axes=1)
            ys = y + sum((a * k for a, k in zip(A[s], ks) if a != 0.0), 0)
            ks.append(dt * _F(step, H, ys, col))
        y = y + sum(b * k for b, k in zip(Bw, ks))
        out.append(y)
    return np.stack(out)


def vjp(h0, hks, sig, dt, y0, solver, step, ybar, col=None, bar_all=False):
    """(grad_signals [K, N], init_bar [D, M]) of one sample for the cotangent `ybar` of the final state ([D, M]) or, with
    bar_all, of every trajectory state ([N, D, M])."""
    A, Bw, nodes = TABLEAUX[solver]
    K, N = sig.shape
    S = len(Bw)
    h0 = np.asarray(h0, dtype=np.complex128)
    hks = np.asarray(hks, dtype=np.complex128).reshape(K, *h0.shape)
    traj = forward(h0, hks, sig, dt, y0, solver, step, col)
    starts = [np.asarray(y0, dtype=np.complex128)] + list(traj[:-1])
    ybar = np.asarray(ybar, dtype=np.complex128)
    g = np.zeros((K, N))
    yb = np.zeros_like(starts[0])
    for n in range(N - 1, -1, -1):
        if bar_all:
            yb = yb + ybar[n]
        elif n == N - 1:
            yb = yb + ybar
        y = starts[n]
        ks, ys, Hs, w = [], [], [], []
        for s in range(S):
            lo, tau = interp_weights(n, nodes[s], N)
            c = (1 - tau) * sig[:, lo] + tau * sig[:, lo + 1]
            H = h0 + np.tensordot(c, hks, axes=1)
            y_s = y + sum((a * k for a, k in zip(A[s], ks) if a != 0.0), 0)
            ks.append(dt * _F(step, H, y_s, col))
            ys.append(y_s)
            Hs.append(H)
            w.append((lo, tau))
        kb = [b * yb for b in Bw]
        for s in range(S - 1, -1, -1):
            zb = dt * _Fadj(step, Hs[s], kb[s], col)
            lo, tau = w[s]
            for k in range(K):
                cb = np.real(np.vdot(kb[s], dt * _dF(step, hks[k], ys[s])))
                g[k, lo] += (1 - tau) * cb
                g[k, lo + 1] += tau * cb
            yb = yb + zb
            for j, a in enumerate(A[s]):
                if a != 0.0:
                    kb[j] = kb[j] + a * zb
    return g, yb


def vjp_batch(h0, hks, sig, dt, init, solver, step, bar, col=None, bar_all=False):
    """The batch: sig [B, K, N], init [D, M] or [B, D, M], bar [B, D, M] or [B, N, D, M]."""
    B = sig.shape[0]
    init = np.asarray(init)
    gs, ib = [], []
    for b in range(B):
        g, y = vjp(h0, hks, sig[b], dt, init[b] if init.ndim == 3 else init, solver, step, bar[b], col, bar_all)
        gs.append(g)
        ib.append(y)
    return np.stack(gs), np.stack(ib)


def ketket_infid_and_bar(target, psi):
    """1 - |<t|psi>| (tf_ketket_fid) and its cotangent -(z / |z|) t (zero where the overlap is zero)."""
    z = np.vdot(target, psi)
    a = abs(z)
    return 1 - a, (-(z / a) * target if a > 0 else np.zeros_like(target))


def dmket_infid_and_bar(target, rho):
    """1 - sqrt(Re <t|rho|t>) (tf_dmket_fid) and its cotangent -t t^+ / (2 sqrt(.))."""
    t = np.asarray(target).reshape(-1)
    r = np.real(np.conj(t) @ rho @ t)
    f = np.sqrt(r)
    return 1 - f, (-np.outer(t, np.conj(t)) / (2 * f) if r > 0 else np.zeros_like(rho))
