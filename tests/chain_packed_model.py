"""Lane-level numpy model of the chain step of the small-D real loop with the column border and the corner of the state PACKED
(c3p_smalld.hip, chain_step8<NC> with GBorder<NC>, D = 4 NC + 1), operation by operation as the kernel forms it.

A register of a chain is a [4][4] array indexed by the lane's (r, c), as in tests/chain_border_model.py, whose mfma4 (out = a^T b + c)
and SMat / GMat this model is built on.  The complex border column u = U[:, D-1] and the corner are carried as ONE register each, Re
and Im dealt over the quad index c:
    Pc[K][r][c] = {Re u, Im u, -Re u, -Im u}[c] at row 4K + r,      Ps[r][c] = the same of the corner, replicated over r.
The quad rotation (lane c reads lane (c + 1) mod 4 of its quad) turns {Re, Im, -Re, -Im} into {Im, -Re, -Im, Re}, the packed form of
-i u.  With E = C - i S, column c of C P + S Q is the packed form of E u again.
Shared by tests/test_chain_packed_model.py and tests/test_gpu_smalld_packed_border.py; imports nothing but numpy and chain_border_model."""
import numpy as np

from chain_border_model import ONES, GMat, SMat, mfma4


def quad_rot(p, k=1):
    """lane (r, c) reads lane (r, (c + k) mod 4)"""
    return np.roll(p, -k, axis=1)


def pack_lanes(re, im):
    """[4][4] packed register from the values every lane holds (arrays over (r, c)): select on c, negate where c >= 2"""
    c = np.arange(4)[None, :]
    v = np.where(c & 1, im, re)
    return np.where(c & 2, -v, v)


class Border:
    """packed column border and corner of a complex D x D state"""

    def __init__(self, U):
        D = U.shape[0]
        nc = (D - 1) // 4
        self.nc = nc
        rep = lambda v: np.repeat(v[:, None], 4, axis=1)  # r form: replicated over c
        self.Pc = [pack_lanes(rep(U[4 * K : 4 * K + 4, D - 1].real), rep(U[4 * K : 4 * K + 4, D - 1].imag)) for K in range(nc)]
        self.Ps = pack_lanes(np.full((4, 4), U[D - 1, D - 1].real), np.full((4, 4), U[D - 1, D - 1].imag))

    def column(self, swap=False):
        """the complex border column and corner as the kernel stores them: lanes c = 0 and c = 1 hold Re and Im (rows from r; the
        corner from lane r = 0).  swap: Re and Im exchanged, a wrong unpack"""
        re, im = (1, 0) if swap else (0, 1)
        col = np.concatenate([P[:, re] + 1j * P[:, im] for P in self.Pc])
        return np.append(col, self.Ps[0, re] + 1j * self.Ps[0, im])


class State:
    """the chain state: core and row border of the real and the imaginary part (GMat of chain_border_model; its cr and s are not
    used), column border and corner packed"""

    def __init__(self, U):
        self.nc = (U.shape[0] - 1) // 4
        self.Ur, self.Ui, self.Ub = GMat(U.real.copy()), GMat(U.imag.copy()), Border(U)

    def dense(self, swap=False):
        D = 4 * self.nc + 1
        M = self.Ur.dense() + 1j * self.Ui.dense()
        M[:, D - 1] = self.Ub.column(swap)
        return M


def chain_step(Cc, Sc, st, rot=1, corner_in_column=True, ss_in_corner=True):
    """st <- (C - i S) st in place.  The keyword arguments switch on the WRONG steps that the tests' inputs must tell from the right
    one: rot = 3 rotates the other way (i u instead of -i u: the border column conjugated), corner_in_column = False drops the
    k = D-1 term of the column, ss_in_corner = False drops S.s Qs from the corner."""
    Ur, Ui, Ub = st.Ur, st.Ui, st.Ub
    nc = st.nc
    R = range(nc)
    Qc = [quad_rot(Ub.Pc[K], rot) for K in R]
    Qs = quad_rot(Ub.Ps, rot)
    Dm = [[Cc.m[I][J] - Sc.m[I][J] for J in R] for I in R]
    Us = [[Ur.m[I][J] + Ui.m[I][J] for J in R] for I in R]
    dv = [Cc.vr[I] - Sc.vr[I] for I in R]
    us = [Ur.rc[I] + Ui.rc[I] for I in R]
    T1 = [[Cc.vr[I] * Ur.rc[J] for J in R] for I in R]
    T2 = [[Sc.vr[I] * Ui.rc[J] for J in R] for I in R]
    T3 = [[dv[I] * us[J] for J in R] for I in R]
    # row border, as chain_border_model.chain_step8
    tr, ti, ar, ai = [], [], [], []
    for J in R:
        a, b = Cc.vr[0] * Ur.m[0][J], Cc.vr[0] * Ui.m[0][J]
        for K in range(1, nc):
            a, b = a + Cc.vr[K] * Ur.m[K][J], b + Cc.vr[K] * Ui.m[K][J]
        for K in R:
            a, b = a + Sc.vr[K] * Ui.m[K][J], b - Sc.vr[K] * Ur.m[K][J]
        tr.append(a), ti.append(b)
        ar.append(Sc.s * Ui.rc[J] + Cc.s * Ur.rc[J])
        ai.append(-Sc.s * Ur.rc[J] + Cc.s * Ui.rc[J])
    # column border and corner, packed
    Pn = [Sc.vr[I] * Qs + Cc.vr[I] * Ub.Ps if corner_in_column else np.zeros((4, 4)) for I in R]
    ts = Cc.vr[0] * Ub.Pc[0]
    for K in range(1, nc):
        ts = ts + Cc.vr[K] * Ub.Pc[K]
    for K in R:
        ts = ts + Sc.vr[K] * Qc[K]
    es = Sc.s * Qs + Cc.s * Ub.Ps if ss_in_corner else Cc.s * Ub.Ps
    # the matrix instructions
    for K in R:
        for I in R:
            Pn[I] = mfma4(Cc.m[K][I], Ub.Pc[K], Pn[I])
            for J in R:
                T1[I][J] = mfma4(Cc.m[K][I], Ur.m[K][J], T1[I][J])
                T2[I][J] = mfma4(Sc.m[K][I], Ui.m[K][J], T2[I][J])
                T3[I][J] = mfma4(Dm[K][I], Us[K][J], T3[I][J])
            Pn[I] = mfma4(Sc.m[K][I], Qc[K], Pn[I])
    for I in R:
        Ur.rc[I] = mfma4(ONES, tr[I], ar[I])
        Ui.rc[I] = mfma4(ONES, ti[I], ai[I])
    Ub.Ps = mfma4(ONES, ts, es)
    for I in R:
        Ub.Pc[I] = Pn[I]
        for J in R:
            Ur.m[I][J] = T1[I][J] + T2[I][J]
            Ui.m[I][J] = (T3[I][J] - T1[I][J]) + T2[I][J]


def first_slice(C, S):
    """the peeled first slice of a segment: U <- E = C - i S, the border packed from the r-form border and the corner of C and -S by a
    select on c"""
    return State(C - 1j * S)


def slice_cos_sin(h0, hks, sig_n, dt):
    """C = cos Y, S = sin Y of one slice, Y = dt (H - tr H / D) for the real symmetric H = h0 + sum_k sig_n[k] hks[k]"""
    H = (h0 + np.tensordot(sig_n, hks, axes=1) if len(hks) else h0).real
    D = H.shape[0]
    w, V = np.linalg.eigh(dt * (H - np.trace(H) / D * np.eye(D)))
    C, S = (V * np.cos(w)) @ V.T, (V * np.sin(w)) @ V.T
    return 0.5 * (C + C.T), 0.5 * (S + S.T)


def propagate(h0, hks, sig, dt, seg, swap=False, **wrong):
    """the traceless propagator of one sample ([K, N] amplitudes) as the kernel chains it: every segment [n0, n1) from its peeled first
    slice and the packed step, the segments folded densely, later ones on the left"""
    D = h0.shape[0]
    U = np.eye(D, dtype=complex)
    for n0, n1 in seg:
        st = first_slice(*slice_cos_sin(h0, hks, sig[:, n0], dt))
        for n in range(n0 + 1, n1):
            C, S = slice_cos_sin(h0, hks, sig[:, n], dt)
            chain_step(SMat(C), SMat(S), st, **wrong)
        U = st.dense(swap) @ U
    return U
