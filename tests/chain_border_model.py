"""Lane-level numpy model of ONE block of v_mfma_f64_4x4x4_4b_f64 and of the core + border chain step of the small-D real loop
(c3p_smalld.hip, chain_step8<NC>, D = 4 NC + 1), written exactly as the kernel forms it.

A register of a chain is a [4][4] array indexed by the lane's (r, c).  The instruction is out = a^T b + c on such arrays,
out[i][j] = sum_k a[k][i] b[k][j] + c[i][j]: against a tile of ones as B it delivers sum_r a(r, c = i) replicated over j (the "r form"
of a vector), against ones as A it delivers sum_r b(r, c = j) replicated over i (the "c form").
Shared by tests/test_chain_border_model.py; imports nothing but numpy."""
import numpy as np

ONES = np.ones((4, 4))


def mfma4(a, b, c):
    """one block of the matrix instruction on [r][c] lane arrays"""
    return a.T @ b + c


class SMat:
    """symmetric matrix, left-operand form: core tiles m[K][I] (lane (r, c): M[4K+r][4I+c]), vr[I] (lane (r, c): M[4I+r][D-1]), s"""

    def __init__(self, M):
        D = M.shape[0]
        nc = (D - 1) // 4
        self.m = [[M[4 * K : 4 * K + 4, 4 * I : 4 * I + 4].copy() for I in range(nc)] for K in range(nc)]
        self.vr = [np.repeat(M[4 * I : 4 * I + 4, D - 1][:, None], 4, axis=1) for I in range(nc)]
        self.s = np.full((4, 4), M[D - 1, D - 1])


class GMat:
    """general matrix (the chain state): core tiles, column border cr[I] (r form: lane (r, c) holds M[4I+r][D-1]), row border rc[J]
    (c form: lane (r, c) holds M[D-1][4J+c]), corner s"""

    def __init__(self, M):
        D = M.shape[0]
        nc = (D - 1) // 4
        self.nc = nc
        self.m = [[M[4 * K : 4 * K + 4, 4 * J : 4 * J + 4].copy() for J in range(nc)] for K in range(nc)]
        self.cr = [np.repeat(M[4 * I : 4 * I + 4, D - 1][:, None], 4, axis=1) for I in range(nc)]
        self.rc = [np.repeat(M[D - 1, 4 * J : 4 * J + 4][None, :], 4, axis=0) for J in range(nc)]
        self.s = np.full((4, 4), M[D - 1, D - 1])

    def dense(self):
        """the matrix read back from lane 0's view: core tiles, cr along r at c = 0, rc along c at r = 0, s of lane (0, 0)"""
        nc = self.nc
        D = 4 * nc + 1
        M = np.empty((D, D))
        for I in range(nc):
            for J in range(nc):
                M[4 * I : 4 * I + 4, 4 * J : 4 * J + 4] = self.m[I][J]
            M[4 * I : 4 * I + 4, D - 1] = self.cr[I][:, 0]
            M[D - 1, 4 * I : 4 * I + 4] = self.rc[I][0, :]
        M[D - 1, D - 1] = self.s[0, 0]
        return M


def chain_step8(Cc, Sc, Ur, Ui):
    """(Ur + i Ui) <- (C - i S)(Ur + i Ui) in place, operation by operation as chain_step8<NC> of the kernel"""
    nc = Ur.nc
    R = range(nc)
    Dm = [[Cc.m[I][J] - Sc.m[I][J] for J in R] for I in R]
    Us = [[Ur.m[I][J] + Ui.m[I][J] for J in R] for I in R]
    dv = [Cc.vr[I] - Sc.vr[I] for I in R]
    us = [Ur.rc[I] + Ui.rc[I] for I in R]
    # rank-1 term of the core: initial accumulators, 3M form
    T1 = [[Cc.vr[I] * Ur.rc[J] for J in R] for I in R]
    T2 = [[Sc.vr[I] * Ui.rc[J] for J in R] for I in R]
    T3 = [[dv[I] * us[J] for J in R] for I in R]
    # row border
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
    # column border and corner
    pr, pi, qr, qi = [], [], [], []
    cr_, ci_ = Cc.vr[0] * Ur.cr[0], Cc.vr[0] * Ui.cr[0]
    for I in R:
        a, b = Cc.m[0][I] * Ur.cr[0], Cc.m[0][I] * Ui.cr[0]
        for K in range(1, nc):
            a, b = a + Cc.m[K][I] * Ur.cr[K], b + Cc.m[K][I] * Ui.cr[K]
        for K in R:
            a, b = a + Sc.m[K][I] * Ui.cr[K], b - Sc.m[K][I] * Ur.cr[K]
        pr.append(a), pi.append(b)
        qr.append(Sc.vr[I] * Ui.s + Cc.vr[I] * Ur.s)
        qi.append(-Sc.vr[I] * Ur.s + Cc.vr[I] * Ui.s)
        if I > 0:
            cr_, ci_ = cr_ + Cc.vr[I] * Ur.cr[I], ci_ + Cc.vr[I] * Ui.cr[I]
    for I in R:
        cr_, ci_ = cr_ + Sc.vr[I] * Ui.cr[I], ci_ - Sc.vr[I] * Ur.cr[I]
    er, ei = Sc.s * Ui.s + Cc.s * Ur.s, -Sc.s * Ur.s + Cc.s * Ui.s
    # the matrix instructions
    for K in R:
        for I in R:
            for J in R:
                T1[I][J] = mfma4(Cc.m[K][I], Ur.m[K][J], T1[I][J])
                T2[I][J] = mfma4(Sc.m[K][I], Ui.m[K][J], T2[I][J])
                T3[I][J] = mfma4(Dm[K][I], Us[K][J], T3[I][J])
    for I in R:
        Ur.rc[I] = mfma4(ONES, tr[I], ar[I])
        Ui.rc[I] = mfma4(ONES, ti[I], ai[I])
        Ur.cr[I] = mfma4(pr[I], ONES, qr[I])
        Ui.cr[I] = mfma4(pi[I], ONES, qi[I])
    Ur.s = mfma4(cr_, ONES, er)
    Ui.s = mfma4(ci_, ONES, ei)
    for I in R:
        for J in R:
            Ur.m[I][J] = T1[I][J] + T2[I][J]
            Ui.m[I][J] = (T3[I][J] - T1[I][J]) + T2[I][J]
