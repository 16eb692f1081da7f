"""Host-side description of the small-D model record (include/c3prop.h: c3p_pwc_record_bytes / _build / c3p_pwc_unitary_rec).

A record is the block the small-D chain kernel's table build leaves in LDS for one model (h0, hks, dt): 1 + K tables of
MAT + 4 doubles -- the half image of G_k = -i dt h_k with its diagonal shifted by i mu (see `reference_tables`) in rows of W doubles
(row 2 i: Re G[i, :], row 2 i + 1: Im G[i, :], zero padded), then {Re mu, Im mu, ||G||_1, flag} -- followed by 1 + K blocks of
16 column sums, cs_k[j] = sum_i |G_k[i, j]| (zeros behind column D - 1).  The flag is 0 for a real symmetric Hamiltonian
(the generator is purely imaginary), negative for a complex skew-Hermitian generator, positive otherwise.

Nothing here touches the GPU: the size mirror and the numpy restatement are what the tests check the device's record against.
"""
from __future__ import annotations

import numpy as np

D_MIN, D_MAX, K_MAX = 2, 12, 8
CSW = 16  # column-sum slots per table


def mat_doubles(D: int) -> int:
    """MAT: doubles of one half image (c3p_smalld.hip: SD<D>::MAT)."""
    return 4 * ((D + 1) // 2) * row_stride(D)


def row_stride(D: int) -> int:
    """W: doubles between the rows of a half image."""
    return 4 * ((D + 3) // 4) + 1


def record_bytes(D: int, K: int) -> int:
    """Mirror of c3p_pwc_record_bytes: 0 where no record is served."""
    if D < D_MIN or D > D_MAX or K < 0 or K > K_MAX:
        return 0
    return 8 * (1 + K) * (mat_doubles(D) + 4 + CSW)


def reference_tables(h0, hks, dt: float):
    """numpy restatement of the table build: (G [1+K,D,D] complex, mu_im [1+K], colsums [1+K,D]).

    G = -i dt h with the diagonal shifted by i mu_im, mu_im = Im tr(-i dt h) / D (the shift is imaginary only: a lossy drift
    keeps its real trace); colsums[k, j] = sum_i |G_k[i, j]|."""
    h0 = np.asarray(h0, dtype=np.complex128)
    D = h0.shape[-1]
    hs = np.concatenate([h0[None], np.asarray(hks, dtype=np.complex128).reshape(-1, D, D)])
    G = np.empty_like(hs)
    G.real = hs.imag * dt
    G.imag = -hs.real * dt
    mu = np.array([np.trace(g).imag / D for g in G])
    for g, m in zip(G, mu):
        g[np.diag_indices(D)] -= 1j * m
    cs = np.sqrt(G.real ** 2 + G.imag ** 2).sum(axis=1)
    return G, mu, cs


def unpack_record(rec, D: int, K: int):
    """A record (1-D float64 array) taken apart: {"G": [1+K,D,D] complex, "mu": [1+K,2], "norm1": [1+K], "flag": [1+K],
    "colsums": [1+K,16], "padding": every image word outside the D x D block (all zero in a well-formed record)}."""
    rec = np.asarray(rec, dtype=np.float64).ravel()
    MAT, W = mat_doubles(D), row_stride(D)
    if rec.size * 8 != record_bytes(D, K):
        raise ValueError(f"a record of D={D}, K={K} holds {record_bytes(D, K) // 8} doubles, got {rec.size}")
    T = (1 + K) * (MAT + 4)
    tabs = rec[:T].reshape(1 + K, MAT + 4)
    img = tabs[:, :MAT].reshape(1 + K, MAT // W, W)
    G = img[:, 0 : 2 * D : 2, :D] + 1j * img[:, 1 : 2 * D : 2, :D]
    pad = img.copy()
    pad[:, : 2 * D, :D] = 0.0
    return {"G": G, "mu": tabs[:, MAT : MAT + 2], "norm1": tabs[:, MAT + 2], "flag": tabs[:, MAT + 3],
            "colsums": rec[T:].reshape(1 + K, CSW), "padding": pad}
