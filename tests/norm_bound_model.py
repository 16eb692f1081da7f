"""numpy model of the small-D chain kernels' segment-wide bound on ||X(t)||_1, X(t) = G_0 + sum_k c_k(t) G_k with
G = -i dt (h - Re tr h / D): the sum of norms the kernels used, the column-wise bound they use now (c3p_smalld.hip,
c3p_sd_segment_norm) and the exact maximum over the slices of a segment.  Shared by tests/test_norm_bound.py (CPU) and
tests/test_gpu_smalld_norm_bound.py."""
import numpy as np

MM6_THETA, MM8_THETA = 0.83, 1.85  # radii of the degree-6 and degree-8 cos / sin pairs (c3p_common.h)


def segments(n, s, per_mille=700):
    """[n0, n1) of the s segments of a sample as launch_chain_t / split_segments deal them in the workgroup-per-sample mode with
    eight waves (s = 32): the first s / 2 chains take the long segments, the others share the rest.  per_mille = 500: equal
    segments, [g n / s, (g + 1) n / s)."""
    if per_mille == 500:
        return [((g * n) // s, ((g + 1) * n) // s) for g in range(s)]
    h = s // 2
    la = max(1, (n * per_mille) // (500 * s))
    if h * la > n - h:
        la = (n - h) // h
    rest = n - h * la
    edge = lambda g: g * la if g <= h else h * la + ((g - h) * rest) // h
    return [(edge(g), edge(g + 1)) for g in range(s)]


def shifted_abs(h, dt):
    """|G|, G = -i dt h with the imaginary trace shift of build_tables (the real part of tr h)"""
    D = h.shape[-1]
    return np.abs(dt * (h - np.trace(h).real / D * np.eye(D)))


def column_sums(h0, hks, dt):
    """[1 + K, D]: cs_k[j] = sum_i |G_k[i][j]|"""
    return np.stack([shifted_abs(h, dt).sum(axis=0) for h in [h0, *hks]])


def bounds(h0, hks, sig, dt, n0, n1):
    """(exact, column-wise, sum of norms) of one sample's segment [n0, n1); sig is [K, N]"""
    K = sig.shape[0]
    D = h0.shape[-1]
    cs = column_sums(h0, hks, dt)
    cmax = np.abs(sig[:, n0:n1]).max(axis=1) if K else np.zeros(0)
    son = cs[0].max() + float(np.dot(cmax, cs[1:].max(axis=1))) if K else cs[0].max()
    col = (cs[0] + cmax @ cs[1:]).max() if K else cs[0].max()
    shift = lambda h: h - np.trace(h).real / D * np.eye(D)
    X = shift(h0)[None] + (np.einsum("kn,kij->nij", sig[:, n0:n1], np.stack([shift(h) for h in hks])) if K else 0.0)
    exact = np.abs(dt * X).sum(axis=-2).max()
    return float(exact), float(col), float(son)


def wave_bounds(h0, hks, sig, dt, s, per_mille=700):
    """[B, s / 4, 3]: per sample and wave (four consecutive segments) the maximum of each of the three bounds; sig is [B, K, N],
    h0 / hks shared ([D, D], [K, D, D]) or per sample ([B, D, D], [B, K, D, D])"""
    B, _, N = sig.shape
    seg = segments(N, s, per_mille)
    out = np.empty((B, s // 4, 3))
    for b in range(B):
        hb0 = h0[b] if h0.ndim == 3 else h0
        hbk = hks[b] if hks.ndim == 4 else hks
        per_seg = np.array([bounds(hb0, hbk, sig[b], dt, n0, n1) for n0, n1 in seg])
        out[b] = per_seg.reshape(s // 4, 4, 3).max(axis=1)
    return out
