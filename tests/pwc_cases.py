"""Cases of the extended-precision tests of the assembled PWC propagators (`propagate_batch`: c3p_pwc_unitary, c3p_pwc_lindblad).

One case = one library call: a problem (operators, amplitudes, dt: a pure function of the `Problem` tuple), the launch form
(library options, want_dUs), the kernel class it is expected to run in and the polynomial scheme it claims to reach.  The
scheme is steered by the NORM BOUND the device plans with, restated here kernel family by kernel family (`norm_bound`,
`scheme_of`) from the radii of c3_amd/csrc/c3p_common.h; tests/test_pwc_extended_ref.py asserts, without a GPU, that every case's
bound lies in the band it claims and that every slice stays inside the radius of Pade-13 (above it the oracle's floor rule
inflates e_cpu and the bar of tests/test_gpu_pwc_extended.py would go slack).

Amplitudes have magnitude exactly 1 on every even slice (random sign) and a magnitude in [0.3, 1) on the odd ones: every time
segment of two or more slices has max_t |c_k(t)| = 1, so the bound of every segment is the bound of the sample, whatever the
segmentation.  Launches whose default segmentation could deal single slices set the library's segment options.
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

import extended_ref as x

# ---------------------------------------------------------------------------------------------------------------------------
# radii (c3_amd/csrc/c3p_common.h) and the plans built on them, restated
# ---------------------------------------------------------------------------------------------------------------------------
MM6_THETA, MM8_THETA = 0.83, 1.85  # C3P_MM6_THETA, C3P_MM8_THETA: economised cos / sin pairs of degree 6 and 8
T18_THETA, E4N_THETA, T18N_THETA = 1.13, 1.35, 2.0  # C3P_T18_THETA, C3P_E4N_THETA, C3P_T18N_THETA
T18N_MAX_NONNORMAL = 0.25  # C3P_T18N_MAX_NONNORMAL
Q4_THETA = x.Q4_THETA  # c3p_pick_plan_q4
EDGE = x.EDGE


def squarings(nrm: float, theta: float) -> int:
    """c3p_squarings: the smallest s with theta 2^s >= nrm."""
    s, p = 0, theta
    while p < nrm and s < 40:
        p *= 2.0
        s += 1
    return s


def plan_q4(nrm: float):
    """c3p_pick_plan_q4 -> (r, s): degree 4r, s squarings."""
    best = (5, 0, 1 << 30)
    for i, th in enumerate(Q4_THETA):
        si = squarings(nrm, th)
        cost = i + si
        if cost < best[2] or (cost == best[2] and si <= best[1]):
            best = (i + 1, si, cost)
    return best[0], best[1]


def plan_mfma(nrm: float, theta18: float = T18_THETA, normal: bool = False):
    """c3p_pick_plan_mfma -> (t18, r, s): t18 = 1 T18 (published or economised parameters), 2 the four-product scheme."""
    r, s = plan_q4(nrm)
    s18 = squarings(nrm, theta18)
    t18, cost = (1, 5 + s18) if 5 + s18 < 3 + (r - 1) + s else (0, 3 + (r - 1) + s)
    if t18:
        r, s = 0, s18
    if normal:
        s4 = squarings(nrm, E4N_THETA)
        if 4 + s4 < cost:
            t18, r, s = 2, 0, s4
    return t18, r, s


# kernel family -> which bound the kernel plans with
#   "col":   max_j (cs_0[j] + sum_k max|c_k| cs_k[j]), cs the column sums of |G| (small-D chain kernel, tables)
#   "sum":   ||G_0||_1 + sum_k max|c_k| ||G_k||_1 (mid-D, regd, bigd, tiled)
#   "hb":    "sum" of the REAL generators in the Hermitian basis, no trace shift (smallr, regr), with the symmetric part
#   "slice": max_n ||X_n - i Im tr X_n / D||_1 (supplied generators: branch B)
FAMILY_BOUND = {"sd_real": "col", "sd_real_pad": "col", "sd_normal": "col", "sd_general": "col", "md_real": "sum", "md_normal": "sum",
                "md_general": "sum", "t18": "sum", "hb_small": "hb", "hb_reg": "hb", "xg_general": "slice", "xg_t18": "slice"}


def scheme_of(family: str, bound: float, nsym: float = 0.0) -> str:
    """The polynomial and squarings a kernel of `family` takes at norm bound `bound` (symmetric part `nsym`), as
    "<polynomial>+<squarings>"."""
    if family in ("sd_real", "sd_real_pad", "md_real"):
        s = squarings(bound, MM8_THETA)
        deg6 = family == "sd_real" and bound * 2.0**-s <= MM6_THETA  # the core + border loop of D = 5, 9 alone has the degree-6 pair
        return f"{'mm6' if deg6 else 'mm8'}+{s}"
    if family in ("sd_normal", "md_normal"):
        t18, r, s = plan_mfma(bound, T18N_THETA, True)
        return f"{('ps%d' % (4 * r), 't18n', 'e4n')[t18]}+{s}"
    if family in ("sd_general", "md_general", "xg_general"):
        t18, r, s = plan_mfma(bound)
        return f"{('ps%d' % (4 * r), 't18')[t18]}+{s}"
    if family in ("t18", "xg_t18"):
        return f"t18+{squarings(bound, T18_THETA)}"
    if family in ("hb_small", "hb_reg"):
        econ = nsym <= T18N_MAX_NONNORMAL
        s = squarings(bound, T18N_THETA if econ else T18_THETA)
        if family == "hb_small" and econ and 4 + squarings(bound, E4N_THETA) < 5 + s:
            return f"e4n+{squarings(bound, E4N_THETA)}"
        return f"{'t18n' if econ else 't18'}+{s}"
    raise ValueError(family)


# ---------------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------------
# ham: "real" (real symmetric), "herm" (complex Hermitian), "nonherm" (a traceless non-Hermitian part of 5 %),
#      "mixed" (per-sample operators, sample 1 with a complex Hermitian control among real ones)
# bound: the key of FAMILY_BOUND's values the target refers to;  target: value of that bound (dt is chosen for it)
# trace: h0 + trace 1, hk + trace / 2 1 and amplitudes mostly of one sign (the summed phase winds);  phase: fr_phase given
# lind: None | (C, rate, per_sample): C annihilation-type collapse operators sqrt(rate) a-like, shared or one set per sample
# per_slice: branch B, the per-slice Hamiltonians handed over themselves, every slice scaled to its own norm
Problem = namedtuple("Problem", "tag D K N B ham bound target trace phase lind per_slice hk_scale")
Case = namedtuple("Case", "id problem family scheme opts dUs kernel")


def _problem(tag, D, K, N, B, ham, bound, target, trace=0.0, phase=False, lind=None, per_slice=False, hk_scale=0.4):
    return Problem(tag, D, K, N, B, ham, bound, float(target), float(trace), phase, lind, per_slice, hk_scale)


def _rng(p: Problem):
    return np.random.default_rng([zlib.crc32(p.tag.encode()), p.D, p.K, p.N, p.B])


def _herm(rng, D, s, real):
    m = rng.normal(size=(D, D)) + (0 if real else 1j) * rng.normal(size=(D, D))
    return (s * (m + m.conj().T) / 2).astype(np.complex128)


def hb_transform(D: int) -> np.ndarray:
    """T[D^2, D^2]: row-major vec(rho) -> its coefficients in the Hermitian basis E_ii, (E_ij + E_ji) / sqrt 2,
    i (E_ji - E_ij) / sqrt 2 (c3p_smallr.hip, c3p_regr.hip); unitary.  The order of the basis does not enter a 1-norm."""
    rows = []
    for i in range(D):
        for j in range(i, D):
            if i == j:
                b = np.zeros((D, D), complex)
                b[i, i] = 1
                rows.append(b)
            else:
                s, a = np.zeros((D, D), complex), np.zeros((D, D), complex)
                s[i, j] = s[j, i] = 2**-0.5
                a[j, i], a[i, j] = 1j * 2**-0.5, -1j * 2**-0.5
                rows += [s, a]
    return np.stack([np.conj(b).reshape(-1) for b in rows])


def _shifted(G):
    """G - tr G / D: the generator tables carry the trace as a separate phase."""
    D = G.shape[-1]
    return G - np.trace(G) / D * np.eye(D)


def generator_tables(h0, hks, dt, col=None):
    """[G_0, G_1 .. G_K] of one sample in double: -i dt h, or dt L(h0) with the dissipator and dt (L(hk) - dissipator)."""
    from oracle import c3_oracle as o

    if col is None:
        return [-1j * dt * h0] + [-1j * dt * hk for hk in hks]
    clp = o.lindblad_dissipator(col)
    return [dt * o.lindblad_generator(h0, col)[0]] + [dt * (o.lindblad_generator(hk, col)[0] - clp) for hk in hks]


def norm_bound(kind: str, tables, cmax, D: int = 0):
    """(bound, symmetric part) of one sample or segment from its generator tables and max_t |c_k(t)| (`cmax[K]`)."""
    w = [1.0] + [float(c) for c in cmax]
    if kind == "hb":
        T = hb_transform(D)
        Gp = [T @ G @ T.conj().T for G in tables]
        assert all(np.abs(g.imag).max() <= 1e-13 * max(1.0, np.abs(g).max()) for g in Gp), "generator not real in the Hermitian basis"
        Gp = [g.real for g in Gp]
        return (sum(a * x.norm1(g) for a, g in zip(w, Gp)), sum(a * x.norm1((g + g.T) / 2) for a, g in zip(w, Gp)))
    S = [_shifted(G) for G in tables]
    if kind == "col":
        return float(sum(a * np.abs(g).sum(axis=0) for a, g in zip(w, S)).max()), 0.0
    if kind == "sum":
        return sum(a * x.norm1(g) for a, g in zip(w, S)), 0.0
    raise ValueError(kind)


PwcInputs = namedtuple("PwcInputs", "h0 hks signals dt col fr_phase bounds nsyms")


def _amplitudes(rng, p: Problem):
    mag = rng.uniform(0.3, 1.0, size=(p.B, p.K, p.N))
    mag[:, :, 0::2] = 1.0
    sign = np.where(rng.uniform(size=(p.B, p.K, p.N)) < (0.85 if p.trace else 0.5), 1.0, -1.0)
    return sign * mag


def _collapse(rng, p: Problem):
    C, rate, per_sample = p.lind
    D = p.D
    a = np.diag(np.sqrt(np.arange(1.0, D)), 1).astype(np.complex128)
    one = lambda: np.stack([np.sqrt(rate * (1 + 0.3 * c)) * (a + 0.1 * (rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))) * (c > 0)) for c in range(C)])
    return np.stack([one() * (1 + 0.2 * b) for b in range(p.B)]) if per_sample else one()


def _build(p: Problem) -> PwcInputs:
    rng = _rng(p)
    D, K, N, B = p.D, p.K, p.N, p.B
    real = p.ham in ("real", "mixed")
    h0 = np.diag(rng.uniform(0, 1, D)).astype(np.complex128) + _herm(rng, D, 0.05, real) + p.trace * np.eye(D)
    hks = np.stack([_herm(rng, D, p.hk_scale, real) + 0.5 * p.trace * np.eye(D) for _ in range(K)]) if K else np.zeros((0, D, D), np.complex128)
    if p.ham == "nonherm":
        m = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
        h0 = h0 + 0.05 * (m - np.trace(m) / D * np.eye(D))
    if p.ham == "mixed":
        h0, hks = np.stack([h0] * B), np.stack([hks] * B)
        a = rng.normal(size=(D, D))
        hks[1, 0] = hks[1, 0] + 0.2j * (a - a.T)
    sig = _amplitudes(rng, p)
    col = _collapse(rng, p) if p.lind else None
    ph = rng.uniform(0, 6.28, size=(B, D * D if p.lind else D)) if p.phase else None
    cmax = np.ones(K)

    def sample_bound(b, dt):
        hb, kb = (h0[b], hks[b]) if h0.ndim == 3 else (h0, hks)
        cb = None if col is None else (col[b] if col.ndim == 4 else col)
        return norm_bound(p.bound, generator_tables(hb, kb, dt, cb), cmax, D)

    if p.per_slice:
        # branch B: H_n = h0 + sum_k c_k(n) hk, then every slice scaled so that ||X_n - i Im tr X_n / D||_1 is the target on the
        # even slices and [0.5, 1) of it on the odd ones
        from oracle import c3_oracle as o

        dt = 0.05
        w = rng.uniform(0.5, 1.0, size=(B, N))
        w[:, 0::2] = 1.0
        H = h0[None, None] + np.einsum("bkn,kij->bnij", sig, hks)
        for b in range(B):
            for n in range(N):
                Xn = (dt * o.lindblad_generator(H[b, n], col)[0]) if p.lind else (-1j * dt * H[b, n])
                H[b, n] *= w[b, n] * p.target / x.device_norm(Xn)
        if p.lind:
            # the dissipator does not scale with H: settle the norms by a second pass (the generator is affine in H)
            for _ in range(60):
                for b in range(B):
                    for n in range(N):
                        H[b, n] *= w[b, n] * p.target / x.device_norm(dt * o.lindblad_generator(H[b, n], col)[0])
        bounds = np.array([max(x.device_norm((dt * o.lindblad_generator(H[b, n], col)[0]) if p.lind else (-1j * dt * H[b, n])) for n in range(N)) for b in range(B)])
        out = PwcInputs(np.ascontiguousarray(H), None, None, dt, col, ph, bounds, np.zeros(B))
    else:
        # the bound is linear in dt: one evaluation at dt = 1 fixes dt for the largest sample bound
        dt = p.target / max(sample_bound(b, 1.0)[0] for b in range(B if (h0.ndim == 3 or (col is not None and col.ndim == 4)) else 1))
        bs = [sample_bound(b, dt) for b in range(B)]
        out = PwcInputs(h0, hks, sig, float(dt), col, ph, np.array([v[0] for v in bs]), np.array([v[1] for v in bs]))
    for a in out[:6]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pwc_inputs(p: Problem) -> PwcInputs:
    return _build(p)


def slice_generators(inp: PwcInputs, lind: bool):
    """X[B, N, Dm, Dm] in double, assembled as the oracle assembles it."""
    from oracle import c3_oracle as o

    out = []
    B = inp.signals.shape[0] if inp.signals is not None else inp.h0.shape[0]
    for b in range(B):
        if inp.signals is None:
            H = inp.h0[b]
        else:
            H = o.sum_h0_hks(inp.h0[b] if inp.h0.ndim == 3 else inp.h0, inp.hks[b] if inp.hks.ndim == 4 else inp.hks, inp.signals[b])
        cb = None if inp.col is None else (inp.col[b] if inp.col.ndim == 4 else inp.col)
        out.append(o.lindblad_generator(H, cb) * complex(inp.dt) if lind else -1.0j * H * complex(inp.dt))
    return np.stack(out)


PwcRef = namedtuple("PwcRef", "U dUs X e_cpu e_oracle e_scipy r_cpu_slices")


@functools.lru_cache(maxsize=None)
def pwc_reference(p: Problem) -> PwcRef:
    """Long-double propagators of a problem (once per process, read-only), and the errors of the two double-precision CPU routes
    against them: `oracle.propagate_batch`, and scipy's expm slice by slice under the oracle's fold.  e_cpu is the worst of both
    over the samples; r_cpu_slices the worst `expm_ratio` of both over the slices."""
    import scipy.linalg

    from oracle import c3_oracle as o

    inp = pwc_inputs(p)
    lind = p.lind is not None
    U, dUs = x.pwc_ld(inp.h0, inp.hks, inp.signals, inp.dt, col_ops=inp.col, fr_phase=inp.fr_phase, want_dUs=True)
    Xld = x.pwc_generators_ld(inp.h0, inp.hks, inp.signals, inp.dt, col_ops=inp.col)
    X = slice_generators(inp, lind)
    B = X.shape[0]
    rows = None if inp.fr_phase is None else np.exp(1j * inp.fr_phase)
    dU_o, dU_s = o.expm(X), np.stack([scipy.linalg.expm(X[b]) for b in range(B)])
    e = []
    for dU in (dU_o, dU_s):
        Ud = np.stack([o.tf_matmul_n(dU[b]) for b in range(B)])
        if rows is not None:
            Ud = rows[:, :, None] * Ud
        e.append(x.pwc_err(Ud, U))
    r_cpu = max(x.slices_ratio(dU_o, Xld, dUs), x.slices_ratio(dU_s, Xld, dUs))
    for a in (U, dUs, Xld):
        a.setflags(write=False)
    return PwcRef(U, dUs, Xld, max(e), e[0], e[1], r_cpu)


# ---------------------------------------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------------------------------------
SD_N, SD_S = 131, 32  # eight waves of four chains: the fused workgroup-per-sample kernel with unequal segments
SD_OPTS = (("smalld_segments", SD_S),)
MD_N = 70  # one segment (segments=1) that crosses a 64-slice staging chunk
MD_OPTS = (("segments", 1),)


# Targets 10 % inside a band: below the radius where the band is the polynomial's own (its error is largest there), above the lower
# edge where the band is a squaring count (the unshifted slice norms must stay inside the radius of Pade-13)
T_PS4, T_PS8, T_PS12 = 0.9 * Q4_THETA[0], 0.9 * Q4_THETA[1], 0.9 * Q4_THETA[2]
T_MM6, T_MM8, T_MM8_1, T_MM8_2 = 0.9 * MM6_THETA, 0.9 * MM8_THETA, 1.1 * MM8_THETA, 1.1 * 2 * MM8_THETA
T_E4N, T_T18N, T_E4N_1 = 0.9 * E4N_THETA, 1.1 * E4N_THETA, 1.1 * T18N_THETA
T_T18, T_T18_1 = 0.9 * T18_THETA, 1.1 * T18_THETA
T_T18N_HI, T_T18N_1 = 0.9 * T18N_THETA, 1.1 * T18N_THETA


def _cases():
    cs = []

    def add(id_, prob, family, scheme, opts=(), dUs=False, kernel=None):
        cs.append(Case(id_, prob, family, scheme, tuple(opts), dUs, kernel or id_))

    # ---- small-D, real symmetric, core + border (D = 5, 9) ----
    real_bands = (("mm6+0", T_MM6), ("mm8+0", T_MM8), ("mm8+1", T_MM8_1),
                  ("mm8+2", T_MM8_2))
    for D in (5, 9):
        k = f"sd-real-D{D}"
        for scheme, t in real_bands:
            add(f"sd-real-D{D}-K2-{scheme}", _problem(f"sdr{scheme}", D, 2, SD_N, 3, "real", "col", t), "sd_real", scheme, SD_OPTS, kernel=k)
        add(f"sd-real-D{D}-K0-mm6+0", _problem("sdrK0", D, 0, SD_N, 3, "real", "col", real_bands[0][1]), "sd_real", "mm6+0", SD_OPTS, kernel=k)
        add(f"sd-real-D{D}-K3-mm6+0", _problem("sdrK3a", D, 3, SD_N, 3, "real", "col", real_bands[0][1]), "sd_real", "mm6+0", SD_OPTS, kernel=k)
        add(f"sd-real-D{D}-K3-mm8+0", _problem("sdrK3b", D, 3, SD_N, 3, "real", "col", real_bands[1][1]), "sd_real", "mm8+0", SD_OPTS, kernel=k)
        add(f"sd-real-D{D}-K2-trace-phase", _problem("sdrtr", D, 2, SD_N, 3, "real", "col", real_bands[0][1], trace=10.0, phase=True), "sd_real", "mm6+0", SD_OPTS, kernel=k)
        # a pair on either side of every edge
        for edge, lo, hi in ((MM6_THETA, "mm6+0", "mm8+0"), (MM8_THETA, "mm8+0", "mm8+1"), (2 * MM8_THETA, "mm8+1", "mm8+2")) if D == 9 else ((MM6_THETA, "mm6+0", "mm8+0"),):
            add(f"sd-real-D{D}-below-{edge:g}", _problem("sdre-", D, 2, SD_N, 2, "real", "col", edge * (1 - EDGE)), "sd_real", lo, SD_OPTS, kernel=k)
            add(f"sd-real-D{D}-above-{edge:g}", _problem("sdre+", D, 2, SD_N, 2, "real", "col", edge * (1 + EDGE)), "sd_real", hi, SD_OPTS, kernel=k)
    # the same at D = 9 without the core + border form (padded tiles: the degree-8 pair alone)
    k = "sd-real-D9-no_split81"
    o81 = SD_OPTS + (("no_split81", 1),)
    add("sd-real-D9-no_split81-mm8+0", _problem("sdrmm6+0", 9, 2, SD_N, 3, "real", "col", real_bands[0][1]), "sd_real_pad", "mm8+0", o81, kernel=k)
    add("sd-real-D9-no_split81-mm8+1", _problem("sdrmm8+1", 9, 2, SD_N, 3, "real", "col", real_bands[2][1]), "sd_real_pad", "mm8+1", o81, kernel=k)
    add("sd-real-D9-no_split81-trace-phase", _problem("sdrtr", 9, 2, SD_N, 3, "real", "col", real_bands[0][1], trace=10.0, phase=True), "sd_real_pad", "mm8+0", o81, kernel=k)
    # the other launch forms, same problem and reference as sd-real-D9-K2-mm6+0
    base = _problem("sdrmm6+0", 9, 2, SD_N, 3, "real", "col", real_bands[0][1])
    add("sd-real-D9-no_mw", base, "sd_real", "mm6+0", SD_OPTS + (("no_mw", 1),))
    add("sd-real-D9-no_fuse", base, "sd_real", "mm6+0", SD_OPTS + (("no_fuse", 1),))
    add("sd-real-D9-prep_kernel", base, "sd_real", "mm6+0", SD_OPTS + (("prep_kernel", 1),))
    add("sd-real-D9-dUs", base, "sd_real_pad", "mm8+0", SD_OPTS, dUs=True)
    # ---- small-D, real symmetric, padded tiles ----
    for D in (3, 4, 8, 12):
        k = f"sd-real-D{D}"
        add(f"sd-real-D{D}-mm8+0", _problem("sdp0", D, 2, SD_N, 3, "real", "col", T_MM8, phase=(D == 8)), "sd_real_pad", "mm8+0", SD_OPTS, kernel=k)
        add(f"sd-real-D{D}-mm8+1", _problem("sdp1", D, 2, SD_N, 3, "real", "col", T_MM8_1), "sd_real_pad", "mm8+1", SD_OPTS, kernel=k)
    # ---- small-D, complex Hermitian: the schemes for normal generators ----
    normal_bands = (("ps4+0", T_PS4), ("ps8+0", T_PS8), ("e4n+0", T_E4N),
                    ("t18n+0", T_T18N), ("e4n+1", T_E4N_1))
    for D in (3, 9, 12):
        k = f"sd-herm-D{D}"
        for scheme, t in normal_bands:
            add(f"sd-herm-D{D}-{scheme}", _problem("sdh" + scheme, D, 2, SD_N, 3, "herm", "col", t, phase=(scheme == "t18n+0")), "sd_normal", scheme, SD_OPTS, kernel=k)
    for edge, lo, hi in ((Q4_THETA[0], "ps4+0", "ps8+0"), (Q4_THETA[1], "ps8+0", "e4n+0"), (E4N_THETA, "e4n+0", "t18n+0"), (T18N_THETA, "t18n+0", "e4n+1")):
        add(f"sd-herm-D9-below-{edge:g}", _problem("sdhe-", 9, 2, SD_N, 2, "herm", "col", edge * (1 - EDGE)), "sd_normal", lo, SD_OPTS, kernel="sd-herm-D9")
        add(f"sd-herm-D9-above-{edge:g}", _problem("sdhe+", 9, 2, SD_N, 2, "herm", "col", edge * (1 + EDGE)), "sd_normal", hi, SD_OPTS, kernel="sd-herm-D9")
    # ---- small-D, non-Hermitian: published T18, Paterson-Stockmeyer ----
    k = "sd-nonherm-D9"
    for scheme, t in (("ps8+0", T_PS8), ("ps12+0", T_PS12), ("t18+0", T_T18),
                      ("t18+1", T_T18_1)):
        add(f"sd-nonherm-D9-{scheme}", _problem("sdn" + scheme, 9, 2, SD_N, 3, "nonherm", "col", t), "sd_general", scheme, SD_OPTS, kernel=k)
    add("sd-nonherm-D9-below-1.13", _problem("sdne-", 9, 2, SD_N, 2, "nonherm", "col", T18_THETA * (1 - EDGE)), "sd_general", "t18+0", SD_OPTS, kernel=k)
    add("sd-nonherm-D9-above-1.13", _problem("sdne+", 9, 2, SD_N, 2, "nonherm", "col", T18_THETA * (1 + EDGE)), "sd_general", "t18+1", SD_OPTS, kernel=k)
    # ---- one complex sample among real ones in the same launch ----
    add("sd-mixed-D9", _problem("sdmix", 9, 2, SD_N, 3, "mixed", "col", real_bands[0][1], trace=1.5, phase=True), "sd_real", "mm6+0", SD_OPTS)

    # ---- mid-D, real instance ----
    for D, scheme, K in ((13, "mm8+0", 3), (13, "mm8+1", 3), (16, "mm8+1", 4), (17, "mm8+0", 4), (27, "mm8+1", 3), (32, "mm8+0", 3), (36, "mm8+1", 4), (40, "mm8+0", 4)):
        t = T_MM8 if scheme == "mm8+0" else T_MM8_1
        add(f"md-real-D{D}-K{K}-{scheme}", _problem("mdr" + scheme, D, K, MD_N, 2, "real", "sum", t, phase=(D == 17)), "md_real", scheme, MD_OPTS, kernel=f"md-real-D{D}-K{K}")
    add("md-real-D13-below-1.85", _problem("mdre-", 13, 3, MD_N, 2, "real", "sum", MM8_THETA * (1 - EDGE)), "md_real", "mm8+0", MD_OPTS, kernel="md-real-D13-K3")
    add("md-real-D13-above-1.85", _problem("mdre+", 13, 3, MD_N, 2, "real", "sum", MM8_THETA * (1 + EDGE)), "md_real", "mm8+1", MD_OPTS, kernel="md-real-D13-K3")
    # ---- mid-D, complex instance ----
    for D in (13, 27, 36):
        add(f"md-herm-D{D}-e4n+0", _problem("mdh4", D, 2, MD_N, 2, "herm", "sum", T_E4N), "md_normal", "e4n+0", MD_OPTS, kernel=f"md-cplx-D{D}")
        add(f"md-herm-D{D}-t18n+0", _problem("mdh18", D, 2, MD_N, 2, "herm", "sum", T_T18N, phase=True), "md_normal", "t18n+0", MD_OPTS, kernel=f"md-cplx-D{D}")
        add(f"md-nonherm-D{D}-t18+0", _problem("mdn18", D, 2, MD_N, 2, "nonherm", "sum", T_T18), "md_general", "t18+0", MD_OPTS, kernel=f"md-cplx-D{D}")
        add(f"md-nonherm-D{D}-ps12+0", _problem("mdnps", D, 2, MD_N, 2, "nonherm", "sum", T_PS12), "md_general", "ps12+0", MD_OPTS, kernel=f"md-cplx-D{D}")
    add("md-herm-D13-dUs", _problem("mdh4", 13, 2, MD_N, 2, "herm", "sum", T_E4N), "md_normal", "e4n+0", MD_OPTS, dUs=True)

    # ---- 41 and above, unitary (published T18; the bound is the sum of norms) ----
    for D, scheme, ham in ((49, "t18+0", "herm"), (65, "t18+1", "real"), (81, "t18+0", "herm"), (41, "t18+0", "herm"), (60, "t18+0", "real"), (52, "t18+1", "herm"), (92, "t18+0", "herm"), (96, "t18+0", "herm")):
        t = T_T18 if scheme == "t18+0" else T_T18_1
        add(f"big-D{D}-{scheme}", _problem("big", D, 2, 6, 2, ham, "sum", t, phase=(D == 49), hk_scale=0.1), "t18", scheme)
    add("big-D49-no_regd", _problem("big", 49, 2, 6, 2, "herm", "sum", T_T18, phase=True, hk_scale=0.1), "t18", "t18+0", (("no_regd", 1),))

    # ---- Lindblad ----
    LSD = (("smalld_segments", 8),)
    for D in (2, 3, 4):
        k = f"lind-smallr-D{D}"
        add(f"lind-smallr-D{D}-e4n+0", _problem("lsr4", D, 2, 40, 3, "herm", "hb", T_E4N, lind=(1, 0.05, False)), "hb_small", "e4n+0", LSD, kernel=k)
        add(f"lind-smallr-D{D}-t18n+0", _problem("lsr18n", D, 2, 40, 3, "herm", "hb", T_T18N, lind=(2, 0.05, False)), "hb_small", "t18n+0", LSD, kernel=k)
        add(f"lind-smallr-D{D}-t18+0", _problem("lsr18", D, 2, 40, 3, "herm", "hb", T_T18, lind=(1, 2.0, False)), "hb_small", "t18+0", LSD, kernel=k)
    add("lind-D3-no_smallr", _problem("lsr4", 3, 2, 40, 3, "herm", "col", T_T18, lind=(1, 0.05, False)), "sd_general", "t18+0", LSD + (("no_smallr", 1),))
    add("lind-D3-nonherm", _problem("lsn", 3, 2, 40, 3, "nonherm", "col", T_T18, lind=(1, 0.05, False)), "sd_general", "t18+0", LSD)
    add("lind-D3-per-sample-col", _problem("lsrps", 3, 2, 40, 3, "herm", "hb", T_E4N, lind=(2, 0.05, True)), "hb_small", "e4n+0", LSD)
    add("lind-D4-mid", _problem("lmd", 4, 2, 12, 2, "herm", "hb", T_E4N, lind=(1, 0.05, False)), "hb_small", "e4n+0")
    add("lind-D4-no_smallr", _problem("lmd", 4, 2, 12, 2, "herm", "sum", T_T18, lind=(1, 0.05, False)), "md_general", "t18+0", (("no_smallr", 1),))
    for D in (5, 6):
        add(f"lind-D{D}-mid", _problem("lmd", D, 2, 12, 2, "herm", "sum", T_T18, lind=(1, 0.05, False)), "md_general", "t18+0")
    for D, scheme, rate in ((7, "t18n+0", 0.05), (7, "t18+0", 3.0), (7, "t18n+1", 0.05), (8, "t18n+0", 0.05), (9, "t18n+0", 0.05), (9, "t18+0", 3.0)):
        t = {"t18n+0": T_T18N_HI, "t18+0": T_T18, "t18n+1": T_T18N_1}[scheme]
        add(f"lind-regr-D{D}-{scheme}", _problem("lrr" + scheme, D, 2, 4, 2, "herm", "hb", t, lind=(1, rate, False), hk_scale=0.1), "hb_reg", scheme, kernel=f"lind-regr-D{D}")
    add("lind-D7-no_hermitian_basis", _problem("lrrt18n+0", 7, 2, 4, 2, "herm", "sum", T_T18, lind=(1, 0.05, False), hk_scale=0.1), "t18", "t18+0", (("no_hermitian_basis", 1),))
    add("lind-D7-nonherm", _problem("lrn", 7, 2, 4, 2, "nonherm", "sum", T_T18, lind=(1, 0.05, False), hk_scale=0.1), "t18", "t18+0")
    add("lind-D7-per-sample-col", _problem("lrrps", 7, 2, 4, 2, "herm", "hb", T_T18N_HI, lind=(2, 0.02, True), hk_scale=0.1), "hb_reg", "t18n+0")
    add("lind-D10-tiled", _problem("lt", 10, 2, 3, 1, "herm", "sum", T_T18, lind=(1, 0.05, False), hk_scale=0.1), "t18", "t18+0")

    # ---- branch B: one Hamiltonian per slice (supplied-generator instances of the chain kernels) ----
    add("per-slice-D9", _problem("psl", 9, 2, SD_N, 3, "herm", "slice", T_T18, phase=True, per_slice=True), "xg_general", "t18+0", SD_OPTS)
    add("per-slice-D27", _problem("psl", 27, 2, MD_N, 2, "herm", "slice", T_T18_1, per_slice=True), "xg_general", "t18+1", MD_OPTS)
    add("per-slice-lind-D3", _problem("pslL", 3, 2, 40, 2, "herm", "slice", T_T18, lind=(1, 0.05, False), per_slice=True), "xg_general", "t18+0", LSD)
    add("per-slice-lind-D7", _problem("pslL", 7, 2, 4, 2, "herm", "slice", T_T18, lind=(1, 0.05, False), per_slice=True, hk_scale=0.1), "xg_t18", "t18+0")
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
