"""Cases of the extended-precision tests of the PWC signal gradients (`propagate_batch_vjp`, `propagate_batch_lindblad_vjp`,
`propagate_batch_goal_vjp`, `propagate_per_slice_vjp`), next to tests/pwc_cases.py and on its machinery.

One case = one library call: a problem of pwc_cases (operators and amplitudes are `pwc_inputs`' own draw, untouched), a cotangent
U_bar (complex Gaussian from a generator of its own, keyed by the problem tag), the bound that fixes dt (`bound`, `target`), the
backward sweep it is expected to run in (`family`, `kernel`) and the polynomial scheme it claims there.  The sweeps are not the
forward kernels run backwards: their plans are restated in `grad_scheme_of` from c3p_smalld.hip, c3p_midd.hip, c3p_smallr.hip,
c3p_regrg_body.inc, c3p_grad.hip and c3p_tiled.hip.  tests/test_grad_extended_ref.py asserts, without a GPU, that the bound of
every SEGMENT of the pinned segmentation lies in the band the case claims, and the conditions that keep the yardstick e_cpu honest.

dt is rescaled per case: every bound is linear in dt, so dt = target / (largest sample bound at dt = 1).  Cases that share
(problem, bound, target) share inputs and reference (the launch forms: no_real_grad, a forced Taylor degree, both goal kinds).
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

import extended_ref as x
import pwc_cases as pc
from pwc_cases import EDGE, MM6_THETA, MM8_THETA, T18_THETA, T18N_MAX_NONNORMAL, T18N_THETA, _problem, squarings

REGRG_THETA = x.Q4_THETA[1:]  # c3p_regrg_body.inc: Taylor degree 8, 12, 16, 20
SDG_MAXS = 3  # c3p_smalld.hip


def midd_maxs(D: int) -> int:
    """MGR<NIG>::MAXS of c3p_midd.hip: NIG = ceil(ceil(D / 2) / 4) row groups; two squarings up to D = 32, one above."""
    nig = ((D + 1) // 2 + 3) // 4
    return 1 if (nig + 1) // 2 >= 3 else 2


# backward sweep -> the bound it plans with
#   "col":    column-wise bound of the tables (the real small-D sweep: the forward kernel's own)
#   "sum":    sum of the tables' 1-norms
#   "sumT":   the same of the tables of X^H (the general sweeps exponentiate X^H: row sums of X)
#   "hbT":    sum of the 1-norms of the TRANSPOSED real generators in the Hermitian basis, and their symmetric part
#   "slice":  per SLICE, ||X_n^H - i Im tr / D||_1 (vector-unit sweeps: every slice has its own squaring count)
#   "seg":    max over the segment's slices of the same (supplied generators: branch B)
FAMILY_BOUND = {"sdg_real": "col", "sdg_pair": "sum", "sdg_general": "sumT", "sdg_xg": "seg", "mdg_real": "sum", "mdg_pair": "sum",
                "mdg_general": "sumT", "mdg_xg": "seg", "hbg_small": "hbT", "hbg_reg": "hbT", "valu": "slice", "tiled": "sum"}


def regr_plan(nrm: float, degree: int = 0):
    """regr_grad_kernel: (degree, squarings) with the fewest products 3 J + 3 s, J = degree / 2 - 1; the lower degree on a tie."""
    best = None
    for i, th in enumerate(REGRG_THETA):
        J = 3 + 2 * i
        if degree and degree != 2 * J + 2:
            continue
        s = squarings(nrm, th)
        if best is None or 3 * J + 3 * s < best[0]:
            best = (3 * J + 3 * s, 2 * J + 2, s)
    return best[1], best[2]


def grad_scheme_of(family: str, bound: float, nsym: float = 0.0, D: int = 0, degree: int = 0) -> str:
    """The polynomial pair and squarings a backward sweep of `family` takes at `bound`; "handover" where the real sweep leaves
    the wave to the complex one."""
    if family in ("sdg_real", "mdg_real"):
        s = squarings(bound, MM8_THETA)
        if s > (SDG_MAXS if family == "sdg_real" else midd_maxs(D)):
            return "handover"
        return f"{'mm6' if family == 'sdg_real' and s == 0 and bound <= MM6_THETA else 'mm8'}+{s}"
    if family in ("sdg_pair", "sdg_general", "sdg_xg", "mdg_pair", "mdg_general", "mdg_xg", "valu", "tiled"):
        return f"t18+{squarings(bound, T18_THETA)}"
    if family == "hbg_small":
        econ = nsym <= T18N_MAX_NONNORMAL
        return f"{'t18n' if econ else 't18'}+{squarings(bound, T18N_THETA if econ else T18_THETA)}"
    if family == "hbg_reg":
        return "ty%d+%d" % regr_plan(bound, degree)
    raise ValueError(family)


# call: "vjp" | "lind" | "goal" | "per_slice";  S: segments per sample of the backward sweep as the options pin them (or, where no
# option reaches the rule, as the rule gives them: min(.., N / 8), never shorter than eight slices)
# handover: the family and scheme of the sweep that takes the waves the real sweep leaves
# goal: None | (kind, dims, index)
# variant: "" | "cancel" | "per_sample_h0": what `grad_inputs` does to the draw of pwc_inputs (below)
GradCase = namedtuple("GradCase", "id problem bound target family scheme call S opts kernel handover goal variant degree")
GradKey = namedtuple("GradKey", "problem bound target variant goal")


def key_of(c: GradCase) -> GradKey:
    return GradKey(c.problem, c.bound, c.target, c.variant, c.goal)


def _shift_im(G):
    D = G.shape[-1]
    return G - 1j * (np.trace(G).imag / D) * np.eye(D)


def bound_of(kind: str, tables, cmax, D: int):
    """(bound, symmetric part) of one sample or segment: tables [G_0 .. G_K] at the case's dt, cmax[K] = max_t |c_k(t)| there."""
    w = [1.0] + [float(c) for c in cmax]
    if kind == "hbT":
        T = pc.hb_transform(D)
        Gp = [(T @ G @ T.conj().T) for G in tables]
        assert all(np.abs(g.imag).max() <= 1e-13 * max(1.0, np.abs(g).max()) for g in Gp), "generator not real in the Hermitian basis"
        Gp = [g.real.T for g in Gp]
        return sum(a * x.norm1(g) for a, g in zip(w, Gp)), sum(a * x.norm1((g + g.T) / 2) for a, g in zip(w, Gp))
    S = [_shift_im(G.conj().T if kind == "sumT" else G) for G in tables]
    if kind == "col":
        return float(sum(a * np.abs(g).sum(axis=0) for a, g in zip(w, S)).max()), 0.0
    if kind in ("sum", "sumT"):
        return sum(a * x.norm1(g) for a, g in zip(w, S)), 0.0
    raise ValueError(kind)


GradInputs = namedtuple("GradInputs", "h0 hks signals dt col fr_phase U_bar ideal")


def _sample(a, b, base_ndim):
    return a[b] if a is not None and a.ndim > base_ndim else a


def sample_tables(inp: GradInputs, b: int, dt: float):
    return pc.generator_tables(_sample(inp.h0, b, 2), _sample(inp.hks, b, 3), dt, _sample(inp.col, b, 3))


def slice_norms(inp: GradInputs, lind: bool):
    """[B, N]: ||X_n^H - i Im tr / D||_1 of every slice (double)."""
    X = pc.slice_generators(inp, lind)
    return np.array([[x.device_norm(X[b, n].conj().T) for n in range(X.shape[1])] for b in range(X.shape[0])])


def segments(N: int, S: int):
    return [((g * N) // S, ((g + 1) * N) // S) for g in range(S)]


def segment_bounds(c: GradCase, inp: GradInputs, family: str = None):
    """[(sample, n0, n1, bound, symmetric part)] over the segments of the case's segmentation, by the bound of `family` (the
    case's own by default); per slice for the vector-unit sweeps."""
    p = c.problem
    kind = FAMILY_BOUND[family or c.family]
    lind = p.lind is not None
    out = []
    if kind in ("slice", "seg"):
        nrm = slice_norms(inp, lind)
        for b in range(p.B):
            for n0, n1 in (segments(p.N, p.N) if kind == "slice" else segments(p.N, c.S)):
                out.append((b, n0, n1, float(nrm[b, n0:n1].max()), 0.0))
        return out
    for b in range(p.B):
        tables = sample_tables(inp, b, inp.dt)
        for n0, n1 in segments(p.N, c.S):
            cmax = np.abs(inp.signals[b, :, n0:n1]).max(axis=1) if p.K else np.zeros(0)
            out.append((b, n0, n1) + tuple(bound_of(kind, tables, cmax, p.D)))
    return out


def _ubar(p, Dm):
    rng = np.random.default_rng([zlib.crc32(("ubar:" + p.tag).encode()), p.D, p.K, p.N, p.B])
    return rng.normal(size=(p.B, Dm, Dm)) + 1j * rng.normal(size=(p.B, Dm, Dm))


def _ideal(p, L):
    rng = np.random.default_rng([zlib.crc32(("ideal:" + p.tag).encode()), p.D, L])
    q, _ = np.linalg.qr(rng.normal(size=(L, L)) + 1j * rng.normal(size=(L, L)))
    return q


@functools.lru_cache(maxsize=None)
def grad_inputs(k: GradKey) -> GradInputs:
    p = k.problem
    base = pc.pwc_inputs(p)
    Dm = p.D * p.D if p.lind else p.D
    h0, hks, sig, col = base.h0, base.hks, base.signals, base.col
    if k.variant == "per_sample_h0":
        # one real drift per sample (a diagonal detuning that grows with the sample index), shared drives: per-sample tables on the real sweep
        assert h0.ndim == 2 and not p.per_slice and p.ham == "real"
        h0 = np.stack([h0 + 0.1 * b * np.diag(np.linspace(-1.0, 1.0, p.D)) for b in range(p.B)])
    if k.variant == "cancel":
        # the second drive repeats the first with 0.9 of its amplitude and the opposite sign: the bound adds 1.9 ||G_1||, the slices
        # carry 0.1 c_1 h_1 -- a bound far above the radius of Pade-13 with every slice well inside it
        assert p.K >= 2 and hks.ndim == 3 and not p.per_slice
        hks = hks.copy()
        hks[1] = hks[0]
        sig = sig.copy()
        sig[:, 1, :] = -0.9 * sig[:, 0, :]
    tmp = GradInputs(h0, hks, sig, 1.0, col, base.fr_phase, None, None)
    if p.per_slice:
        dt = base.dt  # every slice was scaled to its own norm at this dt
        assert k.bound == "seg" and abs(base.bounds.max() - k.target) <= 1e-12 * k.target
    elif k.bound == "slice":
        dt = k.target / slice_norms(tmp, p.lind is not None).max()
    else:
        dt = k.target / max(bound_of(k.bound, sample_tables(tmp, b, 1.0), np.abs(sig[b]).max(axis=1) if p.K else np.zeros(0), p.D)[0] for b in range(p.B))
    ideal = _ideal(p, 2 ** len(k.goal[2])) if k.goal else None
    out = GradInputs(h0, hks, sig, float(dt), col, base.fr_phase, None if k.goal else _ubar(p, Dm), ideal)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# references and the CPU yardstick
# ---------------------------------------------------------------------------------------------------------------------------
GradRef = namedtuple("GradRef", "g gph U_bar e_cpu e_oracle e_scipy e_cpu_ph floor")


def _fro(a):
    return float(np.sqrt((np.abs(a) ** 2).sum()))


def goal_rows(dims, index):
    from oracle import c3_oracle as o

    Pm = np.asarray(o.projector(list(dims), list(index)))
    return np.array([int(np.flatnonzero(Pm[:, j])[0]) for j in range(Pm.shape[1])])


def goal_cotangent(U, ideal, rows, kind):
    """U_bar[B, D, D] of the goal 1 - |s / L|^2 (unitary) or 1 - (|s|^2 / L + 1) / (L + 1) (average), s = sum conj(G_ac) U[r_a, r_c]
    (`extended_ref.infid_ld`), in the precision of U: d goal = Re sum conj(U_bar) dU, U_bar[r_a, r_c] = -2 c s G_ac."""
    L = len(rows)
    cplx = x.CLD if U.dtype == x.CLD else np.complex128
    G = np.asarray(ideal).astype(cplx)
    c = (x.LD(1) if U.dtype == x.CLD else 1.0) / (L * L if kind == "unitary" else L * (L + 1))
    out = np.zeros(U.shape, dtype=cplx)
    for b in range(U.shape[0]):
        s = (U[b][rows[:, None], rows[None, :]] * np.conj(G)).sum()
        out[b][rows[:, None], rows[None, :]] = -2 * c * s * G
    return out


def phase_gradient(U, U_bar):
    """d loss / d fr_phase[b, i] = Re sum_j conj(U_bar_ij) i U_ij = -Im sum_j conj(U_bar_ij) U_ij (U carries the row phases)."""
    return -(np.conj(U_bar) * U).sum(axis=-1).imag


def scipy_signal_gradient(X, Gk, lam):
    """The second double-precision route, one sample: scipy.linalg.expm per slice, double prefix products and running adjoint,
    scipy.linalg.expm_frechet of X^H with the slice cotangent; returns Z[N, Dm, Dm] (Gk None) or g[K, N]."""
    import scipy.linalg

    N, Dm = X.shape[0], X.shape[-1]
    dUs = [scipy.linalg.expm(X[n]) for n in range(N)]
    P = [np.eye(Dm, dtype=np.complex128)]
    for n in range(N - 1):
        P.append(dUs[n] @ P[-1])
    Z = np.empty_like(X)
    for n in range(N - 1, -1, -1):
        Z[n] = scipy.linalg.expm_frechet(X[n].conj().T, lam @ P[n].conj().T, compute_expm=False)
        lam = dUs[n].conj().T @ lam
    if Gk is None:
        return Z
    return np.stack([(np.conj(Z) * G[None]).sum(axis=(-2, -1)).real for G in Gk]) if len(Gk) else np.zeros((0, N))


@functools.lru_cache(maxsize=None)
def grad_reference(k: GradKey) -> GradRef:
    """Long-double gradient of a problem (once per process, read-only) and the errors of the two double-precision CPU routes
    against it: the oracle's gradient, and the scipy route.  e_cpu: the worst of both over the samples of max|g - ref| / max|ref|."""
    from oracle import c3_oracle as o

    p, inp = k.problem, grad_inputs(k)
    lind = p.lind is not None
    B, D = p.B, p.D
    hb = lambda b: _sample(inp.h0, b, 2)
    kb = lambda b: _sample(inp.hks, b, 3)
    cb = lambda b: _sample(inp.col, b, 3)
    phb = lambda b: None if inp.fr_phase is None else inp.fr_phase[b]
    X = pc.slice_generators(inp, lind)
    gph = e_ph = None
    if k.goal:
        kind, dims, index = k.goal
        rows = goal_rows(dims, index)
        U_ld = x.pwc_ld(inp.h0, inp.hks, inp.signals, inp.dt, fr_phase=inp.fr_phase)
        Ubar_ld = goal_cotangent(U_ld, inp.ideal, rows, kind)
        g = x.pwc_signal_gradient_ld(inp.h0, inp.hks, inp.signals, inp.dt, Ubar_ld, fr_phase=inp.fr_phase)
        gph = phase_gradient(U_ld, Ubar_ld)
        # the double routes form their own cotangent from their own propagator, as a caller of the three-call form does
        U_d = o.propagate_batch(inp.h0, inp.hks, inp.signals, inp.dt, fr_phase=inp.fr_phase)
        Ubar_d = goal_cotangent(U_d, inp.ideal, rows, kind)
        import scipy.linalg

        U_s = np.stack([o.tf_matmul_n(np.stack([scipy.linalg.expm(Xn) for Xn in X[b]])) for b in range(B)])
        if inp.fr_phase is not None:
            U_s = np.exp(1j * inp.fr_phase)[:, :, None] * U_s
        e_ph = max(x.grad_err(phase_gradient(U_d, Ubar_d), gph), x.grad_err(phase_gradient(U_s, goal_cotangent(U_s, inp.ideal, rows, kind)), gph))
        Ubar = Ubar_d
        Ubar_ref = Ubar_ld
    else:
        Ubar = Ubar_ref = inp.U_bar
        if p.per_slice:
            g = x.pwc_per_slice_cotangents_ld(inp.h0, inp.dt, Ubar, fr_phase=inp.fr_phase)
        else:
            g = x.pwc_signal_gradient_ld(inp.h0, inp.hks, inp.signals, inp.dt, Ubar, col_ops=inp.col, fr_phase=inp.fr_phase)
    rows_adj = np.ones((B, X.shape[-1])) if inp.fr_phase is None else np.exp(-1j * inp.fr_phase)
    go, gs = [], []
    for b in range(B):
        lam = rows_adj[b][:, None] * Ubar[b]
        if p.per_slice:
            go.append(o.pwc_per_slice_hamiltonian_cotangents(inp.h0[b], inp.dt, Ubar[b], phb(b)))
            gs.append(1j * inp.dt * scipy_signal_gradient(X[b], None, lam))
        elif lind:
            go.append(o.pwc_lindblad_signal_gradient(hb(b), kb(b), cb(b), inp.signals[b], inp.dt, Ubar[b], phb(b)))
            one = np.eye(D)
            gs.append(scipy_signal_gradient(X[b], [-1j * inp.dt * (np.kron(h, one) - np.kron(one, h.T)) for h in kb(b)], lam))
        else:
            go.append(o.pwc_signal_gradient(hb(b), kb(b), inp.signals[b], inp.dt, Ubar[b], phb(b)))
            gs.append(scipy_signal_gradient(X[b], [-1j * inp.dt * h for h in kb(b)], lam))
    e_o, e_s = x.grad_err(np.stack(go), g), x.grad_err(np.stack(gs), g)
    # floor: the largest entry per sample against ||U_bar||_F dt max_k ||h_k||_F (Lindblad: dt ||h_k (x) 1 - 1 (x) h_k^T||_F; branch B: dt)
    if p.per_slice:
        gen = [inp.dt] * B
    elif lind:
        one = np.eye(D)
        gen = [inp.dt * max(_fro(np.kron(h, one) - np.kron(one, h.T)) for h in kb(b)) for b in range(B)]
    else:
        gen = [inp.dt * max(_fro(h) for h in kb(b)) for b in range(B)]
    floor = min(float(np.abs(g[b]).max()) / (_fro(Ubar_ref[b]) * gen[b]) for b in range(B))
    for a in (g, gph):
        if a is not None:
            a.setflags(write=False)
    return GradRef(g, gph, Ubar_ref, max(e_o, e_s), e_o, e_s, e_ph, floor)


# ---------------------------------------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------------------------------------
SD_N, SD_S = pc.SD_N, pc.SD_S  # N = 131 on 32 segments of four or five slices
SD_OPTS = pc.SD_OPTS
MD_N = pc.MD_N  # one segment of 70 slices
VG_N = 34  # vector-unit sweeps on the Lindblad superoperators: four segments of eight or nine slices
LSD = (("smalld_segments", 8),)  # N = 40: segments of five slices


def _cases():
    cs = []

    def add(id_, prob, bound, target, family, scheme, call="vjp", S=1, opts=(), kernel=None, handover=None, goal=None, cancel=False, degree=0, variant=""):
        cs.append(GradCase(id_, prob, bound, float(target), family, scheme, call, S, tuple(opts), kernel or id_, handover, goal, "cancel" if cancel else variant, degree))

    below = lambda r: r * (1 - EDGE)
    above = lambda r: r * (1 + EDGE)
    # ---- small-D real sweep: smalld_grad_real_kernel<D> (column-wise bound; degree 6 below 0.83, degree 8 with up to three squarings)
    real_bands = (("mm6+0", 0.9 * MM6_THETA), ("mm8+0", 0.9 * MM8_THETA), ("mm8+1", 1.1 * MM8_THETA), ("mm8+2", 1.1 * 2 * MM8_THETA), ("mm8+3", 1.1 * 4 * MM8_THETA))
    sd = lambda tag, D, K=2, B=3, ham="real", **kw: _problem(tag, D, K, SD_N, B, ham, "col", 1.0, **kw)
    for D in (5, 9):
        kern = f"sdg-real-D{D}"
        for scheme, t in real_bands:
            add(f"sdg-real-D{D}-K2-{scheme}", sd("g" + scheme, D), "col", t, "sdg_real", scheme, S=SD_S, opts=SD_OPTS, kernel=kern, cancel=(scheme == "mm8+3"))
        add(f"sdg-real-D{D}-K3-mm6+0", sd("gK3a", D, 3), "col", real_bands[0][1], "sdg_real", "mm6+0", S=SD_S, opts=SD_OPTS, kernel=kern)
        add(f"sdg-real-D{D}-K3-mm8+1", sd("gK3b", D, 3), "col", real_bands[2][1], "sdg_real", "mm8+1", S=SD_S, opts=SD_OPTS, kernel=kern)
        add(f"sdg-real-D{D}-trace-phase", sd("gtr", D, trace=1.5, phase=True), "col", real_bands[0][1], "sdg_real", "mm6+0", S=SD_S, opts=SD_OPTS, kernel=kern)
    for D in (3, 4, 8, 12):
        for scheme, t in (real_bands[0], real_bands[2]) if D in (3, 8) else (real_bands[1], real_bands[3]):
            add(f"sdg-real-D{D}-{scheme}", sd("gp" + scheme, D, phase=(D == 8)), "col", t, "sdg_real", scheme, S=SD_S, opts=SD_OPTS, kernel=f"sdg-real-D{D}")
    for edge, lo, hi, cancel in ((MM6_THETA, "mm6+0", "mm8+0", False), (MM8_THETA, "mm8+0", "mm8+1", False), (2 * MM8_THETA, "mm8+1", "mm8+2", False),
                                 (4 * MM8_THETA, "mm8+2", "mm8+3", True)):
        add(f"sdg-real-D9-below-{edge:g}", sd("ge-", 9, B=2), "col", below(edge), "sdg_real", lo, S=SD_S, opts=SD_OPTS, kernel="sdg-real-D9", cancel=cancel)
        add(f"sdg-real-D9-above-{edge:g}", sd("ge+", 9, B=2), "col", above(edge), "sdg_real", hi, S=SD_S, opts=SD_OPTS, kernel="sdg-real-D9", cancel=cancel)
    # the hand-over: above 8 x 1.85 every wave of the launch is left to the complex pair sweep (which plans with the sum of norms)
    add("sdg-real-D9-below-14.8", sd("ge-", 9, B=2), "col", below(8 * MM8_THETA), "sdg_real", "mm8+3", S=SD_S, opts=SD_OPTS, kernel="sdg-real-D9", cancel=True)
    add("sdg-real-D9-above-14.8", sd("ge+", 9, B=2), "col", above(8 * MM8_THETA), "sdg_real", "handover", S=SD_S, opts=SD_OPTS, kernel="sdg-real-D9-handover",
        cancel=True, handover=("sdg_pair", "t18+4"))
    # one complex sample (sample 1) among real ones, per-sample operators: its waves go to the complex pair sweep
    add("sdg-mixed-D9", sd("gmix", 9, ham="mixed"), "col", real_bands[1][1], "sdg_real", "mm8+0", S=SD_S, opts=SD_OPTS, handover=("sdg_pair", "t18+1"))
    add("sdg-mixed-D9-trace-phase", sd("gmix", 9, ham="mixed", trace=1.5, phase=True), "col", real_bands[1][1], "sdg_real", "mm8+0", S=SD_S, opts=SD_OPTS,
        handover=("sdg_pair", "t18+1"))
    # per-sample drifts, all real: per-sample tables on the real sweep alone
    for D, (scheme, t) in ((9, real_bands[0]), (9, real_bands[1]), (5, real_bands[1])):
        add(f"sdg-real-D{D}-per-sample-h0-{scheme}", sd("gps", D), "col", t, "sdg_real", scheme, S=SD_S, opts=SD_OPTS, kernel=f"sdg-real-D{D}-per-sample-h0", variant="per_sample_h0")
    # the same problem and reference as sdg-real-D9-K2-mm8+0 on the complex pair sweep
    add("sdg-real-D9-no_real_grad", sd("gmm8+0", 9), "col", real_bands[1][1], "sdg_pair", "t18+1", S=SD_S, opts=SD_OPTS + (("no_real_grad", 1),))

    # ---- small-D complex pair: smalld_grad_kernel<D> (sum of norms, published T18)
    t18_bands = (("t18+0", 0.9 * T18_THETA), ("t18+1", 1.1 * T18_THETA), ("t18+2", 1.1 * 2 * T18_THETA))
    for D in (3, 9, 12):
        for scheme, t in t18_bands:
            add(f"sdg-herm-D{D}-{scheme}", sd("gh" + scheme, D, ham="herm", phase=(scheme == "t18+1")), "sum", t, "sdg_pair", scheme, S=SD_S, opts=SD_OPTS, kernel=f"sdg-herm-D{D}")
    # the trace shift and the row phases on the complex pair sweep (same band as sdg-herm-D9-t18+1)
    add("sdg-herm-D9-trace", sd("ghtr", 9, ham="herm", trace=1.5), "sum", t18_bands[1][1], "sdg_pair", "t18+1", S=SD_S, opts=SD_OPTS, kernel="sdg-herm-D9-trace")
    add("sdg-herm-D9-trace-phase", sd("ghtr", 9, ham="herm", trace=1.5, phase=True), "sum", t18_bands[1][1], "sdg_pair", "t18+1", S=SD_S, opts=SD_OPTS,
        kernel="sdg-herm-D9-trace-phase")
    for edge, lo, hi in ((T18_THETA, "t18+0", "t18+1"), (2 * T18_THETA, "t18+1", "t18+2")):
        add(f"sdg-herm-D9-below-{edge:g}", sd("ghe-", 9, B=2, ham="herm"), "sum", below(edge), "sdg_pair", lo, S=SD_S, opts=SD_OPTS, kernel="sdg-herm-D9")
        add(f"sdg-herm-D9-above-{edge:g}", sd("ghe+", 9, B=2, ham="herm"), "sum", above(edge), "sdg_pair", hi, S=SD_S, opts=SD_OPTS, kernel="sdg-herm-D9")

    # ---- small-D general sweep: smalld_grad_general_kernel (Lindblad D = 3; branch B)
    lsd = lambda tag, D, ham="herm", lind=(1, 0.05, False): _problem(tag, D, 2, 40, 3, ham, "col", 1.0, lind=lind)
    add("lindg-D3-nonherm", lsd("gln", 3, "nonherm"), "sumT", t18_bands[0][1], "sdg_general", "t18+0", "lind", 8, LSD)
    add("lindg-D3-no_smallr", lsd("gls", 3), "sumT", t18_bands[1][1], "sdg_general", "t18+1", "lind", 8, LSD + (("no_smallr", 1),))
    add("per-slice-grad-D9", _problem("gpsl", 9, 2, SD_N, 3, "herm", "slice", t18_bands[0][1], phase=True, per_slice=True), "seg", t18_bands[0][1], "sdg_xg", "t18+0",
        "per_slice", SD_S, SD_OPTS)

    # ---- mid-D real sweep: midd_grad_real_kernel (sum of norms; degree 8, two squarings up to D = 32, one above; K <= 3)
    md = lambda tag, D, K=3, B=2, ham="real", **kw: _problem(tag, D, K, MD_N, B, ham, "sum", 1.0, **kw)
    mdo = lambda B: (("grad_target", B),)
    for D in (13, 16, 17, 27, 36, 40):
        B = 2 if D <= 17 else 1
        for s in range(midd_maxs(D) + 1):
            add(f"mdg-real-D{D}-mm8+{s}", md("gmr%d" % s, D, B=B, phase=(D == 17)), "sum", (0.9 if s == 0 else 1.1) * MM8_THETA * 2.0 ** max(s - 1, 0), "mdg_real", f"mm8+{s}",
                opts=mdo(B), kernel=f"mdg-real-D{D}")
    for D, edge, lo, hi in ((13, MM8_THETA, "mm8+0", "mm8+1"), (13, 2 * MM8_THETA, "mm8+1", "mm8+2")):
        add(f"mdg-real-D{D}-below-{edge:g}", md("gmre-", D), "sum", below(edge), "mdg_real", lo, opts=mdo(2), kernel=f"mdg-real-D{D}")
        add(f"mdg-real-D{D}-above-{edge:g}", md("gmre+", D), "sum", above(edge), "mdg_real", hi, opts=mdo(2), kernel=f"mdg-real-D{D}")
    # the hand-over just above each row class's limit: the pair sweep plans with the same bound
    add("mdg-real-D13-below-7.4", md("gmre-", 13, K=2), "sum", below(4 * MM8_THETA), "mdg_real", "mm8+2", opts=mdo(2), kernel="mdg-real-D13", cancel=True)
    add("mdg-real-D13-above-7.4", md("gmre+", 13, K=2), "sum", above(4 * MM8_THETA), "mdg_real", "handover", opts=mdo(2), kernel="mdg-real-D13-handover", cancel=True,
        handover=("mdg_pair", "t18+3"))
    add("mdg-real-D36-below-3.7", md("gmre-", 36, B=1), "sum", below(2 * MM8_THETA), "mdg_real", "mm8+1", opts=mdo(1), kernel="mdg-real-D36")
    add("mdg-real-D36-above-3.7", md("gmre+", 36, B=1), "sum", above(2 * MM8_THETA), "mdg_real", "handover", opts=mdo(1), kernel="mdg-real-D36-handover",
        handover=("mdg_pair", "t18+2"))
    # ---- mid-D complex pair (Hermitian) and general sweep (Lindblad D = 4 no_smallr, 5, 6; branch B)
    for D in (13, 27, 36):
        B = 2 if D == 13 else 1
        for scheme, t in t18_bands[:2] if D > 13 else t18_bands:
            add(f"mdg-herm-D{D}-{scheme}", md("gmh" + scheme, D, K=2, B=B, ham="herm", phase=(scheme == "t18+1")), "sum", t, "mdg_pair", scheme, opts=mdo(B), kernel=f"mdg-herm-D{D}")
    lmd = lambda tag, D, ham="herm": _problem(tag, D, 2, 12, 2, ham, "sum", 1.0, lind=(1, 0.05, False))
    add("lindg-D4-no_smallr", lmd("glm", 4), "sumT", t18_bands[0][1], "mdg_general", "t18+0", "lind", 1, (("no_smallr", 1),))
    add("lindg-D4-nonherm", lmd("glmn", 4, "nonherm"), "sumT", t18_bands[1][1], "mdg_general", "t18+1", "lind", 1, kernel="lindg-D4-no_smallr")
    for D in (5, 6):
        add(f"lindg-D{D}-t18+0", lmd("glm", D), "sumT", t18_bands[0][1], "mdg_general", "t18+0", "lind", 1, kernel=f"lindg-D{D}")
        add(f"lindg-D{D}-t18+1", lmd("glm1", D), "sumT", t18_bands[1][1], "mdg_general", "t18+1", "lind", 1, kernel=f"lindg-D{D}")
    add("per-slice-grad-D27", _problem("gpsl", 27, 2, MD_N, 1, "herm", "slice", t18_bands[1][1], per_slice=True), "seg", t18_bands[1][1], "mdg_xg", "t18+1", "per_slice", 8)

    # ---- Hermitian-basis sweeps
    # smallr_grad_kernel<D^2>: T18N (radius 2) while the symmetric part stays below 0.25, else T18
    for D in (2, 3, 4):
        kern = f"lindg-smallr-D{D}"
        for scheme, t, lind in (("t18n+0", 0.9 * T18N_THETA, (2, 0.02, False)), ("t18n+1", 1.1 * T18N_THETA, (1, 0.01, False)), ("t18+0", 0.9 * T18_THETA, (1, 2.0, False)),
                                ("t18+1", 1.1 * T18_THETA, (1, 2.0, False))):
            add(f"lindg-smallr-D{D}-{scheme}", lsd("gsr" + scheme, D, lind=lind), "hbT", t, "hbg_small", scheme, "lind", 8, LSD, kernel=kern)
    add("lindg-smallr-D3-per-sample-col", lsd("gsrps", 3, lind=(2, 0.02, True)), "hbT", 0.9 * T18N_THETA, "hbg_small", "t18n+0", "lind", 8, LSD)
    # regr_grad_kernel<n>: Taylor pairs of degree 8 .. 20
    rg = lambda tag, D, lind=(1, 0.05, False): _problem(tag, D, 2, 4, 2, "herm", "hb", 1.0, lind=lind, hk_scale=0.1)
    for D in (7, 8, 9):
        kern = f"lindg-regr-D{D}"
        for deg, s in ((8, 3), (12, 0), (16, 0), (20, 0)):
            add(f"lindg-regr-D{D}-degree{deg}", rg("grf", D), "hbT", 0.9 * REGRG_THETA[1], "hbg_reg", f"ty{deg}+{s}", "lind", 1, (("regr_grad_degree", deg),), kernel=kern, degree=deg)
        add(f"lindg-regr-D{D}-ty12+1", rg("gr121", D), "hbT", 0.5, "hbg_reg", "ty12+1", "lind", 1, kernel=kern)
    for i, (lo, hi) in enumerate((("ty8+0", "ty8+1"), ("ty12+0", "ty8+3"), ("ty8+4", "ty8+4"), ("ty8+5", "ty8+5"))):
        add(f"lindg-regr-D7-below-{REGRG_THETA[i]:g}", rg("gre", 7), "hbT", below(REGRG_THETA[i]), "hbg_reg", lo, "lind", 1, kernel="lindg-regr-D7")
        add(f"lindg-regr-D7-above-{REGRG_THETA[i]:g}", rg("gre", 7), "hbT", above(REGRG_THETA[i]), "hbg_reg", hi, "lind", 1, kernel="lindg-regr-D7")
    add("lindg-regr-D7-ty8+2", rg("gr82", 7), "hbT", 0.15, "hbg_reg", "ty8+2", "lind", 1, kernel="lindg-regr-D7")
    add("lindg-regr-D7-ty12+2", rg("gr122", 7), "hbT", 1.0, "hbg_reg", "ty12+2", "lind", 1, kernel="lindg-regr-D7")
    add("lindg-regr-D8-per-sample-col", rg("grps", 8, lind=(2, 0.02, True)), "hbT", 0.9 * REGRG_THETA[1], "hbg_reg", "ty12+0", "lind", 1)

    # ---- vector-unit sweeps (every slice planned on its own norm) and the tiled sweep (one bound per launch)
    big = lambda tag, D, ham, N=6, B=2: _problem(tag, D, 2, N, B, ham, "sum", 1.0, phase=(D == 48), hk_scale=0.1)
    vgo = lambda S: (("valu_grad_segments", S),)
    for D, ham in ((41, "herm"), (48, "real"), (64, "herm")):
        for scheme, t in (("t18+0", 0.9 * T18_THETA), ("t18+1", 0.98 * 2 * T18_THETA)):
            add(f"valug-D{D}-{scheme}", big("gv" + scheme, D, ham), "slice", t, "valu", scheme, S=2, opts=vgo(2), kernel=f"valug-D{D}")
    for D, ham, N, B in ((65, "real", 4, 2), (96, "herm", 3, 1)):
        for scheme, t in t18_bands[:2]:
            add(f"tiledg-D{D}-{scheme}", big("gt" + scheme, D, ham, N, B), "sum", t, "tiled", scheme)
    for scheme, t in t18_bands[:2]:
        add(f"tiledg-lind-D10-{scheme}", _problem("gtl" + scheme, 10, 2, 3, 1, "herm", "sum", 1.0, lind=(1, 0.05, False), hk_scale=0.1), "sum", t, "tiled", scheme, "lind")
    for D in (3, 5):
        for scheme, t in (("t18+0", 0.9 * T18_THETA), ("t18+1", 0.98 * 2 * T18_THETA)):
            add(f"valug-lind-D{D}-{scheme}", _problem("gvl" + scheme, D, 2, VG_N, 2, "herm", "sum", 1.0, lind=(1, 0.05, False)), "slice", t, "valu", scheme, "lind", 4,
                vgo(4) + (("valu_grad", 1),), kernel=f"valug-lind-D{D}")

    # ---- fused goal: gradient and phase gradient, both kinds
    for kind in ("unitary", "average"):
        g9 = (kind, (3, 3), (0, 1))
        add(f"goal-D9-real-{kind}", sd("ggoal", 9, phase=True), "col", real_bands[1][1], "sdg_real", "mm8+0", "goal", SD_S, SD_OPTS, kernel="goal-D9-real", goal=g9)
        add(f"goal-D9-herm-{kind}", sd("ggoalh", 9, ham="herm", phase=True), "sum", t18_bands[1][1], "sdg_pair", "t18+1", "goal", SD_S, SD_OPTS, kernel="goal-D9-herm", goal=g9)
        add(f"goal-D48-{kind}", big("ggoal", 48, "herm"), "slice", 0.98 * 2 * T18_THETA, "valu", "t18+1", "goal", 2, vgo(2), kernel="goal-D48", goal=(kind, (6, 8), (0, 1)))
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
KEYS = sorted({key_of(c) for c in CASES}, key=lambda k: [c.id for c in CASES if key_of(c) == k][0])


# ---------------------------------------------------------------------------------------------------------------------------
# groups: what an expected failure of the GPU test may be declared for
# ---------------------------------------------------------------------------------------------------------------------------
def band_position(c: GradCase) -> str:
    """Where the case's bound lies in the band of its squaring count: q = bound / (radius 2^s) is in (1/2, 1] once s >= 1.  "lo" (q < 0.52:
    the scaled norm is just above half the radius -- the member of a pair just ABOVE an edge), "hi" (q > 0.98: just below an edge), else
    "mid" (the 10 %-inside targets, and every case without a squaring)."""
    if c.scheme == "handover":
        fam, scheme = c.handover
    else:
        fam, scheme = c.family, c.scheme
    s = int(scheme.split("+")[1])
    if s == 0 or c.bound == "slice":
        return "mid"
    if scheme.startswith("ty"):
        theta = REGRG_THETA[(int(scheme[2:].split("+")[0]) - 8) // 4]
    else:
        theta = {"mm8": MM8_THETA, "t18": T18_THETA, "t18n": T18N_THETA}[scheme.split("+")[0]]
    if FAMILY_BOUND[fam] != c.bound:
        return "mid"  # (the bound that fixed dt is not the one this sweep plans with: no edge was aimed at)
    q = c.target / (theta * 2.0**s)
    assert 0.5 < q <= 1.0, (c.id, q)
    return "lo" if q < 0.52 else ("hi" if q > 0.98 else "mid")


def group_of(c: GradCase):
    """(kernel class, scheme, position in the band, variant): computable without a GPU.  The expected failures of the GPU test are whole
    groups (tests/test_grad_extended_ref.py asserts that the listed cases are exactly the members of the listed groups)."""
    scheme = c.scheme + (">" + c.handover[1] if c.handover else "")
    return (c.kernel, scheme, band_position(c), c.variant)


def call_case(prop, _lib, c: GradCase, inp: GradInputs):
    """The library call of a case under its options: (gradient, phase gradient or None, launch log)."""
    p = c.problem
    gph = None
    with _lib.options(**dict(c.opts)):
        if c.call == "vjp":
            g = prop.propagate_batch_vjp(inp.h0, inp.hks, inp.signals, inp.dt, inp.U_bar, fr_phase=inp.fr_phase)
        elif c.call == "lind":
            g = prop.propagate_batch_lindblad_vjp(inp.h0, inp.hks, inp.signals, inp.dt, inp.col, inp.U_bar, fr_phase=inp.fr_phase)
        elif c.call == "per_slice":
            g = prop.propagate_per_slice_vjp(inp.h0, inp.dt, inp.U_bar, fr_phase=inp.fr_phase)
        elif c.call == "goal":
            kind, dims, index = c.goal
            r = prop.propagate_batch_goal_vjp(inp.h0, inp.hks, inp.signals, inp.dt, inp.ideal, list(index), list(dims), kind=kind, fr_phase=inp.fr_phase, want_U=False)
            g, gph = r["grad_signals"], np.asarray(r["grad_fr_phase"])
        else:
            raise ValueError(c.call)
        detail = _lib.last_kernel_detail()
    return np.asarray(g), gph, detail


# K = 0: no control line, so no signal gradient to hold to a bar; the gradient entry refuses these sizes (tests/test_gpu_grad_extended.py)
K0_CASE = GradCase("sdg-real-D9-K0", _problem("gK0", 9, 0, SD_N, 3, "real", "col", 1.0), "col", 0.9 * MM6_THETA, "sdg_real", "mm6+0", "vjp", SD_S, SD_OPTS,
                   "sdg-real-D9-K0", None, None, "", 0)

