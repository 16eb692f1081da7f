"""CPU tests of the extended-precision reference of the assembled PWC propagators (`extended_ref.pwc_ld`) and of the case list
of tests/test_gpu_pwc_extended.py (tests/pwc_cases.py).

* `pwc_ld` against 40-digit mpmath, unitary and Lindblad, with frame phases;
* its superoperator convention against `oracle.propagate_batch(..., lindbladian=True)`;
* for every GPU case: the inputs are a pure function of the case, every slice lies inside the radius of Pade-13 (above it the
  oracle's floor rule inflates e_cpu, and the bar 8 e_cpu would go slack), and the norm bound the device plans with -- restated
  in pwc_cases.norm_bound -- falls in the band of the scheme the case claims.
"""
import numpy as np
import pytest

import extended_ref as x
import pwc_cases as pc
from oracle import c3_oracle as o
from test_extended_ref import _ld_to_mp, _mp_matrix


def _mp_kron(mp, A, B):
    n, m = A.rows, B.rows
    out = mp.matrix(n * m, n * m)
    for i in range(n):
        for j in range(n):
            for p in range(m):
                for q in range(m):
                    out[i * m + p, j * m + q] = A[i, j] * B[p, q]
    return out


def _mp_pwc(mp, h0, hks, sig, dt, col, ph):
    """One sample in 40 digits: product over the slices (later slice on the left) of exp(-i dt H_n), or of exp(dt L(H_n))."""
    D = h0.shape[-1]
    one = mp.eye(D)
    U = None
    for n in range(sig.shape[1]):
        H = _mp_matrix(mp, h0)
        for k in range(sig.shape[0]):
            H = H + mp.mpf(float(sig[k, n])) * _mp_matrix(mp, hks[k])
        if col is None:
            X = mp.mpc(0, -1) * mp.mpf(dt) * H
        else:
            L = mp.mpc(0, -1) * (_mp_kron(mp, H, one) - _mp_kron(mp, one, H.T))
            for C in col:
                C = _mp_matrix(mp, C)
                CC = C.H * C
                L = L + _mp_kron(mp, C, C.conjugate()) - (_mp_kron(mp, CC, one) + _mp_kron(mp, one, CC.T)) / 2
            X = mp.mpf(dt) * L
        E = mp.expm(X)
        U = E if U is None else E * U
    if ph is not None:
        for i in range(U.rows):
            f = mp.expj(mp.mpf(float(ph[i])))
            for j in range(U.cols):
                U[i, j] = f * U[i, j]
    return U


@pytest.mark.parametrize("D,lind", [(2, False), (3, False), (2, True)], ids=["D2-unitary", "D3-unitary", "D2-lindblad"])
def test_pwc_ld_against_mpmath(D, lind):
    """The criterion `expm_ld` is held to, with the norms of the N = 3 slices added up (the first-order error of a product of
    exponentials is the sum of theirs): |pwc_ld - exact|_max <= 4 eps_ld max(1, sum_n ||X_n||_1) ||U||_max."""
    mp = pytest.importorskip("mpmath")
    rng = np.random.default_rng([D, int(lind)])
    B, K, N = 2, 2, 3
    h0 = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    h0 = (h0 + h0.conj().T) / 2 + 0.7 * np.eye(D)
    hks = rng.normal(size=(K, D, D)) + 1j * rng.normal(size=(K, D, D))  # not Hermitian: nothing is assumed of the operators
    sig = rng.uniform(-1, 1, size=(B, K, N))
    dt = 0.37
    col = 0.3 * (rng.normal(size=(2, D, D)) + 1j * rng.normal(size=(2, D, D))) if lind else None
    Dm = D * D if lind else D
    ph = rng.uniform(0, 6.28, size=(B, Dm))
    U = x.pwc_ld(h0, hks, sig, dt, col_ops=col, fr_phase=ph)
    X = x.pwc_generators_ld(h0, hks, sig, dt, col_ops=col)
    worst = 0.0
    with mp.workdps(40):
        for b in range(B):
            M = _mp_pwc(mp, h0, hks, sig[b], dt, col, ph[b])
            ref_max = max(abs(complex(M[i, j])) for i in range(Dm) for j in range(Dm))
            diff = max(abs(mp.mpc(_ld_to_mp(mp, U[b, i, j].real), _ld_to_mp(mp, U[b, i, j].imag)) - M[i, j]) for i in range(Dm) for j in range(Dm))
            worst = max(worst, float(diff) / (x.EPS_LD * max(1.0, sum(x.norm1(X[b, n]) for n in range(N))) * ref_max))
    print(f"pwc_ld vs mpmath D={D} lindblad={lind}: worst error / (eps_ld max(1, sum ||X_n||) ||U||max) = {worst:.3g}")
    assert worst <= 4.0


def test_pwc_ld_superoperator_convention():
    """`pwc_ld` with collapse operators is the oracle's Lindblad propagator (row-major vectorisation, `lindblad_generator`)."""
    rng = np.random.default_rng(11)
    D, B, K, N = 3, 2, 2, 5
    h0 = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    h0 = (h0 + h0.conj().T) / 2
    hks = rng.normal(size=(K, D, D)) + 1j * rng.normal(size=(K, D, D))
    hks = (hks + hks.conj().transpose(0, 2, 1)) / 2
    col = 0.2 * (rng.normal(size=(2, D, D)) + 1j * rng.normal(size=(2, D, D)))
    sig = rng.uniform(-1, 1, size=(B, K, N))
    ref = o.propagate_batch(h0, hks, sig, 0.2, col_ops=col, lindbladian=True)
    U, dUs = x.pwc_ld(h0, hks, sig, 0.2, col_ops=col, want_dUs=True)
    assert dUs.shape == (B, N, D * D, D * D)
    err = x.pwc_err(ref, U)
    print(f"oracle vs pwc_ld, Lindblad D=3: |U - U_ld|_F = {err:.3g}")
    assert err <= 1e-13
    # per-sample operators [B,D,D], [B,K,D,D], [B,C,D,D] and branch B give the same propagators
    Ub = x.pwc_ld(np.stack([h0] * B), np.stack([hks] * B), sig, 0.2, col_ops=np.stack([col] * B))
    assert np.array_equal(Ub, U)
    H = np.stack([o.sum_h0_hks(h0, hks, sig[b]) for b in range(B)])
    assert x.pwc_err(x.pwc_ld(H, None, None, 0.2, col_ops=col).astype(np.complex128), U) <= 1e-14


def test_plans_restate_the_header():
    """The radii of pwc_cases are the ones of c3p_common.h."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "c3_amd", "csrc", "c3p_common.h")).read()
    for name, v in (("C3P_MM6_THETA", pc.MM6_THETA), ("C3P_MM8_THETA", pc.MM8_THETA), ("C3P_T18_THETA", pc.T18_THETA), ("C3P_E4N_THETA", pc.E4N_THETA),
                    ("C3P_T18N_THETA", pc.T18N_THETA), ("C3P_T18N_MAX_NONNORMAL", pc.T18N_MAX_NONNORMAL)):
        assert float(re.search(r"#define %s\s+([0-9.eE+-]+)" % name, src).group(1)) == v, name
    th = re.search(r"c3p_pick_plan_q4.*?th\[5\] = \{([^}]*)\}", src, re.S).group(1)
    assert tuple(float(t) for t in th.split(",")) == pc.Q4_THETA


@pytest.mark.parametrize("c", pc.CASES, ids=pc.CASE_IDS)
def test_case_keeps_the_bar_honest(c):
    p = c.problem
    inp = pc.pwc_inputs(p)
    # a pure function of the case
    again = pc._build(p)
    for a, b in zip(inp, again):
        assert (a is None and b is None) or (np.asarray(a).tobytes() == np.asarray(b).tobytes())
    # every slice inside the radius of Pade-13, by the plain 1-norm the CPU routes plan with
    X = pc.slice_generators(inp, p.lind is not None)
    worst = max(x.norm1(X[b, n]) for b in range(X.shape[0]) for n in range(X.shape[1]))
    assert worst < o.PADE_THETA[4], worst
    # the bound the device plans with is the one the problem was built for, and lies in the claimed band
    assert pc.FAMILY_BOUND[c.family] == p.bound
    assert abs(inp.bounds.max() - p.target) <= 1e-12 * p.target
    for b in range(p.B):
        if p.ham == "mixed" and b == 1:  # the complex sample among real ones: the four-product scheme of the complex loop
            assert pc.scheme_of("sd_normal", inp.bounds[b]) == "e4n+0"
            continue
        assert pc.scheme_of(c.family, inp.bounds[b], inp.nsyms[b]) == c.scheme, (b, inp.bounds[b], inp.nsyms[b])
    if p.bound in ("col", "sum", "hb") and p.K:
        # every second slice has |c_k| = 1: the bound of a segment of two or more slices is the bound of the sample
        assert np.all(np.abs(inp.signals[:, :, 0::2]) == 1.0) and np.abs(inp.signals).max() == 1.0
    if p.bound == "slice":
        nrm = np.array([[x.device_norm(X[b, n]) for n in range(X.shape[1])] for b in range(X.shape[0])])
        assert np.all(np.abs(nrm[:, 0::2] - p.target) <= 1e-9 * p.target) and nrm.max() <= p.target * (1 + 1e-9)
    if p.bound == "sum" and c.family == "t18" and p.lind is None and p.D >= 93:
        # (the tiled path may plan slice by slice: the slices themselves lie in the same band)
        for b in range(X.shape[0]):
            for n in range(X.shape[1]):
                assert pc.scheme_of("t18", x.device_norm(X[b, n])) == c.scheme
    if p.trace:
        # the summed phase of every sample winds many times
        tr = lambda h: np.trace(h).real / p.D
        h0 = inp.h0[0] if inp.h0.ndim == 3 else inp.h0
        hks = inp.hks[0] if inp.hks.ndim == 4 else inp.hks
        total = inp.dt * (p.N * tr(h0) + sum(inp.signals[:, k, :].sum(axis=1) * tr(hks[k]) for k in range(p.K)))
        assert np.abs(total).min() > (20 if p.trace >= 10 else 2) * 2 * np.pi, total


def test_case_list_reaches_every_band_edge():
    """A pair of cases straddles each radius at (1 -+ 1e-3), and the two take different schemes."""
    by_id = {c.id: c for c in pc.CASES}
    for lo, hi in (("sd-real-D9-below-0.83", "sd-real-D9-above-0.83"), ("sd-real-D9-below-1.85", "sd-real-D9-above-1.85"), ("sd-real-D9-below-3.7", "sd-real-D9-above-3.7"),
                   ("sd-real-D5-below-0.83", "sd-real-D5-above-0.83"), ("sd-herm-D9-below-0.0004", "sd-herm-D9-above-0.0004"), ("sd-herm-D9-below-0.0545", "sd-herm-D9-above-0.0545"),
                   ("sd-herm-D9-below-1.35", "sd-herm-D9-above-1.35"), ("sd-herm-D9-below-2", "sd-herm-D9-above-2"), ("sd-nonherm-D9-below-1.13", "sd-nonherm-D9-above-1.13"),
                   ("md-real-D13-below-1.85", "md-real-D13-above-1.85")):
        a, b = by_id[lo], by_id[hi]
        assert a.scheme != b.scheme and abs(b.problem.target / a.problem.target - (1 + x.EDGE) / (1 - x.EDGE)) < 1e-12


def test_every_kernel_class_has_a_recorded_launch_log(golden_dir):
    """tests/golden/pwc_extended_kernels.json (launch logs recorded on the MI355X) names exactly the kernel classes of the cases."""
    import json
    import os

    recorded = json.load(open(os.path.join(golden_dir, "pwc_extended_kernels.json")))
    assert sorted(recorded) == sorted({c.kernel for c in pc.CASES})
    assert all(isinstance(v, str) and ".hip: " in v for v in recorded.values())
