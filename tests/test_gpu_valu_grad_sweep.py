"""The vector-unit backward sweeps of c3p_grad.hip (grad_seg_kernel, grad_scan_kernel, grad_bwd_kernel; grad_scan_general_kernel,
grad_bwd_general_kernel<GLOBAL, MODEL>) at every thread and memory class, at 41 <= D <= 64 on the default dispatch, and across
segments.

c3p_pwc_unitary_vjp takes the unitary sweep by default for 41 <= D <= 64 below the tiled rule, it is the only path of gen_bar_out
and of the fused goal above D = 40, its scan is the scan of the mid-D sweeps, and the general form is the second opinion of every
Lindblad gradient test (valu_grad).  The segment rule S = min(4096 / B, N / 8) gives every small shape one to five segments of eight
or more slices: segments of one slice, a scan longer than its prefetch (15 segment products on LDS), a long scan on global scratch
and odd next to even squaring counts inside one segment (t18_pair swaps the roles of its buffers once per squaring and hands them on
to the next slice) never ran.  Here the `valu_grad_segments` option pins S: two or three samples of N = 34 slices are cut into
segments of 34, 17/17, 11/12/11, 8/9/8/9 (the default), 2/3 (S = 16: every later product prefetched), 2 (S = 17: one product read in
the loop) and 1 slices.

Every case compares with the CPU oracle (oracle/c3_oracle.py) at the bar of tests/test_gradient.py, max|g - want| < 1e-10 max|want|
per sample and per output array.  Every target (the column-wise bound of a sample, see unitary_case) is at most 6: at most three
squarings of theta_18 = 1.13.  HIGH below is 6.0 at even D and 4.6 at odd D: with three drives (odd D) the slice norms lie at 0.4 ..
0.55 of the column-wise bound, and at 6.0 every slice of those draws took two squarings; at 4.6 they straddle 2.26 as the even D
straddle 4.52 at 6.0 (test_squaring_counts_mix_inside_segments).  The inputs and references are checked without a GPU by the CPU
tests at the end: the oracle against an eigen-decomposition form of the same gradients, a floor under the largest entry of every
reference, finite differences of the oracle's propagator, and the squaring counts per slice.

Every comparison prints one line `VALUERR <family> D=<D> S=<S> <ratio>`; DESIGN.md 5.6 records the worst per family, D and S of one
run."""
import functools

import numpy as np
import pytest

import lindblad_model_grad_ref as ref
from norm_bound_model import segments
from oracle import c3_oracle as o
from test_gpu_smalld_grad_segments import (FLOOR, _fd_check, _floor_ok, _fro, _frozen, _hb, goal_case, lindblad_case, lindblad_want,
                                           spectral_signal_gradient, unitary_case, unitary_want)

NB, N = 2, 34
BAR = 1e-10
T18_THETA = 1.13  # c3p_common.h
S_DEFAULT = 4  # min(4096 / B, N / 8)
S_LIST = (1, 2, 3, 16, 17, 34)
NPRE = 15  # grad_scan_kernel on LDS: C3P_GRAD_NMAT - 4 segment products fetched in one pass
HIGH = lambda D: 4.6 if D % 2 else 6.0

FORCED_D = (2, 9, 10, 11, 12, 13, 20, 21, 22, 27, 40)  # force_generic: below 41 the default dispatch has matrix-core sweeps
DEFAULT_D = (41, 48, 63, 64)  # no option, no flag
DIM_CASES = [(D, "complex", False) for D in FORCED_D + DEFAULT_D] + [(D, "real", False) for D in (21, 22, 63)] + [(27, "complex", True)]
SEG_CASES = [(9, 2), (16, 2), (27, 3), (48, 3)]  # (D, samples)
GEN_BAR_D = (48, 9)
GOAL48 = ((6, 8), (0, 1))  # dims, index
LIND_CASES = [(3, 2), (4, 2), (5, 3)]  # (D, samples): Dm = 9 and 16 on LDS, 25 on global scratch
LIND_S = (1, None, 17, 34)


def dim_key(D, kind, per_sample, target):
    return (D, kind, target, per_sample, NB, N)


def seg_key(D, nb):
    return (D, "complex", HIGH(D), False, nb, N)


def lind_key(D, nb):
    return (D, 1, True, N, 0.1, False, None, nb)


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import _lib, propagation

    _lib.require_gpu()
    return propagation


# ------------------------------------------------------------------------------------------------------------------------------
# references (cached: pure functions of the key, shared by the GPU tests and the CPU checks)
# ------------------------------------------------------------------------------------------------------------------------------
def slice_hamiltonians(h0, hks, sig_b):
    return h0[None] + np.einsum("kn,kij->nij", sig_b, hks)


@functools.lru_cache(maxsize=None)
def gen_bar_want(D):
    """(Hbar [B,N,D,D], g0 [B,D,D], gk [B,K,D,D]): the oracle's per-slice Hamiltonian cotangents on H_n = h0 + sum_k c_k(n) h_k
    and their contractions g0 = sum_n Hbar_n, gk = sum_n c_k(n) Hbar_n"""
    h0, hks, sig, dt, Ubar, ph = unitary_case(*seg_key(D, NB))
    hb = np.stack([o.pwc_per_slice_hamiltonian_cotangents(slice_hamiltonians(h0, hks, sig[b]), dt, Ubar[b], None if ph is None else ph[b])
                   for b in range(NB)])
    return _frozen(hb), _frozen(hb.sum(axis=1)), _frozen(np.einsum("bkn,bnij->bkij", sig, hb))


def goal48_case():
    return goal_case(48, seg_key(48, NB), GOAL48)


@functools.lru_cache(maxsize=None)
def goal48_want(kind):
    """(goal [B], d goal / d signals [B,K,N], d goal / d fr_phase [B,D], U [B,D,D], cotangents [B,D,D]) from the oracle alone.
    average_infid = 1 - (|s|^2 / L + 1) / (L + 1) against unitary_infid = 1 - |s|^2 / L^2 with the same overlap s: its cotangent is
    the oracle's unitary_infid_cotangent times L / (L + 1) (held to finite differences of o.average_infid below)."""
    h0, hks, sig, dt, q, ph = goal48_case()
    dims, index = (list(x) for x in GOAL48)
    L = q.shape[0]
    U = o.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    fac = 1.0 if kind == "unitary" else L / (L + 1.0)
    infid = o.unitary_infid if kind == "unitary" else o.average_infid
    Ubar = np.stack([fac * o.unitary_infid_cotangent(q, U[b], index, dims) for b in range(NB)])
    goal = np.array([infid(q, U[b], index=index, dims=dims) for b in range(NB)])
    grad = np.stack([o.pwc_signal_gradient(h0, hks, sig[b], dt, Ubar[b], ph[b]) for b in range(NB)])
    gph = -(np.conj(Ubar) * U).sum(axis=-1).imag
    return _frozen(goal), _frozen(grad), _frozen(gph), _frozen(U), _frozen(Ubar)


@functools.lru_cache(maxsize=None)
def lind_model_want(D, nb):
    """(grad_h0 [B,D,D], grad_hks [B,K,D,D], grad_col_ops [B,C,D,D]) of tests/lindblad_model_grad_ref.py"""
    h0, hks, sig, dt, col, Ubar, ph = lindblad_case(*lind_key(D, nb))
    r = [ref.lindblad_model_cotangents(h0, hks, col, sig[b], dt, Ubar[b], None if ph is None else ph[b]) for b in range(nb)]
    return tuple(_frozen(np.stack([x[i] for x in r])) for i in range(3))


# ------------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ------------------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(np.asarray(a)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def check(g, want, family, D, S, what=()):
    """per sample: max|g - want| / max|want| below the bar"""
    g = np.asarray(g)
    assert g.shape == want.shape, (g.shape, want.shape)
    err = max(np.abs(g[b] - want[b]).max() / np.abs(want[b]).max() for b in range(want.shape[0]))
    print(f"VALUERR {family} D={D} S={S_DEFAULT if S is None else S} {err:.3e}")
    assert err < BAR, (family, D, S, *what, err)
    return g


def check_array(g, want, family, D, S):
    """a whole array against its largest entry"""
    g = np.asarray(g)
    assert g.shape == want.shape, (g.shape, want.shape)
    err = np.abs(g - want).max() / np.abs(want).max()
    print(f"VALUERR {family} D={D} S={S_DEFAULT if S is None else S} {err:.3e}")
    assert err < BAR, (family, D, S, err)
    return g


def seg_opts(S, **opts):
    return dict(opts) if S is None else dict(opts, valu_grad_segments=S)


def launched():
    from c3_amd import _lib

    return _lib.last_kernel_detail().split("; ")


def unitary_sweep_log(D):
    """LDS up to D = 21 (19 (D | 1) D 16 B <= 150 KiB), the compile-time scans up to D = 12"""
    g = "false" if D <= 21 else "true"
    return [f"c3p_grad.hip: grad_seg_kernel<{g}>", f"c3p_grad.hip: grad_scan_kernel<{g}, {D if D <= 12 else 0}>", f"c3p_grad.hip: grad_bwd_kernel<{g}>"]


def assert_unitary_sweep(D):
    from c3_amd import _lib

    assert _lib.last_kernel() == ("generic_lds" if D <= 21 else "generic_global"), _lib.last_kernel()
    assert launched() == unitary_sweep_log(D), launched()


def uvjp(prop, case, S=None, **kw):
    """D <= 40 under force_generic, above on the default dispatch"""
    from c3_amd import _lib

    h0, hks, sig, dt, Ubar, ph = case
    with _lib.options(**seg_opts(S)):
        out = prop.propagate_batch_vjp(h0, hks, sig, dt, Ubar, fr_phase=ph, force_generic=h0.shape[-1] <= 40, **kw)
    assert_unitary_sweep(h0.shape[-1])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["low", "high"])
@pytest.mark.parametrize("D,kind,per_sample", DIM_CASES)
def test_dimension_classes(prop, D, kind, per_sample, target):
    """(a) the thread classes (64 threads up to D = 10, 128 up to 20, 256 above; 2 x 2 tiles with a clamped last row and column at
    odd D, 441 tiles at D = 41, 1024 at D = 63 and 64), the memory variants (LDS / global scratch at 21 / 22, the compile-time scans up
    to D = 12, the raised LDS limit from D = 13) on the default rule's four segments of 8/9/8/9 slices, without a squaring (target 1)
    and with one to three"""
    key = dim_key(D, kind, per_sample, 1.0 if target == "low" else HIGH(D))
    family = "dims/" + kind + ("/per-sample" if per_sample else "")
    check(uvjp(prop, unitary_case(*key)), unitary_want(*key), family, D, None, key)


@pytest.mark.gpu
@pytest.mark.parametrize("D,nb", SEG_CASES)
def test_segments_of_the_unitary_sweep(prop, D, nb):
    """(b) one segment of 34 slices down to 34 segments of one; with three samples the scan of the second and third sample works in
    scratch that lies behind the chains of other samples.  The launch log carries no grid size: that the option is live shows in the
    bits (another order of the same products), that it is clamped in S = 1000 returning the bits of S = 34."""
    key = seg_key(D, nb)
    case, want = unitary_case(*key), unitary_want(*key)
    got = {}
    for S in (None,) + S_LIST:
        got[S] = check(uvjp(prop, case, S), want, "segments", D, S, key)
    for S in (None, 1, 34):
        assert same_bits(got[S], uvjp(prop, case, S)), S
    assert same_bits(got[34], uvjp(prop, case, 1000))
    assert not (same_bits(got[1], got[None]) and same_bits(got[34], got[None]))


@pytest.mark.gpu
@pytest.mark.parametrize("D", GEN_BAR_D)
def test_model_cotangents_of_the_unitary_sweep(prop, D):
    """(c) gen_bar_out (want_model_grads): the only path above D = 40, on global scratch at D = 48 and on LDS at D = 9"""
    case = unitary_case(*seg_key(D, NB))
    _, g0w, gkw = gen_bar_want(D)
    want = unitary_want(*seg_key(D, NB))
    for S in (None, 17):
        g, g0, gk = uvjp(prop, case, S, want_model_grads=True)
        check(g, want, "gen_bar/signals", D, S)
        check_array(g0, g0w, "gen_bar/h0", D, S)
        check_array(gk, gkw, "gen_bar/hks", D, S)
        assert same_bits(g, uvjp(prop, case, S))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["unitary", "average"])
def test_fused_goal_above_40(prop, kind):
    """(d) c3p_pwc_unitary_goal_vjp at D = 48: goal, gradient, phase gradient and U against oracle quantities alone; the three-call
    form (the same kernels) at 1e-11 as test_fused_goal does"""
    from c3_amd import _lib, fidelities as fid

    h0, hks, sig, dt, q, ph = goal48_case()
    dims, index = (list(x) for x in GOAL48)
    goal, want, gph, U, _ = goal48_want(kind)
    for S in (None, 17):
        with _lib.options(**seg_opts(S)):
            r = prop.propagate_batch_goal_vjp(h0, hks, sig, dt, q, index, dims, kind=kind, fr_phase=ph)
            assert_unitary_sweep(48)
            Ug = np.asarray(prop.propagate_batch(h0, hks, sig, dt, fr_phase=ph)["U"])
            Ubar, goal3 = (fid.unitary_infid_cotangent if kind == "unitary" else fid.average_infid_cotangent)(q, Ug, index, dims)
            g3 = np.asarray(prop.propagate_batch_vjp(h0, hks, sig, dt, np.asarray(Ubar), fr_phase=ph))
            assert_unitary_sweep(48)
        g = check(r["grad_signals"], want, "goal/" + kind, 48, S)
        check_array(r["grad_fr_phase"], gph, "goal-phase/" + kind, 48, S)
        err = np.abs(np.asarray(r["goal"]) - goal).max()
        print(f"VALUERR goal-value/{kind} D=48 S={S_DEFAULT if S is None else S} {err:.3e}")
        assert err < 1e-11
        err = max(np.linalg.norm(np.asarray(r["U"])[b] - U[b]) for b in range(NB))
        print(f"VALUERR goal-U/{kind} D=48 S={S_DEFAULT if S is None else S} {err:.3e}")
        assert err < 1e-10
        assert np.abs(np.asarray(r["goal"]) - np.asarray(goal3)).max() < 1e-11
        assert np.abs(g - g3).max() < 1e-11 * np.abs(g3).max()


def lind_log(Dm, model):
    g = "false" if Dm <= 16 else "true"  # 20 (Dm | 1) Dm 16 B <= 150 KiB
    log = ["c3p_generic.hip: clp_kernel", "c3p_grad.hip: lind_gen_kernel", f"c3p_grad.hip: grad_seg_kernel<{g}>", "c3p_grad.hip: grad_scan_general_kernel<false>",
           f"c3p_grad.hip: grad_bwd_general_kernel<{g}, {'true' if model else 'false'}>"]
    return log + (["c3p_grad.hip: lind_model_reduce_kernel"] if model else [])


def lind_vjp(prop, case, S, model):
    from c3_amd import _lib

    h0, hks, sig, dt, col, Ubar, ph = case
    Dm = h0.shape[-1] ** 2
    with _lib.options(**seg_opts(S, valu_grad=1)):
        out = prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph, want_model_grads=model)
    assert _lib.last_kernel() == ("generic_lds" if Dm <= 16 else "generic_global"), _lib.last_kernel()
    assert launched() == lind_log(Dm, model), launched()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("D,nb", LIND_CASES)
def test_general_sweep_under_segments(prop, D, nb):
    """(e) grad_scan_general_kernel and grad_bwd_general_kernel<GLOBAL, MODEL> with one segment, the default four, 17 and 34 segments
    of one slice: there the prefix pass ends at its first break, no slice steps the left adjoint on, `first` is true on every slice of
    the model accumulators and 34 partial blocks per sample reach lind_model_reduce_kernel"""
    key = lind_key(D, nb)
    case, want = lindblad_case(*key), lindblad_want(*key)
    got = {}
    for S in LIND_S:
        got[S] = check(lind_vjp(prop, case, S, False), want, "lindblad", D, S, key)
        if D >= 4:
            out = lind_vjp(prop, case, S, True)
            assert same_bits(out[0], got[S]), S
            for g, w, what in zip(out[1:], lind_model_want(D, nb), ("h0", "hks", "col_ops")):
                check_array(g, w, "lindblad-model/" + what, D, S)
    assert same_bits(got[34], lind_vjp(prop, case, 34, False))
    assert not (same_bits(got[1], got[None]) and same_bits(got[34], got[None]))


# ------------------------------------------------------------------------------------------------------------------------------
# CPU part: the inputs and the references
# ------------------------------------------------------------------------------------------------------------------------------
def _unitary_keys():
    keys = [dim_key(D, kind, ps, t) for D, kind, ps in DIM_CASES for t in (1.0, HIGH(D))] + [seg_key(D, nb) for D, nb in SEG_CASES]
    return list(dict.fromkeys(keys))


def spectral_per_slice_cotangents(Hs, dt, Ubar, ph=None):
    """pwc_per_slice_hamiltonian_cotangents for Hermitian slices from their eigen-decompositions: Hbar_n = conj(-i dt) L(X_n^H; W_n)
    with the Frechet derivative along the general direction W_n by divided differences (Daleckii-Krein),
    L(V a V^+; W) = V (Psi o V^+ W V) V^+, Psi_ij = e^{(a_i + a_j) / 2} sin(y_ij) / y_ij, a = i dt w, y = dt (w_i - w_j) / 2"""
    n_sl, D = Hs.shape[0], Hs.shape[-1]
    ev = [np.linalg.eigh(H) for H in Hs]
    E = [(V * np.exp(-1j * dt * w)) @ V.conj().T for w, V in ev]
    pre = [np.eye(D, dtype=np.complex128)]
    for n in range(n_sl):
        pre.append(E[n] @ pre[-1])
    lam = Ubar.astype(np.complex128)  # post_n^H FR^H Ubar
    if ph is not None:
        lam = np.exp(-1j * ph)[:, None] * lam
    out = np.zeros((n_sl, D, D), dtype=np.complex128)
    for n in range(n_sl - 1, -1, -1):
        w, V = ev[n]
        Psi = np.exp(1j * dt * (w[:, None] + w[None, :]) / 2) * np.sinc(dt * (w[:, None] - w[None, :]) / (2 * np.pi))
        out[n] = (1j * dt) * V @ (Psi * (V.conj().T @ (lam @ pre[n].conj().T) @ V)) @ V.conj().T
        lam = E[n].conj().T @ lam
    return out


def test_the_oracle_itself_is_two_orders_below_the_bar():
    """every unitary reference of this module against spectral_signal_gradient, and the per-slice cotangents of (c) against
    spectral_per_slice_cotangents: 1e-12 of the largest entry per sample"""
    cases = [(unitary_case(*key), unitary_want(*key), key) for key in _unitary_keys()]
    h0, hks, sig, dt, q, ph = goal48_case()
    cases += [((h0, hks, sig, dt, goal48_want(kind)[4], ph), goal48_want(kind)[1], ("goal", kind)) for kind in ("unitary", "average")]
    for (h0, hks, sig, dt, Ubar, ph), want, key in cases:
        for b in range(want.shape[0]):
            g = spectral_signal_gradient(_hb(h0, b), hks, sig[b], dt, Ubar[b], None if ph is None else ph[b])
            assert np.abs(g - want[b]).max() < 1e-12 * np.abs(want[b]).max(), (key, b)
    for D in GEN_BAR_D:
        h0, hks, sig, dt, Ubar, ph = unitary_case(*seg_key(D, NB))
        hb, g0, gk = gen_bar_want(D)
        for b in range(NB):
            sp = spectral_per_slice_cotangents(slice_hamiltonians(h0, hks, sig[b]), dt, Ubar[b], None if ph is None else ph[b])
            assert np.abs(sp - hb[b]).max() < 1e-12 * np.abs(hb[b]).max(), (D, b)
            assert np.abs(sp.sum(axis=0) - g0[b]).max() < 1e-12 * np.abs(g0[b]).max(), (D, b)
            assert np.abs(np.einsum("kn,nij->kij", sig[b], sp) - gk[b]).max() < 1e-12 * np.abs(gk[b]).max(), (D, b)


def test_reference_gradients_are_not_at_roundoff_level():
    """the FLOOR rule of tests/test_gpu_smalld_grad_segments.py on every reference of this module.  The scale of the per-slice
    cotangents is ||Ubar||_F dt, that of the contracted model cotangents the same (one slice's worth: the sum over the slices is not
    counted on), times ||h -> -i (h (x) 1 - 1 (x) h^T)|| <= 2 sqrt(D) for the Lindblad Hamiltonians and 4 sqrt(D) ||C||_F for an
    entry of a collapse operator."""
    for key in _unitary_keys():
        h0, hks, sig, dt, Ubar, ph = unitary_case(*key)
        assert _floor_ok(unitary_want(*key), [_fro(u) for u in Ubar], dt * max(_fro(h) for h in hks)), key
    h0, hks, sig, dt, q, ph = goal48_case()
    for kind in ("unitary", "average"):
        goal, want, gph, U, Ubar = goal48_want(kind)
        assert _floor_ok(want, [_fro(u) for u in Ubar], dt * max(_fro(h) for h in hks)), kind
        assert _floor_ok(gph, [_fro(u) for u in Ubar], 1.0), kind  # |U_ij| <= 1
        assert goal.min() > 1e-3  # (a goal at its minimum has no gradient)
    for D in GEN_BAR_D:
        h0, hks, sig, dt, Ubar, ph = unitary_case(*seg_key(D, NB))
        for w in gen_bar_want(D):
            assert _floor_ok(w, [_fro(u) for u in Ubar], dt), D
    for D, nb in LIND_CASES:
        h0, hks, sig, dt, col, Ubar, ph = lindblad_case(*lind_key(D, nb))
        I = np.eye(D)
        gen = dt * max(_fro(np.kron(h, I) - np.kron(I, h.T)) for h in hks)
        assert _floor_ok(lindblad_want(*lind_key(D, nb)), [_fro(u) for u in Ubar], gen), D
        if D >= 4:
            g0, gk, gc = lind_model_want(D, nb)
            ub = [_fro(u) for u in Ubar]
            assert _floor_ok(g0, ub, dt * 2 * np.sqrt(D)) and _floor_ok(gk, ub, dt * 2 * np.sqrt(D)), D
            assert _floor_ok(gc, ub, dt * 4 * np.sqrt(D) * _fro(col)), D


def test_references_match_finite_differences_of_the_oracle_propagator():
    """one sample per case family; the goal cases through the oracle's own infidelities (the factor L / (L + 1) of the average kind)"""
    rng = np.random.default_rng(3)
    for key, b in [(dim_key(41, "complex", False, 4.6), 1), (dim_key(27, "complex", True, 1.0), 0), (dim_key(22, "real", False, 6.0), 1), (seg_key(48, 3), 2)]:
        h0, hks, sig, dt, Ubar, ph = unitary_case(*key)
        loss = lambda s: np.real(np.vdot(Ubar[b], o.propagate_batch(_hb(h0, b), hks, s[None], dt, fr_phase=None if ph is None else ph[b : b + 1])[0]))
        _fd_check(unitary_want(*key)[b], loss, sig[b], rng, 1e-5)
    h0, hks, sig, dt, q, ph = goal48_case()
    dims, index = (list(x) for x in GOAL48)
    for kind, infid in (("unitary", o.unitary_infid), ("average", o.average_infid)):
        loss = lambda s: infid(q, o.propagate_batch(h0, hks, s[None], dt, fr_phase=ph[1:2])[0], index=index, dims=dims)
        _fd_check(goal48_want(kind)[1][1], loss, sig[1], rng, 1e-5)
        at = lambda p: infid(q, o.propagate_batch(h0, hks, sig[1:2], dt, fr_phase=p[None])[0], index=index, dims=dims)
        gph = goal48_want(kind)[2][1]
        for i in (0, 1, 8, 9):  # the rows of the computational subspace of dims (6, 8)
            e = 1e-5 * np.eye(48)[i]
            assert abs((at(ph[1] + e) - at(ph[1] - e)) / 2e-5 - gph[i]) < 1e-6 * np.abs(gph).max(), (kind, i)
    for key, b in [(lind_key(3, 2), 1), (lind_key(5, 3), 2)]:
        h0, hks, sig, dt, col, Ubar, ph = lindblad_case(*key)
        rows = np.ones(Ubar.shape[-1]) if ph is None else np.exp(1j * ph[b])
        loss = lambda s: np.real(np.vdot(Ubar[b], rows[:, None] * o.propagate_batch(h0, hks, s[None], dt, col_ops=col, lindbladian=True)[0]))
        _fd_check(lindblad_want(*key)[b], loss, sig[b], rng, 1e-5)
    h0, hks, sig, dt, col, Ubar, ph = lindblad_case(*lind_key(4, 2))  # the model cotangents along random directions of every operator
    g0, gk, gc = lind_model_want(4, 2)
    at = lambda a, k, c: ref.loss(a, k, c, sig[1], dt, Ubar[1], None if ph is None else ph[1])
    cplx = lambda shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    d0, dk, dc = cplx(h0.shape), cplx(hks.shape), cplx(col.shape)
    fd = (at(h0 + 1e-6 * d0, hks + 1e-6 * dk, col + 1e-6 * dc) - at(h0 - 1e-6 * d0, hks - 1e-6 * dk, col - 1e-6 * dc)) / 2e-6
    lin = sum(np.real(np.sum(np.conj(g[1]) * d)) for g, d in ((g0, d0), (gk, dk), (gc, dc)))
    assert abs(fd - lin) < 1e-7 * max(1.0, abs(fd)), (fd, lin)
    for D in GEN_BAR_D:  # (the rule of test_oracle_per_slice_cotangents_match_finite_differences)
        h0, hks, sig, dt, Ubar, ph = unitary_case(*seg_key(D, NB))
        Hs, want = slice_hamiltonians(h0, hks, sig[1]), gen_bar_want(D)[0][1]
        rows = np.ones(D) if ph is None else np.exp(1j * ph[1])

        def loss(H):
            U = np.eye(D, dtype=complex)
            for n in range(N):
                U = o.expm(-1j * dt * H[n]) @ U
            return np.real(np.vdot(Ubar[1], rows[:, None] * U))

        # a direction of Frobenius norm 1 over all slices and a step of 1e-5: the third derivative along it is of the order of
        # dt^3 ||Ubar||_F ~ 2e3 at D = 48, so the central difference is off by ~ 3e-8; the bar of _fd_check, 1e-6
        for _ in range(2):
            dH = rng.normal(size=Hs.shape) + 1j * rng.normal(size=Hs.shape)
            dH /= _fro(dH)
            fd = (loss(Hs + 1e-5 * dH) - loss(Hs - 1e-5 * dH)) / 2e-5
            assert abs(fd - np.real(np.sum(np.conj(want) * dH))) < 1e-6 * max(1.0, abs(fd))


def slice_squarings(key):
    """what assemble (c3p_grad.hip) computes per slice: the 1-norm of -i dt H_n less its imaginary trace shift, and
    c3p_squarings(., 1.13); [B, N] counts and the distance of the nearest norm from a threshold 1.13 x 2^j, relative"""
    h0, hks, sig, dt, _, _ = unitary_case(*key)
    D = hks.shape[-1]
    s = np.zeros(sig.shape[::2], dtype=int)
    margin = np.inf
    for b in range(sig.shape[0]):
        for n, H in enumerate(slice_hamiltonians(_hb(h0, b), hks, sig[b])):
            nrm = np.abs(dt * (H - np.trace(H).real / D * np.eye(D))).sum(axis=0).max()
            p = T18_THETA
            while p < nrm:
                p, s[b, n] = 2 * p, s[b, n] + 1
            margin = min(margin, abs(nrm / p - 1), abs(2 * nrm / p - 1))
    return s, margin


def _mixed_segments(s, S):
    """segments [g N / S, (g + 1) N / S) of any sample that hold an odd and an even squaring count"""
    return sum(len({int(x) % 2 for x in s[b, n0:n1]}) == 2 for b in range(s.shape[0]) for n0, n1 in segments(N, S, per_mille=500))


def test_squaring_counts_mix_inside_segments():
    """no squaring at target 1; at the high target one to three, no slice nearer than 1e-9 to a threshold (the device sums in
    another order), and odd next to even counts inside a segment -- where t18_pair hands swapped buffer roles to the next slice -- in
    every (a) case from D = 41 on the default four segments and in every (b) case at every S that has segments of two slices or more"""
    for D, kind, ps in DIM_CASES:
        s, _ = slice_squarings(dim_key(D, kind, ps, 1.0))
        assert s.max() == 0, (D, kind, ps)
        s, margin = slice_squarings(dim_key(D, kind, ps, HIGH(D)))
        assert 1 <= s.min() and s.max() <= 3 and margin > 1e-9, (D, kind, ps, s.min(), s.max(), margin)
        if D >= 41:
            assert _mixed_segments(s, S_DEFAULT) > 0, (D, kind, ps)
    for D, nb in SEG_CASES + [(D, NB) for D in GEN_BAR_D]:
        s, margin = slice_squarings(seg_key(D, nb))
        assert 1 <= s.min() and s.max() <= 3 and margin > 1e-9, (D, nb, margin)
        for S in (1, 2, 3, S_DEFAULT, 16, 17):
            assert _mixed_segments(s, S) > 0, (D, nb, S)
        assert _mixed_segments(s, 34) == 0


def test_the_cases_are_what_the_gpu_tests_take_them_for():
    """the segment lengths of every S, the scan's prefetch split, the memory classes, and that every target stays at or below 6"""
    lens = lambda S: sorted({n1 - n0 for n0, n1 in segments(N, S, per_mille=500)})
    assert [lens(S) for S in S_LIST] == [[34], [17], [11, 12], [2, 3], [2], [1]] and lens(S_DEFAULT) == [8, 9]
    assert min(4096 // 3, N // 8) == S_DEFAULT == min(4096 // NB, N // 8)
    assert 16 - 1 <= NPRE < 17 - 1  # S = 16: every later product prefetched; S = 17: one read in the loop
    lds = lambda D, nmat: nmat * (D | 1) * D * 16
    assert lds(21, 19) <= 150 * 1024 < lds(22, 19) and lds(12, 19) <= 48 * 1024 < lds(13, 19)
    assert lds(16, 20) <= 150 * 1024 < lds(25, 20)
    for key in _unitary_keys():
        h0, hks, sig, dt, Ubar, ph = unitary_case(*key)
        assert key[2] <= 6.0 and sig.shape == (key[4], 3 if key[0] % 2 else 1, N) and (h0.ndim == 3) == key[3]
    for D, nb in LIND_CASES:
        h0, hks, sig, dt, col, Ubar, ph = lindblad_case(*lind_key(D, nb))
        assert sig.shape == (nb, 3, N) and Ubar.shape == (nb, D * D, D * D) and col.shape == (1, D, D)
