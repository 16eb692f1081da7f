"""Collapse operators per sample (C3P_COL_PER_SAMPLE, col_ops [B,C,D,D]) through the PWC Lindblad path on the GPU: the forward
call on every kernel family, the control gradient, the model-operator cotangents, and the refusals.

References: the pinned oracle (oracle/c3_oracle.py) and the numpy restatements of tests/lindblad_model_grad_ref.py and
tests/lindblad_model_grad_fast_ref.py, called per sample with col_ops[b].  Bars, all taken from the neighbouring files:
|U[b] - U_oracle[b]|_F < 1e-10 (the parity bar), 1e-10 max|want| for the control gradient (tests/test_gradient.py) and per
cotangent array (tests/test_gpu_lindblad_model_grad.py, tests/test_gpu_lindblad_model_grad_hb.py).

Inputs: Hermitian h0 / hks as _inputs of tests/test_gpu_lindblad_model_grad.py, dt = 0.3, K = 2, C = 2, and
col_ops[b] = s_b (complex Gaussian), independent draws per sample, s = (0.1, 0.25, 0.4): a kernel that reads sample 0's
dissipator misses by O(0.1), not by rounding -- every forward test asserts that the references of the samples differ."""
import functools

import numpy as np
import pytest

import lindblad_model_grad_fast_ref as fast
import lindblad_model_grad_ref as ref
from c3_amd import _lib
from oracle import c3_oracle as o

pytestmark = pytest.mark.gpu
DT, K, C = 0.3, 2, 2
SCALES = (0.1, 0.25, 0.4)
TOL = 1e-10


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation

    _lib.require_gpu()
    return propagation


@functools.lru_cache(maxsize=None)
def _inputs(D, N, B, hermitian=True, per_sample_h0=False, nC=C, seed=0):
    rng = np.random.default_rng(7000 + 100 * D + N + seed)
    herm = lambda s: (lambda a: s * (a + a.conj().T) / 2)(rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D)))
    h0 = np.stack([herm(0.8) for _ in range(B if per_sample_h0 else 1)])
    if not hermitian:
        h0 = h0 + 0.1 * (rng.normal(size=h0.shape) + 1j * rng.normal(size=h0.shape))
    if not per_sample_h0:
        h0 = h0[0]
    hks = np.stack([herm(0.5) for _ in range(K)])
    col = np.stack([SCALES[b] * (rng.normal(size=(nC, D, D)) + 1j * rng.normal(size=(nC, D, D))) for b in range(B)])
    sig = rng.uniform(-1, 1, size=(B, K, N))
    Dm = D * D
    Ubar = rng.normal(size=(B, Dm, Dm)) + 1j * rng.normal(size=(B, Dm, Dm))
    ph = rng.uniform(0, 2 * np.pi, size=(B, Dm))
    return h0, hks, sig, col, Ubar, ph


def _h0(h0, b):
    return h0[b] if h0.ndim == 3 else h0


def _ref_U(h0, hks, sig, col, ph=None):
    """the oracle per sample with col[b] (and h0[b]), the row phases ph [B,D^2] applied as the library defines them
    (U <- diag(exp(i ph)) U); also asserts that the samples' references differ"""
    U = np.stack([o.propagate_batch(_h0(h0, b), hks, sig[b : b + 1], DT, col_ops=col[b], lindbladian=True)[0] for b in range(sig.shape[0])])
    if ph is not None:
        U = np.exp(1j * ph)[:, :, None] * U
    assert max(np.linalg.norm(U[b] - U[0]) for b in range(len(U))) > 1e-3
    return U


def _check_U(got, want, what):
    got = np.asarray(got)
    errs = [np.linalg.norm(got[b] - want[b]) for b in range(len(want))]
    print(f"{what}: max_b |U[b] - U_oracle[b]|_F = {max(errs):.3e}")
    assert max(errs) < TOL, (what, errs)


def _close(got, want, what, tol=TOL):
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    print(f"{what}: max|got - want| = {err:.3e}, max|want| = {np.abs(want).max():.3e}")
    assert err < tol * np.abs(want).max(), (what, err, np.abs(want).max())


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- forward ----

# D, N, B, hermitian, source file that must have launched, options, propagate_batch keywords
FORWARD = [
    (2, 41, 3, True, "c3p_smallr", {}, {}),
    (3, 41, 3, True, "c3p_smallr", {}, {}),
    (4, 41, 3, True, "c3p_smallr", {}, {}),
    (3, 24, 3, False, "c3p_smalld", {}, {}),
    (4, 24, 3, False, "c3p_midd", {}, {}),
    (5, 24, 3, True, "c3p_midd", {}, {}),
    (6, 24, 3, True, "c3p_midd", {}, {}),
    (7, 24, 3, True, "c3p_regr", {}, {}),
    (9, 16, 2, True, "c3p_regr", {}, {}),
    (7, 16, 3, False, "c3p_regd", {}, {}),
    (7, 16, 3, True, "c3p_bigd", {"no_regd": 1}, {}),
    (10, 8, 2, True, "c3p_tiled", {}, {}),
    (3, 24, 3, True, "c3p_generic", {}, {"force_generic": True}),
]


@pytest.mark.parametrize("D,N,B,hermitian,source,options,kw", FORWARD, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, dict) else "")
def test_forward_every_family(prop, D, N, B, hermitian, source, options, kw):
    h0, hks, sig, col, _, ph = _inputs(D, N, B, hermitian)
    want = _ref_U(h0, hks, sig, col, ph)
    with _lib.options(**options):
        got = prop.propagate_batch(h0, hks, sig, DT, col_ops=col, lindbladian=True, fr_phase=ph, **kw)["U"]
        detail = _lib.last_kernel_detail()
    assert source + ".hip" in detail, detail
    _check_U(got, want, f"D={D} N={N} B={B} {source}")


def test_forward_with_slice_propagators(prop):
    """want_dUs at D = 2 (the complex small-D kernel): U and every slice propagator"""
    D, N, B = 2, 24, 3
    h0, hks, sig, col, _, _ = _inputs(D, N, B)
    r = prop.propagate_batch(h0, hks, sig, DT, col_ops=col, lindbladian=True, want_dUs=True)
    assert "c3p_smalld.hip" in _lib.last_kernel_detail(), _lib.last_kernel_detail()
    _check_U(r["U"], _ref_U(h0, hks, sig, col), "D=2 want_dUs U")
    dUs = np.stack([o.tf_propagation_lind(h0, hks, col[b], sig[b], DT) for b in range(B)])
    err = max(np.linalg.norm(np.asarray(r["dUs"])[b, n] - dUs[b, n]) for b in range(B) for n in range(N))
    print(f"D=2 dUs: max |dU - dU_oracle|_F = {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("D", [3, 5])
def test_forward_per_slice_hamiltonians(prop, D):
    """h0 [B,N,D,D] with lindbladian=True: the supplied-generator route (one dense generator per slice, with the sample's
    dissipator)"""
    N, B = 24, 3
    h0, hks, sig, col, _, _ = _inputs(D, N, B)
    hs = np.stack([o.sum_h0_hks(h0, hks, sig[b]) for b in range(B)])  # [B,N,D,D]
    assert hs.shape == (B, N, D, D)
    want = np.stack([o.tf_matmul_left(o.tf_propagation_lind(hs[b], None, col[b], None, DT)) for b in range(B)])
    assert max(np.linalg.norm(want[b] - want[0]) for b in range(B)) > 1e-3
    got = prop.propagate_batch(hs, None, None, DT, col_ops=col, lindbladian=True)["U"]
    detail = _lib.last_kernel_detail()
    assert "lind_slice_gen_kernel" in detail and ("c3p_smalld.hip" if D == 3 else "c3p_midd.hip") in detail, detail
    _check_U(got, want, f"D={D} per-slice")


def test_forward_per_sample_h0_and_col(prop):
    D, N, B = 3, 24, 3
    h0, hks, sig, col, _, ph = _inputs(D, N, B, True, True)
    assert h0.shape == (B, D, D)
    got = prop.propagate_batch(h0, hks, sig, DT, col_ops=col, lindbladian=True, fr_phase=ph)["U"]
    _check_U(got, _ref_U(h0, hks, sig, col, ph), "D=3 per-sample h0 and col_ops")


def test_forward_device_tensors_match_host_arrays(prop):
    import torch

    D, N, B = 3, 24, 3
    h0, hks, sig, col, _, ph = _inputs(D, N, B, False)
    host = prop.propagate_batch(h0, hks, sig, DT, col_ops=col, lindbladian=True, fr_phase=ph)["U"]
    t = lambda a: torch.as_tensor(a, device="cuda:0")
    dev = prop.propagate_batch(t(h0), t(hks), t(sig), DT, col_ops=t(col), lindbladian=True, fr_phase=t(ph))["U"]
    assert _bits(host, dev.cpu().numpy())
    _check_U(host, _ref_U(h0, hks, sig, col, ph), "D=3 host arrays")


@pytest.mark.parametrize("D,N", [(3, 24), (5, 24), (7, 16)])
def test_identical_copies_equal_the_per_sample_h0_plan(prop, D, N):
    """B identical copies of col_ops with a shared h0, against shared col_ops with h0 broadcast to [B,D,D]: both calls build one
    table set per sample from the same numbers on the same plan, so the results are the same bits"""
    B = 3
    h0, hks, sig, col, _, ph = _inputs(D, N, B)
    one = np.ascontiguousarray(col[1])
    a = prop.propagate_batch(h0, hks, sig, DT, col_ops=np.broadcast_to(one, (B,) + one.shape).copy(), lindbladian=True, fr_phase=ph)["U"]
    da = _lib.last_kernel_detail()
    b = prop.propagate_batch(np.broadcast_to(h0, (B, D, D)).copy(), hks, sig, DT, col_ops=one, lindbladian=True, fr_phase=ph)["U"]
    assert da == _lib.last_kernel_detail(), (da, _lib.last_kernel_detail())
    diff = np.abs(np.asarray(a) - np.asarray(b)).max()
    print(f"D={D}: max|copies - broadcast h0| = {diff:.3e}")
    assert _bits(a, b)


def test_reserve_takes_the_flag(prop):
    """c3p_reserve with C3P_COL_PER_SAMPLE sizes the workspace of the per-sample call: the call after it does not grow it"""
    lib = _lib.load()
    D, N, B = 5, 24, 3
    h0, hks, sig, col, _, _ = _inputs(D, N, B)
    import torch

    t = lambda a: torch.as_tensor(a, device="cuda:0")
    _lib.check(lib.c3p_reserve(1, B, K, N, D, C, _lib.COL_PER_SAMPLE))
    gen = lib.c3p_workspace_generation()
    got = prop.propagate_batch(t(h0), t(hks), t(sig), DT, col_ops=t(col), lindbladian=True)["U"]
    torch.cuda.synchronize()
    assert lib.c3p_workspace_generation() == gen
    _check_U(got.cpu().numpy(), _ref_U(h0, hks, sig, col), "D=5 after c3p_reserve")


# ---- control gradient ----

# D, N, B, hermitian, source file of the sweep, options
GRAD = [
    (2, 24, 3, False, "c3p_smalld", {}),
    (3, 24, 3, False, "c3p_smalld", {}),
    (4, 24, 3, False, "c3p_midd", {}),
    (3, 24, 3, True, "c3p_smallr", {}),
    (7, 16, 3, True, "c3p_regrg", {}),
    (3, 24, 3, True, "c3p_grad", {"valu_grad": 1}),
]


@pytest.mark.parametrize("D,N,B,hermitian,source,options", GRAD, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, dict) else "")
def test_control_gradient(prop, D, N, B, hermitian, source, options):
    h0, hks, sig, col, Ubar, ph = _inputs(D, N, B, hermitian)
    with _lib.options(**options):
        g = np.asarray(prop.propagate_batch_lindblad_vjp(h0, hks, sig, DT, col, Ubar, fr_phase=ph))
        detail = _lib.last_kernel_detail()
    assert source + ".hip" in detail, detail
    want = np.stack([o.pwc_lindblad_signal_gradient(h0, hks, col[b], sig[b], DT, Ubar[b], ph[b]) for b in range(B)])
    # the last sample with sample 0's collapse operators is far from its own gradient: the check can fail
    wrong = o.pwc_lindblad_signal_gradient(h0, hks, col[0], sig[B - 1], DT, Ubar[B - 1], ph[B - 1])
    assert np.abs(wrong - want[B - 1]).max() > 1e-3 * np.abs(want).max()
    _close(g, want, f"D={D} {source} grad_signals")


# ---- model-operator cotangents ----

MODEL = [(2, 7, 3, 1, False), (3, 17, 3, 2, True), (5, 17, 2, 2, False)]


@pytest.mark.parametrize("D,N,B,nC,per_sample_h0", MODEL)
def test_model_cotangents_general_sweep(prop, D, N, B, nC, per_sample_h0):
    h0, hks, sig, col, Ubar, ph = _inputs(D, N, B, True, per_sample_h0, nC)
    out = prop.propagate_batch_lindblad_vjp(h0, hks, sig, DT, col, Ubar, fr_phase=ph, want_model_grads=True)
    assert "lind_model_reduce_kernel" in _lib.last_kernel_detail(), _lib.last_kernel_detail()
    r = [ref.lindblad_model_cotangents(_h0(h0, b), hks, col[b], sig[b], DT, Ubar[b], ph[b]) for b in range(B)]
    want = tuple(np.stack([x[i] for x in r]) for i in range(3))
    wrong = ref.lindblad_model_cotangents(_h0(h0, B - 1), hks, col[0], sig[B - 1], DT, Ubar[B - 1], ph[B - 1])[2]
    assert np.abs(wrong - want[2][B - 1]).max() > 1e-3 * np.abs(want[2]).max()
    assert np.asarray(out[3]).shape == (B, nC, D, D)
    for got, w, what in zip(out[1:], want, ("grad_h0", "grad_hks", "grad_col_ops")):
        _close(got, w, f"D={D} {what}")
    with _lib.options(valu_grad=1):
        gv = prop.propagate_batch_lindblad_vjp(h0, hks, sig, DT, col, Ubar, fr_phase=ph)
    assert _bits(out[0], gv)
    again = prop.propagate_batch_lindblad_vjp(h0, hks, sig, DT, col, Ubar, fr_phase=ph, want_model_grads=True)
    for a, b in zip(out, again):
        assert _bits(a, b)


def test_model_cotangents_hermitian_basis_sweep(prop):
    D, N, B = 7, 6, 2
    h0, hks, sig, col, Ubar, ph = _inputs(D, N, B)
    out = prop.propagate_batch_lindblad_vjp(h0, hks, sig, DT, col, Ubar, fr_phase=ph, want_model_grads=True, hermitian_basis=True)
    assert "regr_model_reduce_kernel" in _lib.last_kernel_detail(), _lib.last_kernel_detail()
    r = [fast.lindblad_model_cotangents(h0, hks, col[b], sig[b], DT, Ubar[b], ph[b]) for b in range(B)]
    g0, gk, gc = (np.stack([x[i] for x in r]) for i in range(3))
    wrong = fast.lindblad_model_cotangents(h0, hks, col[0], sig[1], DT, Ubar[1], ph[1])[2]
    assert np.abs(wrong - gc[1]).max() > 1e-3 * np.abs(gc).max()
    _close(out[1], fast.hermitian_part(g0), "D=7 grad_h0")
    _close(out[2], fast.hermitian_part(gk), "D=7 grad_hks")
    _close(out[3], gc, "D=7 grad_col_ops")
    gs = prop.propagate_batch_lindblad_vjp(h0, hks, sig, DT, col, Ubar, fr_phase=ph)
    assert _bits(out[0], gs)


# ---- refusals ----


def test_refusals_then_the_next_call_works(prop):
    import torch

    from c3_amd._lib import C3PropError

    D, N, B = 3, 24, 3
    h0, hks, sig, col, _, ph = _inputs(D, N, B)
    t = lambda a: torch.as_tensor(a, device="cuda:0")
    with pytest.raises(C3PropError, match=r"C3:Error.*col_ops"):
        prop.propagate_batch_lindblad_taped(t(h0), t(hks), t(sig), DT, t(col))
    with pytest.raises(C3PropError, match=r"C3:Error.*col_ops"):
        prop.BatchPropagator(t(h0), t(hks), t(sig), DT, col_ops=t(col))
    rho = np.eye(D, dtype=complex) / D
    with pytest.raises(C3PropError, match=r"C3:Error.*col_ops"):
        prop.ode_solve_batch(h0, hks, sig, DT, rho, col_ops=col)
    with pytest.raises(C3PropError, match=r"C3:Error.*col_ops"):
        prop.propagate_batch(h0, hks, sig, DT, col_ops=col)  # unitary
    with pytest.raises(C3PropError, match=r"C3:Error.*col_ops has shape"):
        prop.propagate_batch(h0, hks, sig, DT, col_ops=col[:2], lindbladian=True)
    # the flag itself, at the C ABI
    lib = _lib.load()
    c = lambda a: np.ascontiguousarray(a, dtype=np.complex128)
    h0c, hkc, colc = c(h0), c(hks), c(col)
    p = lambda a: a.ctypes.data
    U = np.empty((B, D, D), dtype=np.complex128)
    fl = _lib.HOST_PTRS | _lib.COL_PER_SAMPLE
    assert lib.c3p_pwc_unitary(p(h0c), 0, p(hkc), 0, p(sig), DT, B, K, N, D, fl, None, p(U), None, None) != 0
    assert b"C3P_COL_PER_SAMPLE" in lib.c3p_last_error()
    st = np.empty((B, N, D, D), dtype=np.complex128)
    rc = lib.c3p_ode_solve(p(h0c), p(hkc), p(sig), p(colc), C, DT, B, K, N, D, 0, 2, p(c(rho)), 0, 1, fl, p(st), None)
    assert rc != 0 and b"C3P_COL_PER_SAMPLE" in lib.c3p_last_error()
    nseg = _lib.C.c_int(0)
    need = lib.c3p_pwc_lindblad_tape_bytes(B, K, N, D, _lib.C.byref(nseg))
    tape = torch.empty(max(int(need), 16), dtype=torch.uint8, device="cuda:0")
    Ud = torch.empty((B, D * D, D * D), dtype=torch.complex128, device="cuda:0")
    rc = lib.c3p_pwc_lindblad_taped(t(h0c).data_ptr(), 0, t(hkc).data_ptr(), 0, t(sig).data_ptr(), t(colc).data_ptr(), C, DT, B, K, N, D,
                                    _lib.COL_PER_SAMPLE, None, Ud.data_ptr(), tape.data_ptr(), need, nseg.value, None)
    assert rc != 0 and b"C3P_COL_PER_SAMPLE" in lib.c3p_last_error()
    # the next valid call works
    got = prop.propagate_batch(h0, hks, sig, DT, col_ops=col, lindbladian=True, fr_phase=ph)["U"]
    _check_U(got, _ref_U(h0, hks, sig, col, ph), "after the refusals")
