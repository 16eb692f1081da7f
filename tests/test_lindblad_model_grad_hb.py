"""Model-operator cotangents of the Lindblad path at D = 7, 8, 9, host side: the one-Frechet-derivative-per-slice reference
(tests/lindblad_model_grad_fast_ref.py) against the entry-by-entry one (tests/lindblad_model_grad_ref.py), the distance between a
Hamiltonian cotangent and its Hermitian part (what the Hermitian-basis sweep returns), argument checks of the new keyword."""
import numpy as np
import pytest

import lindblad_model_grad_fast_ref as fast
import lindblad_model_grad_ref as ref


def _problem(D, C, N, seed, K=2):
    rng = np.random.default_rng(seed)
    cx = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)
    herm = lambda s: (lambda a: s * (a + a.conj().T) / 2)(cx(D, D))
    h0, hks = herm(0.8), np.stack([herm(0.5) for _ in range(K)])
    col = 0.25 * cx(C, D, D)
    sig = rng.uniform(-1, 1, size=(K, N))
    Dm = D * D
    return h0, hks, col, sig, 0.3, cx(Dm, Dm), rng.uniform(0, 2 * np.pi, size=Dm)


SHAPES = [(2, 1, 7), (3, 2, 5)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "D%d-C%d-N%d" % s)
def both(request):
    D, C, N = request.param
    p = _problem(D, C, N, 10 * D + N)
    return ref.lindblad_model_cotangents(*p), fast.lindblad_model_cotangents(*p)


def test_fast_reference_matches_the_entrywise_reference(both):
    """1e-12 relative per output array (both are exact up to rounding: the same oracle directions, one identity between them)"""
    slow, quick = both
    for s, q, what in zip(slow, quick, ("grad_h0", "grad_hks", "grad_col_ops")):
        err = np.abs(q - s).max() / np.abs(s).max()
        print(f"{what}: relative difference {err:.2e}")
        assert q.shape == s.shape and err < 1e-12, (what, err)


def test_hermitian_part_of_grad_h0_is_far_from_the_full_cotangent(both):
    """the GPU comparison against the Hermitian part can tell it from the full cotangent: more than 0.1 relative apart"""
    g0 = both[0][0]
    gap = np.abs(fast.hermitian_part(g0) - g0).max() / np.abs(g0).max()
    print(f"|herm(grad_h0) - grad_h0| / |grad_h0| = {gap:.2f}")
    assert gap > 0.1
    h = fast.hermitian_part(g0)
    assert np.array_equal(h, h.conj().T)


@pytest.fixture
def no_device_needed(lib, monkeypatch):
    """the checks below raise before any library call: let the binding get as far as its argument checks without a GPU"""
    from c3_amd import _lib

    monkeypatch.setattr(_lib, "require_gpu", lambda: None)


def test_hermitian_basis_keyword_argument_checks(no_device_needed):
    from c3_amd import propagation
    from c3_amd._lib import C3PropError

    h0, hks, col, sig, dt, Ubar, ph = _problem(2, 2, 4, 7)
    with pytest.raises(C3PropError, match="hermitian_basis.*want_model_grads"):
        propagation.propagate_batch_lindblad_vjp(h0, hks, sig[None], dt, col, Ubar[None], hermitian_basis=True)
    kw = dict(want_model_grads=True, hermitian_basis=True)
    with pytest.raises(C3PropError, match=r"U_bar must be \[1,4,4\]"):
        propagation.propagate_batch_lindblad_vjp(h0, hks, sig[None], dt, col, Ubar[None, :2, :2], **kw)
    with pytest.raises(C3PropError, match="needs collapse operators"):
        propagation.propagate_batch_lindblad_vjp(h0, hks, sig[None], dt, None, Ubar[None], **kw)
    with pytest.raises(C3PropError, match=r"fr_phase must be \[1,4\]"):
        propagation.propagate_batch_lindblad_vjp(h0, hks, sig[None], dt, col, Ubar[None], fr_phase=ph[None, :2], **kw)
