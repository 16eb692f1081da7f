"""The core + border chain step of the small-D real loop (chain_step8<NC>: direct border sums, the row border reduced by a matrix
instruction against ones as the A operand) on the lane-level model of tests/chain_border_model.py.  No GPU."""
import numpy as np
import pytest

import chain_border_model as cbm


def operands(nc, seed):
    """C = cos Y, S = sin Y of one random symmetric Y (symmetric, commuting), a random complex U; D = 4 nc + 1"""
    rng = np.random.default_rng(seed)
    D = 4 * nc + 1
    Y = rng.standard_normal((D, D))
    Y = 0.5 * (Y + Y.T)
    w, V = np.linalg.eigh(Y)
    C, S = (V * np.cos(w)) @ V.T, (V * np.sin(w)) @ V.T
    U = rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D))
    return 0.5 * (C + C.T), 0.5 * (S + S.T), U


def test_mfma_against_ones():
    rng = np.random.default_rng(0)
    t, acc = rng.standard_normal((4, 4)), rng.standard_normal((4, 4))
    row = cbm.mfma4(cbm.ONES, t, acc)
    col = cbm.mfma4(t, cbm.ONES, acc)
    for i in range(4):
        for j in range(4):
            assert row[i, j] == pytest.approx(t[:, j].sum() + acc[i, j], abs=1e-15)
            assert col[i, j] == pytest.approx(t[:, i].sum() + acc[i, j], abs=1e-15)


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_step_is_the_complex_product(nc, seed):
    C, S, U = operands(nc, seed)
    Ur, Ui = cbm.GMat(U.real.copy()), cbm.GMat(U.imag.copy())
    cbm.chain_step8(cbm.SMat(C), cbm.SMat(S), Ur, Ui)
    got = Ur.dense() + 1j * Ui.dense()
    want = (C - 1j * S) @ U
    assert np.abs(got - want).max() < 1e-14
    # the row border is replicated over r, the column border and the corner over c, as GMat holds them
    for G in (Ur, Ui):
        for I in range(nc):
            assert np.array_equal(G.rc[I], np.repeat(G.rc[I][:1, :], 4, axis=0))
            assert np.array_equal(G.cr[I], np.repeat(G.cr[I][:, :1], 4, axis=1))
        assert np.array_equal(G.s, np.full((4, 4), G.s[0, 0]))


@pytest.mark.parametrize("nc", [1, 2])
def test_identity_step_passes_the_state_through(nc):
    """a masked slot applies the step with E = I: the border (direct form) comes back bit for bit, the core to the rounding of its
    3M recombination (Im = ((Ur + Ui) - Ur) + 0)"""
    _, _, U = operands(nc, 7)
    D = 4 * nc + 1
    Ur, Ui = cbm.GMat(U.real.copy()), cbm.GMat(U.imag.copy())
    cbm.chain_step8(cbm.SMat(np.eye(D)), cbm.SMat(np.zeros((D, D))), Ur, Ui)
    got = Ur.dense() + 1j * Ui.dense()
    assert np.array_equal(got[D - 1, :], U[D - 1, :]) and np.array_equal(got[:, D - 1], U[:, D - 1])
    assert np.abs(got - U).max() < 1e-14
