"""The chain step of the small-D real loop with the column border and the corner of the state packed (chain_step8<NC> with
GBorder<NC>) on the lane-level model of tests/chain_packed_model.py, NC = 1 and 2.  No GPU.

* the packed step is the dense complex product: over 50 dependent steps to 1e-13 of the state's norm, and one step against
  chain_border_model.chain_step8 to rounding (the bound: the two form a border element from the same 2 D products in a different
  order, each sum within D ulp of its absolute sum -- 2 D eps times sum_k |E_ik| |U_kj| <= 2 D eps sqrt(D) max|U| sqrt(D));
* pack followed by unpack is the identity; a step with C = I, S = 0 (a padded slot) leaves the packed registers unchanged;
* the packed registers keep their form, {x, y, -x, -y} over c, bit for bit through the steps.
* guard inputs: on every case of tests/test_gpu_smalld_packed_border.py each of four wrong steps (rotation the other way, the corner
  term left out of the column, S.s Qs left out of the corner, Re and Im swapped at unpack) moves the model's result by more than 1e-6,
  so the 1e-11 bar of the GPU tests cannot pass such a step; and the right step is within 1e-12 of the oracle there."""
import numpy as np
import pytest

import chain_border_model as cbm
import chain_packed_model as cpm
from test_chain_border_model import operands

EPS = 2.0**-52


def packed_form(p):
    return np.array_equal(p[:, 2], -p[:, 0]) and np.array_equal(p[:, 3], -p[:, 1])


@pytest.mark.parametrize("nc", [1, 2])
def test_pack_then_unpack_is_the_identity(nc):
    _, _, U = operands(nc, 5)
    st = cpm.State(U)
    assert np.array_equal(st.dense(), U)
    for P in st.Ub.Pc + [st.Ub.Ps]:
        assert packed_form(P)
    assert np.array_equal(st.Ub.Ps, np.repeat(st.Ub.Ps[:1, :], 4, axis=0))
    # the rotation is -i times the packed vector
    D = 4 * nc + 1
    rot = cpm.Border(U)
    rot.Pc, rot.Ps = [cpm.quad_rot(P) for P in st.Ub.Pc], cpm.quad_rot(st.Ub.Ps)
    assert np.array_equal(rot.column(), -1j * U[:, D - 1])


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_step_is_the_complex_product_and_the_unpacked_step(nc, seed):
    C, S, U = operands(nc, seed)
    D = 4 * nc + 1
    st = cpm.State(U)
    cpm.chain_step(cbm.SMat(C), cbm.SMat(S), st)
    got = st.dense()
    assert np.abs(got - (C - 1j * S) @ U).max() < 1e-14
    Ur, Ui = cbm.GMat(U.real.copy()), cbm.GMat(U.imag.copy())
    cbm.chain_step8(cbm.SMat(C), cbm.SMat(S), Ur, Ui)
    old = Ur.dense() + 1j * Ui.dense()
    # core and row border are formed as before
    assert np.array_equal(got[:, : D - 1], old[:, : D - 1])
    bound = 2 * D * EPS * D * np.abs(U).max()
    err = np.abs(got[:, D - 1] - old[:, D - 1]).max()
    print(f"nc = {nc}, seed {seed}: packed against unpacked border column {err:.2e} (bound {bound:.2e})")
    assert err < bound
    for P in st.Ub.Pc + [st.Ub.Ps]:
        assert packed_form(P)
    assert np.array_equal(st.Ub.Ps, np.repeat(st.Ub.Ps[:1, :], 4, axis=0))


@pytest.mark.parametrize("nc", [1, 2])
def test_fifty_dependent_steps(nc):
    """unitary steps: the state's norm stays sqrt(D) times the start's scale"""
    D = 4 * nc + 1
    _, _, U = operands(nc, 11)
    st, want = cpm.State(U), U.copy()
    for n in range(50):
        C, S, _ = operands(nc, 100 + n)
        cpm.chain_step(cbm.SMat(C), cbm.SMat(S), st)
        want = (C - 1j * S) @ want
        for P in st.Ub.Pc + [st.Ub.Ps]:
            assert packed_form(P)
    err = np.abs(st.dense() - want).max() / np.linalg.norm(want)
    print(f"nc = {nc}: 50 steps, max |packed - dense| / |U|_F = {err:.2e}")
    assert err < 1e-13
    assert D == want.shape[0]


@pytest.mark.parametrize("nc", [1, 2])
def test_identity_step_leaves_the_packed_state_unchanged(nc):
    _, _, U = operands(nc, 7)
    D = 4 * nc + 1
    st = cpm.State(U)
    before = [P.copy() for P in st.Ub.Pc + [st.Ub.Ps]]
    cpm.chain_step(cbm.SMat(np.eye(D)), cbm.SMat(np.zeros((D, D))), st)
    for P, P0 in zip(st.Ub.Pc + [st.Ub.Ps], before):
        assert np.array_equal(P, P0)
    got = st.dense()
    assert np.array_equal(got[D - 1, :], U[D - 1, :]) and np.array_equal(got[:, D - 1], U[:, D - 1])
    assert np.abs(got - U).max() < 1e-14


WRONG = {
    "rotation the other way": dict(rot=3),
    "corner term left out of the column": dict(corner_in_column=False),
    "S.s Qs left out of the corner": dict(ss_in_corner=False),
    "Re and Im swapped at unpack": dict(swap=True),
}


@pytest.mark.parametrize("nc", [1, 2])
def test_wrong_rotation_conjugates_the_border_column(nc):
    """what the first wrong step is: i u in place of -i u, i.e. E-bar applied to the border column"""
    C, S, U = operands(nc, 3)
    D = 4 * nc + 1
    st = cpm.State(U)
    cpm.chain_step(cbm.SMat(C), cbm.SMat(S), st, rot=3)
    assert np.abs(st.dense()[:, D - 1] - ((C + 1j * S) @ U)[:, D - 1]).max() < 1e-14


def _gpu_cases():
    import test_gpu_smalld_packed_border as g

    return g


def _case_names():
    return list(_gpu_cases().CASES)


@pytest.mark.parametrize("name", _case_names())
def test_gpu_inputs_tell_a_wrong_step(name):
    g = _gpu_cases()
    c = g.case(name)
    D = c["D"]
    small = min(min(np.abs(r[:, D - 1].real).min(), np.abs(r[:, D - 1].imag).min()) for r in c["ref"])
    print(f"{name}: smallest |Re|, |Im| on the reference's border column {small:.3e}")
    assert small > 1e-2
    seg = g.seg_edges(c)
    moved = {w: np.inf for w in WRONG}
    for b in range(c["sig"].shape[0]):
        right = cpm.propagate(c["h0"], c["hks"], c["sig"][b], c["dt"], seg)
        # the model chains what the oracle computes, up to the scalar phase of the trace shift and the row phases
        want = np.exp(-1j * c["ph"][b])[:, None] * c["ref"][b]
        k = np.unravel_index(np.abs(want).argmax(), want.shape)
        assert np.abs(right * (want[k] / right[k]) - want).max() < 1e-12
        assert abs(abs(want[k] / right[k]) - 1) < 1e-12
        for w, kw in WRONG.items():
            moved[w] = min(moved[w], np.abs(cpm.propagate(c["h0"], c["hks"], c["sig"][b], c["dt"], seg, **kw) - right).max())
    for w, m in moved.items():
        print(f"{name}: {w}: moves the result by {m:.3e}")
        assert m > 1e-6, w
