"""Pin the oracle's sequence fidelities (RB, ORBIT, analytical EPC; oracle/c3_oracle.py) to closed forms, with the
reference's Clifford decomposition read from tests/golden/clifford_rb.json.  numpy only: the project's package is not
imported, so these pins are independent of what they are later used to check.  Runs without a GPU."""
import json
import os

import numpy as np
import pytest

from oracle import c3_oracle as o

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GENS = ("rx90p", "rx90m", "ry90p", "ry90m")
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)


def fixture_words():
    with open(os.path.join(GOLDEN, "clifford_rb.json")) as f:
        return json.load(f)


def alternative_words():
    """the fixture's table with C4 and C16 spelled by other words of the same element (as a breadth-first search
    finds them): rx90p rx90p ry90m and rx90p rx90p ry90p"""
    w = [list(x) for x in fixture_words()]
    w[3] = ["rx90p", "rx90p", "ry90m"]
    w[15] = ["rx90p", "rx90p", "ry90p"]
    return w


def same_up_to_phase(A, B, tol=1e-12):
    return abs(abs(np.trace(A.conj().T @ B)) - A.shape[0]) < tol


def rotation(theta, n):
    """exp(-i theta/2 n.sigma)"""
    n = np.asarray(n, dtype=np.float64) / np.linalg.norm(n)
    H = n[0] * X + n[1] * Y + n[2] * Z
    return np.cos(theta / 2) * np.eye(2) - 1j * np.sin(theta / 2) * H


def coherent_generators(target=0):
    """rx90p over-rotated by 2 % with a 0.01 rad tilt of its axis towards Z, ry90p under-rotated by 2 % with a -0.02 rad
    tilt, the other two exact"""
    g = dict(o.RB_GENERATORS)
    g["rx90p"] = rotation(np.pi / 2 * 1.02, [np.cos(0.01), 0, np.sin(0.01)])
    g["ry90p"] = rotation(np.pi / 2 * 0.98, [0, np.cos(-0.02), np.sin(-0.02)])
    return {f"{k}[{target}]": v for k, v in g.items()}


def depolarizing(p):
    """rho -> p rho + (1 - p) tr(rho) I / 2 as a superoperator (vec(I) is the same row- or column-major)"""
    v = np.eye(2).reshape(-1)
    return p * np.eye(4) + (1 - p) / 2 * np.outer(v, v)


def embed(U, D):
    V = np.eye(D, dtype=np.complex128)
    V[:2, :2] = U
    return V


def test_fixture_is_names_only():
    words = fixture_words()
    assert len(words) == 24 and all(isinstance(w, list) and w for w in words)
    assert {g for w in words for g in w} == set(GENS)


@pytest.mark.parametrize("words", [fixture_words(), alternative_words()], ids=["reference", "alternative"])
def test_words_are_the_clifford_group(words):
    C = o.clifford_table(words)
    for a in range(24):
        assert np.allclose(C[a].conj().T @ C[a], np.eye(2), atol=1e-14)
        for b in range(a):
            assert not same_up_to_phase(C[a], C[b], 1e-9), (a, b)
    for a in range(24):  # closed: every product is one of the 24
        for b in range(24):
            assert sum(same_up_to_phase(C[b] @ C[a], C[c], 1e-9) for c in range(24)) == 1
    assert same_up_to_phase(C[0], np.eye(2))  # C1 is the identity, rx90p rx90m


def test_tables_name_the_same_elements():
    A, B = o.clifford_table(fixture_words()), o.clifford_table(alternative_words())
    for k in range(24):
        assert same_up_to_phase(A[k], B[k])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_rb_sequences_multiply_to_identity(seed):
    words = fixture_words()
    np.random.seed(seed)
    for L in (1, 2, 3, 10, 41):
        seqs = o.single_length_RB(7, L, 2, words)
        assert len(seqs) == 7
        for s in seqs:
            assert all(g.endswith("[2]") and g[:-3] in GENS for g in s)
            U = o.evaluate_sequences({f"{g}[2]": v for g, v in o.RB_GENERATORS.items()}, [s])[0]
            assert same_up_to_phase(U, np.eye(2)), (L, s)


def test_inverseC_is_the_trace_search():
    words = fixture_words()
    C = o.clifford_table(words)
    rng = np.random.default_rng(4)
    for _ in range(40):
        seq = rng.integers(1, 25, size=int(rng.integers(0, 9)))
        inv = o.inverseC(seq, words)
        U = np.eye(2, dtype=np.complex128)
        for c in list(seq) + [inv]:
            U = C[c - 1] @ U
        assert same_up_to_phase(U, np.eye(2))


@pytest.mark.parametrize("D", [2, 3])
def test_ideal_gates_survive_and_have_zero_epc(D):
    words = fixture_words()
    gates = {f"{g}[0]": embed(o.RB_GENERATORS[g], D) for g in GENS}
    supers = {k: o.tf_super(v) for k, v in gates.items()}
    assert abs(o.epc_analytical(gates, [0], [D], words)) < 1e-14
    assert abs(o.lindbladian_epc_analytical(supers, [0], [D], words)) < 1e-14
    np.random.seed(5)
    seqs = o.single_length_RB(6, 15, 0, words)
    assert np.abs(o.rb_pop0(gates, seqs) - 1).max() < 1e-13
    assert np.abs(o.rb_pop0(supers, seqs, lindbladian=True) - 1).max() < 1e-13
    assert abs(o.orbit_infid(gates, seqs)) < 1e-13 and abs(o.orbit_infid(supers, seqs, lindblad_population=True)) < 1e-13


def test_rb_fit_of_ideal_gates():
    """ideal gates: every survival is 1 up to rounding, so the standard errors the fit divides by are 0 or rounding
    noise and the reference's weighted fit is not defined there; an error of 1e-9 per gate already gives r = 1 to 1e-6"""
    words = fixture_words()
    lengths = [2, 5, 20, 50, 100]
    ideal = {f"{g}[0]": o.tf_super(v) for g, v in o.RB_GENERATORS.items()}
    np.random.seed(1)
    seqs = [o.single_length_RB(8, L, 0, words) for L in lengths]
    assert np.abs(np.array([o.rb_pop0(ideal, q, lindbladian=True) for q in seqs]) - 1).max() < 1e-13
    near = {k: depolarizing(1 - 1e-9) @ v for k, v in ideal.items()}
    epg, r, surv = o.RB(near, lengths, seqs, lindbladian=True)
    assert 1 - 1e-6 < r <= 1 and 0 <= epg < 1e-6
    assert np.abs(surv - 1).max() < 1e-6  # (1 - p^n) / 2 with n up to ~250 generators


@pytest.mark.parametrize("p", [0.99, 0.9])
def test_depolarizing_noise_closed_forms(p):
    """gate-independent depolarizing Lambda_p after every ideal generator: a sequence of n generators is Lambda_{p^n}
    (Lambda_p commutes with unitary channels) times the identity, so pop_0 = 1/2 + p^n / 2; a Clifford of w generators
    has average fidelity (1 + p^w) / 2, so the Lindblad EPC is the mean over c of (1 - p^(w_c)) / 2"""
    words = fixture_words()
    supers = {f"{g}[0]": depolarizing(p) @ o.tf_super(v) for g, v in o.RB_GENERATORS.items()}
    np.random.seed(7)
    for L in (1, 4, 25):
        seqs = o.single_length_RB(9, L, 0, words)
        n = np.array([len(s) for s in seqs])
        want = 0.5 + 0.5 * p**n
        assert np.abs(o.rb_pop0(supers, seqs, lindbladian=True) - want).max() < 1e-13
        assert o.orbit_infid(supers, seqs, lindblad_population=True) == pytest.approx(np.mean(1 - want), abs=1e-13)
        # the reference's literal ORBIT squares the Lindblad population
        assert o.orbit_infid(supers, seqs) == pytest.approx(np.mean(1 - want**2), abs=1e-13)
    want = np.mean([(1 - p ** len(w)) / 2 for w in words])
    assert o.lindbladian_epc_analytical(supers, [0], [2], words) == pytest.approx(want, abs=1e-14)


@pytest.mark.parametrize("theta", [0.0, 0.03, 0.4, 2.0])
@pytest.mark.parametrize("D", [2, 3])
def test_single_coherent_rotation_closed_form(theta, D):
    """average fidelity of a rotation by theta: (|tr U|^2 / 2 + 1) / 3 = (2 cos^2(theta / 2) + 1) / 3.  With C_k = E C_k^ideal
    for one error E, every Clifford's error C_k^+ E^+ C_k is a rotation by the same angle, so EPC = 1 - F exactly."""
    words = fixture_words()
    E = rotation(theta, [0.3, -0.5, 0.8])
    F = (2 * np.cos(theta / 2) ** 2 + 1) / 3
    assert o.tf_average_fidelity(E, np.eye(2), lvls=[2]) == pytest.approx(F, abs=1e-15)
    C = o.clifford_table(words)
    keyed = {f"C{k + 1}": embed(E @ C[k], D) for k in range(24)}
    assert o.epc_analytical(keyed, [0], [D], words, cliffords=True) == pytest.approx(1 - F, abs=1e-15)
    skeyed = {k: o.tf_super(v) for k, v in keyed.items()}
    assert o.lindbladian_epc_analytical(skeyed, [0], [D], words, cliffords=True) == pytest.approx(1 - F, abs=1e-15)


def test_coherent_epc_depends_on_the_words():
    """the two tables name the same 24 elements, but with imperfect generators the products of their words differ:
    the EPC from the generators is not a property of the group alone"""
    g = coherent_generators()
    ref = o.epc_analytical(g, [0], [2], fixture_words())
    alt = o.epc_analytical(g, [0], [2], alternative_words())
    assert 1e-4 < ref < 1e-3 and 1e-4 < alt < 1e-3
    assert abs(ref - alt) > 0.05 * ref, (ref, alt)
    s = {k: o.tf_super(v) for k, v in g.items()}
    assert o.lindbladian_epc_analytical(s, [0], [2], fixture_words()) == pytest.approx(ref, abs=1e-14)
    assert o.lindbladian_epc_analytical(s, [0], [2], alternative_words()) == pytest.approx(alt, abs=1e-14)


def test_populations_as_the_reference():
    v = np.array([0.6, 0.8j])
    assert np.allclose(o.populations(v, False), [0.36, 0.64])
    rho = np.array([[0.7, 0.1j], [-0.1j, -0.3]])  # not a state: |.| of the diagonal entries
    assert np.allclose(o.populations(rho.reshape(-1), True), [0.7, 0.3])
