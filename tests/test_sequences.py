"""Host side of the indexed sequence path (c3_amd/sequences.py, c3p_seq_chain): the derived Clifford table, RB sequence
generation, the RB fit and the ABI declaration.  No GPU."""
import os
import re

import numpy as np
import pytest

from c3_amd import _lib, sequences as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _equal_up_to_phase(A, B, tol=1e-12):
    k = np.argmax(np.abs(B))
    ph = A.flat[k] / B.flat[k]
    return abs(abs(ph) - 1) < tol and np.allclose(A, ph * B, atol=tol)


def test_clifford_table_is_the_group():
    C = sq.CLIFFORD_MATRICES
    assert len(sq.CLIFFORD_WORDS) == 24 and C.shape == (24, 2, 2)
    for i in range(24):
        assert np.allclose(C[i].conj().T @ C[i], np.eye(2), atol=1e-14)
        for j in range(i):
            assert not _equal_up_to_phase(C[i], C[j], 1e-9), (i, j)
    # closed under multiplication (and so a group: finite, contains the identity)
    for a in range(24):
        for b in range(24):
            sq.clifford_index(C[b] @ C[a])
    assert _equal_up_to_phase(C[0], np.eye(2))
    assert sq.CLIFFORD_WORDS[0] == ["rx90p", "rx90m"]


def test_clifford_words_reproduce_their_matrices():
    gens = sq._ideal_generators()
    for w, U in zip(sq.CLIFFORD_WORDS, sq.CLIFFORD_MATRICES):
        assert set(w) <= set(sq.GENERATORS)
        V = np.eye(2, dtype=complex)
        for g in w:  # first gate applied first
            V = gens[g] @ V
        assert np.allclose(V, U, atol=1e-14)
    # the generators are the reference's ideal gates (c3/libraries/constants.py)
    s = 1 / np.sqrt(2)
    assert np.allclose(gens["rx90p"], s * np.array([[1, -1j], [-1j, 1]]))
    assert np.allclose(gens["ry90m"], s * np.array([[1, 1], [-1, 1]]))


def test_words_are_shortest():
    """breadth-first: no element has a word longer than needed (the single generators have length 1)"""
    lens = sorted(len(w) for w in sq.CLIFFORD_WORDS[1:])
    assert lens[:4] == [1, 1, 1, 1] and max(lens) <= 4


@pytest.mark.parametrize("seed", range(20))
def test_rb_sequences_multiply_to_identity(seed):
    gens = sq._ideal_generators()
    rng = np.random.default_rng(seed)
    for L in (1, 2, 5, 37):
        seqs = sq.single_length_RB(6, L, target=3, rng=rng)
        assert len(seqs) == 6
        for s in seqs:
            assert all(re.fullmatch(r"r[xy]90[pm]\[3\]", g) for g in s)
            U = sq.word_matrix([g[:-3] for g in s], gens)
            assert _equal_up_to_phase(U, np.eye(2)), (L, s)


def test_inverseC_numbers_index_this_table():
    rng = np.random.default_rng(1)
    for _ in range(50):
        seq = rng.integers(1, 25, size=7)
        inv = sq.inverseC(seq)
        assert 1 <= inv <= 24
        U = np.eye(2, dtype=complex)
        for c in list(seq) + [inv]:
            U = sq.CLIFFORD_MATRICES[c - 1] @ U
        assert _equal_up_to_phase(U, np.eye(2))


def test_rb_index_table_matches_names():
    rng = np.random.default_rng(3)
    cl = sq._rb_cliffords(5, 9, rng)
    seqs, lengths = sq._rb_index_table(cl)
    for s in range(5):
        names = [g for c in cl[s] for g in sq.CLIFFORD_WORDS[c]]
        assert lengths[s] == len(names)
        assert [sq.GENERATORS[i] for i in seqs[s, : lengths[s]]] == names


def test_index_table_ragged_and_unknown_gate():
    seqs, lengths = sq.index_table([["a", "b", "a"], [], ["b"]], {"a": 0, "b": 1})
    assert seqs.shape == (3, 3) and list(lengths) == [3, 0, 1]
    assert list(seqs[0]) == [0, 1, 0] and seqs[2, 0] == 1
    with pytest.raises(_lib.C3PropError, match="C3:Error"):
        sq.index_table([["a", "c"]], {"a": 0})


@pytest.mark.parametrize("r_true", [0.97, 0.995])
def test_rb_fit_recovers_known_decay(r_true):
    lengths = np.rint(np.linspace(5, 500, 20)).astype(int)
    rng = np.random.default_rng(0)
    A, B = 0.48, 0.5
    surv = A * r_true ** lengths[:, None] + B + 1e-4 * rng.standard_normal((20, 30))
    r, A_fit, B_fit = sq.rb_fit(lengths, surv)
    assert abs(r - r_true) < 2e-4 and abs(A_fit - A) < 5e-3 and abs(B_fit - B) < 5e-3


def test_new_symbol_is_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "c3prop.h")).read()
    assert re.search(r"\bint c3p_seq_chain\s*\(", text)
    assert "c3p_seq_chain" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["c3p_seq_chain"][1]) == 14
    assert _lib.KERNEL_NAMES[9] == "seq"
    assert re.search(r"#define C3P_KERNEL_SEQ 9\b", text)


def test_library_exports_seq_chain(lib):
    assert hasattr(lib, "c3p_seq_chain")


def test_fidelities_are_registered():
    from c3_amd.fidelities import fidelities

    for name in ("RB", "orbit_infid", "epc_analytical", "lindbladian_epc_analytical", "lindbladian_RB_left", "lindbladian_RB_right"):
        assert name in fidelities, name


def _supplied_cliffords(perm, noise=0.0, rng=None, D=2):
    """C_k = CLIFFORD_MATRICES[perm[k]] (times a small random unitary), embedded in D levels: [1,24,D,D]"""
    out = np.zeros((24, D, D), dtype=complex)
    for k, c in enumerate(perm):
        U = sq.CLIFFORD_MATRICES[c]
        if noise:
            H = rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2))
            w, V = np.linalg.eigh(noise * (H + H.conj().T))
            U = (V * np.exp(-1j * w)) @ V.conj().T @ U
        out[k, :2, :2] = U * np.exp(1j * rng.uniform(0, 6.3) if rng is not None else 1)
        out[k, 2:, 2:] = np.eye(D - 2)
    return out[None]


@pytest.mark.parametrize("seed", range(5))
def test_match_cliffords_ignores_the_numbering(seed):
    """epc_analytical(cliffords=True) pairs each C_k with its own ideal element: any numbering, any global phase, noisy"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(24)
    for D in (2, 3):
        U = _supplied_cliffords(perm, 0.05, rng, D)
        assert np.array_equal(sq.match_cliffords(U, [0, 1]), perm)
        S = np.einsum("pkij,pkab->pkiajb", U, U.conj()).reshape(1, 24, D * D, D * D)
        assert np.array_equal(sq.match_cliffords(S, [0, 1], superop=True), perm)


def test_match_cliffords_refuses_what_is_not_the_group():
    rng = np.random.default_rng(0)
    perm = np.arange(24)
    perm[5] = 6  # two keys implement the same element, one element missing
    with pytest.raises(_lib.C3PropError, match="C3:Error"):
        sq.match_cliffords(_supplied_cliffords(perm, 0.0, rng), [0, 1])
    with pytest.raises(_lib.C3PropError, match="C3:Error"):
        sq.match_cliffords(_supplied_cliffords(np.arange(24), 1.5, rng), [0, 1])  # far from every Clifford


def test_distinct_cliffords_are_at_most_half_faithful():
    """the separation match_cliffords relies on: process fidelity |tr(C_a^+ C_b)|^2 / 4 <= 1/2 for a != b"""
    C = sq.CLIFFORD_MATRICES
    F = np.abs(np.einsum("aij,bij->ab", C.conj(), C)) ** 2 / 4
    assert np.allclose(np.diag(F), 1)
    np.fill_diagonal(F, 0)
    assert F.max() <= 0.5 + 1e-12


def test_epc_refuses_more_than_one_subsystem():
    """the reference switches to two-qubit Cliffords when len(dims) == 2; that group is not provided here"""
    gates = {f"{g}[0]": np.eye(9, dtype=complex) for g in sq.GENERATORS}
    for fn in (sq.epc_analytical, sq.lindbladian_epc_analytical):
        with pytest.raises(_lib.C3PropError, match="single-qubit"):
            fn(gates, [0], [3, 3], True)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's Clifford decomposition (tests/golden/clifford_rb.json), selectable by clifford_words
# ---------------------------------------------------------------------------------------------------------------------------
def _fixture_words():
    import json

    with open(os.path.join(ROOT, "tests", "golden", "clifford_rb.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("seed", [0, 7, 2026])
def test_reference_words_reproduce_the_reference_sequences(seed):
    """with the reference's words and numpy's global stream, single_length_RB returns exactly the oracle's restatement
    of qt_utils.py:448-478 for the same seed (one [n, L-1] draw takes the numbers of n draws of L - 1)"""
    from oracle import c3_oracle as o

    words = _fixture_words()
    for L in (1, 2, 9, 40):
        np.random.seed(seed)
        got = sq.single_length_RB(6, L, target=1, clifford_words=words)
        np.random.seed(seed)
        want = o.single_length_RB(6, L, 1, words)
        assert got == want, (seed, L)
    np.random.seed(seed)
    default = [sq.single_length_RB(6, L, target=1) for L in (9, 40)]
    np.random.seed(seed)
    assert default == [o.single_length_RB(6, L, 1, sq.CLIFFORD_WORDS) for L in (9, 40)]


def test_inverseC_with_the_reference_words_is_the_trace_search():
    from oracle import c3_oracle as o

    words = _fixture_words()
    rng = np.random.default_rng(8)
    for _ in range(50):
        seq = rng.integers(1, 25, size=int(rng.integers(0, 8)))
        assert sq.inverseC(seq, clifford_words=words) == o.inverseC(seq, words)
        assert sq.inverseC(seq) == o.inverseC(seq, sq.CLIFFORD_WORDS)


def test_default_table_spells_two_elements_differently():
    """the derived table names the reference's 24 elements, in another order, and spells C4 and C16 with other words:
    the difference epc_analytical sees under coherent errors"""
    ref = sq.clifford_table(_fixture_words())
    dft = sq.clifford_table()
    assert dft is sq.clifford_table(None) and dft.words == sq.CLIFFORD_WORDS
    differ = []
    for k in range(24):
        j = sq.clifford_index(ref.matrices[k])
        assert _equal_up_to_phase(dft.matrices[j], ref.matrices[k])
        if dft.words[j] != ref.words[k]:
            differ.append((k + 1, dft.words[j]))
    assert differ == [(4, ["rx90p", "rx90p", "ry90m"]), (16, ["rx90p", "rx90p", "ry90p"])]
    assert ref.identity == 0 and np.array_equal(ref.product[ref.inverse, np.arange(24)], np.zeros(24))


def test_clifford_table_refuses_what_is_not_the_group():
    words = _fixture_words()
    with pytest.raises(_lib.C3PropError, match="C3:Error"):
        sq.clifford_table(words[:23])
    with pytest.raises(_lib.C3PropError, match="distinct"):
        sq.clifford_table(words[:23] + [words[0]])
    with pytest.raises(_lib.C3PropError, match="unknown names"):
        sq.clifford_table(words[:23] + [["rz90p"]])


def test_global_stream_is_handed_on():
    """RB and rb_survival resolve rng=None to numpy's global stream once and pass it on: it must stay that stream (it
    was once re-read as a seed, so RB(rng=None), the reference's default, raised before drawing)"""
    r = sq._rng(None)
    assert r is np.random and sq._rng(r) is np.random
    np.random.seed(12)
    a = sq._rb_cliffords(4, 6, sq._rng(None))
    np.random.seed(12)
    assert np.array_equal(a, sq._rb_cliffords(4, 6, None))
    rs = np.random.RandomState(3)
    assert sq._rng(rs) is rs
    g = np.random.default_rng(3)
    assert sq._rng(g) is g
