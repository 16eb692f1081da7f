"""The sequence fidelities of c3_amd/sequences.py (RB, ORBIT, the analytical EPC, their Lindblad forms and the ORBIT
gradient) on the GPU, against the oracle's restatement of the reference's algorithm (oracle/c3_oracle.py), with both the
project's derived Clifford table and the reference's decomposition (tests/golden/clifford_rb.json).

P = 3 parameter samples per case, with coherent errors (over-rotations and tilted axes of different sizes per sample)
and, for superoperators, amplitude damping and dephasing.  Tolerances as tests/test_gpu_sequences.py: values built from
chains of at most a few hundred near-unitary factors agree to 1e-12; fitted decay rates to 1e-6 (curve_fit's own
tolerance, see there).
"""
import json
import os

import numpy as np
import pytest

from oracle import c3_oracle as o

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
GENS = ("rx90p", "rx90m", "ry90p", "ry90m")
P = 3
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)


@pytest.fixture(scope="module")
def sq(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from c3_amd import sequences

    return sequences


def fixture_words():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clifford_rb.json")) as f:
        return json.load(f)


def table(sq, which):
    """(clifford_words to pass to c3_amd, words for the oracle)"""
    return (None, sq.CLIFFORD_WORDS) if which == "default" else (fixture_words(), fixture_words())


def rotation(theta, n):
    n = np.asarray(n, dtype=np.float64) / np.linalg.norm(n)
    return np.cos(theta / 2) * np.eye(2) - 1j * np.sin(theta / 2) * (n[0] * X + n[1] * Y + n[2] * Z)


def coherent(D=2, scale=(1.0, 0.5, 2.0)):
    """{name[0]: [P,D,D]}: sample p has rx90p over-rotated by 2 scale[p] % with a 0.01 scale[p] rad tilt towards Z, ry90p
    under-rotated by 2 scale[p] % with a -0.02 scale[p] rad tilt, the other two exact (sample 0: the issue's example);
    embedded in D levels with the extra levels idle"""
    out = {}
    for g in GENS:
        V = np.zeros((P, D, D), dtype=np.complex128)
        for p, a in enumerate(scale):
            if g == "rx90p":
                U = rotation(np.pi / 2 * (1 + 0.02 * a), [np.cos(0.01 * a), 0, np.sin(0.01 * a)])
            elif g == "ry90p":
                U = rotation(np.pi / 2 * (1 - 0.02 * a), [0, np.cos(-0.02 * a), np.sin(-0.02 * a)])
            else:
                U = o.RB_GENERATORS[g]
            V[p, :2, :2] = U
            V[p, 2:, 2:] = np.eye(D - 2)
        out[f"{g}[0]"] = V
    return out


def lindblad_noise(D, gamma, gphi):
    """exp of amplitude damping (rate gamma, lowering operator) plus dephasing (rate gphi, number operator) for unit time,
    as a superoperator on row-major vec (the convention of o.tf_super: vec(A rho B) = (A (x) B^T) vec(rho))"""
    from scipy.linalg import expm

    a = np.diag(np.sqrt(np.arange(1, D)), 1).astype(np.complex128)
    n = a.conj().T @ a
    I = np.eye(D)
    L = np.zeros((D * D, D * D), dtype=np.complex128)
    for c, r in ((a, gamma), (n, gphi)):
        cd = c.conj().T @ c
        L += r * (np.kron(c, c.conj()) - 0.5 * np.kron(cd, I) - 0.5 * np.kron(I, cd.T))
    return expm(L)


def noisy_supers(gates, D):
    """{name: [P,D^2,D^2]}: damping and dephasing of a different strength per sample after each coherent gate"""
    out = {}
    for k, V in gates.items():
        out[k] = np.stack([lindblad_noise(D, 2e-3 * (p + 1), 1e-3 * (3 - p)) @ o.tf_super(V[p]) for p in range(P)])
    return out


def dev(d):
    return {k: torch.as_tensor(v, device=DEV) for k, v in d.items()}


def sample(d, p):
    return {k: v[p] for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# analytical EPC
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["default", "reference"])
@pytest.mark.parametrize("D", [2, 3])
def test_epc_matches_oracle(sq, which, D):
    cw, words = table(sq, which)
    g = coherent(D)
    s = noisy_supers(g, D)
    got = sq.epc_analytical(dev(g), [0], [D], True, clifford_words=cw)
    want = [o.epc_analytical(sample(g, p), [0], [D], words) for p in range(P)]
    assert np.all(np.asarray(want) > 1e-5) and np.abs(got - want).max() < 1e-12, (got, want)
    got = sq.lindbladian_epc_analytical(dev(s), [0], [D], True, clifford_words=cw)
    want = [o.lindbladian_epc_analytical(sample(s, p), [0], [D], words) for p in range(P)]
    assert np.abs(got - want).max() < 1e-12, (got, want)


def test_epc_depends_on_the_table(sq):
    """the same coherent gates give another EPC with the derived words than with the reference's: the two agree with
    the oracle computed with the same words, and differ from each other by far more than rounding"""
    g = dev(coherent(2))
    ref = sq.epc_analytical(g, [0], [2], True, clifford_words=fixture_words())
    dft = sq.epc_analytical(g, [0], [2], True)
    assert abs(ref[0] - o.epc_analytical(sample(coherent(2), 0), [0], [2], fixture_words())) < 1e-12
    assert abs(dft[0] - o.epc_analytical(sample(coherent(2), 0), [0], [2], sq.CLIFFORD_WORDS)) < 1e-12
    assert np.all(np.abs(ref - dft) > 0.05 * ref), (ref, dft)


@pytest.mark.parametrize("D", [2, 3])
def test_epc_of_cliffords_keyed_in_the_reference_numbering(sq, D):
    """cliffords=True with C1..C24 in the reference's numbering, each the product of its fixture word's actual gates: the
    oracle's literal pairing of C_k with the ideal of word k, and the generator route with the reference's words"""
    words = fixture_words()
    g = coherent(D)
    s = noisy_supers(g, D)
    for gates, fn, ofn in ((g, sq.epc_analytical, o.epc_analytical), (s, sq.lindbladian_epc_analytical, o.lindbladian_epc_analytical)):
        keyed = {f"C{k + 1}": np.stack([o.evaluate_sequences(sample(gates, p), [[f"{x}[0]" for x in words[k]]])[0] for p in range(P)]) for k in range(24)}
        got = fn(dev(keyed), [0], [D], True, cliffords=True)
        want = [ofn(sample(keyed, p), [0], [D], words, cliffords=True) for p in range(P)]
        assert np.abs(got - want).max() < 1e-12, (got, want)
        gen = fn(dev(gates), [0], [D], True, clifford_words=words)
        assert np.abs(got - gen).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# RB and ORBIT with the same seeded sequences
# ---------------------------------------------------------------------------------------------------------------------------
LENGTHS = [2, 32, 62, 92, 122]  # = RB's lengths for min_length 2, max_length 122, num_lengths 5


@pytest.mark.parametrize("which", ["default", "reference"])
def test_rb_survival_and_fit_match_oracle(sq, which):
    cw, words = table(sq, which)
    g = coherent(2, scale=(3.0, 1.5, 6.0))
    np.random.seed(21)
    surv = sq.rb_survival(dev(g), LENGTHS, 12, clifford_words=cw)
    np.random.seed(21)
    seqs = [o.single_length_RB(12, L, 0, words) for L in LENGTHS]
    for p in range(P):
        want = np.array([o.rb_pop0(sample(g, p), q) for q in seqs])
        assert np.abs(surv[p] - want).max() < 1e-12, p
    kw = dict(min_length=2, max_length=122, num_lengths=5, num_seqs=12)
    np.random.seed(22)
    epg, r = sq.RB(dev(g), clifford_words=cw, return_fit=True, **kw)
    np.random.seed(22)
    seqs = [o.single_length_RB(12, L, 0, words) for L in LENGTHS]
    for p in range(P):
        epg_o, r_o, _ = o.RB(sample(g, p), LENGTHS, seqs)
        assert abs(r[p] - r_o) < 1e-6 and abs(epg[p] - epg_o) < 1e-6, (p, r[p], r_o)
    assert np.all((r < 1) & (r > 0.9))


@pytest.mark.parametrize("which", ["default", "reference"])
@pytest.mark.parametrize("D", [2, 3])
def test_orbit_matches_oracle(sq, which, D):
    cw, words = table(sq, which)
    g = coherent(D, scale=(3.0, 1.5, 6.0))
    np.random.seed(31)
    got = sq.orbit_infid(dev(g), RB_number=20, RB_length=25, clifford_words=cw)
    np.random.seed(31)
    seqs = o.single_length_RB(20, 25, 0, words)
    want = [o.orbit_infid(sample(g, p), seqs) for p in range(P)]
    assert np.all(np.asarray(want) > 1e-4) and np.abs(got - want).max() < 1e-12, (got, want)


@pytest.mark.parametrize("lindbladian", [False, True])
def test_orbit_gradient_against_oracle_differences(sq, lindbladian):
    """d infid = Re sum conj(U_bar) dU against central differences of the ORACLE's orbit_infid (h = 1e-6: truncation
    O(h^2), rounding ~eps / h = 1e-10 of values O(1))"""
    words = fixture_words()
    g = coherent(2, scale=(3.0, 1.5, 6.0))
    props = noisy_supers(g, 2) if lindbladian else g
    np.random.seed(41)
    seqs = o.single_length_RB(10, 12, 0, words)
    val, grads = sq.orbit_infid_with_grad(dev(props), seqs=seqs, lindbladian=lindbladian)
    grads = {k: v.cpu().numpy() for k, v in grads.items()}
    rng = np.random.default_rng(4)
    h = 1e-6
    for p in range(P):
        base = sample(props, p)
        f0 = o.orbit_infid(base, seqs, lindblad_population=lindbladian)
        assert abs(val[p] - f0) < 1e-12
        for _ in range(3):
            E = {k: rng.normal(size=v.shape) + 1j * rng.normal(size=v.shape) for k, v in base.items()}
            fp = o.orbit_infid({k: base[k] + h * E[k] for k in base}, seqs, lindblad_population=lindbladian)
            fm = o.orbit_infid({k: base[k] - h * E[k] for k in base}, seqs, lindblad_population=lindbladian)
            fd = (fp - fm) / (2 * h)
            an = sum(float(np.sum(np.conj(grads[k][p]) * E[k]).real) for k in base)
            assert an == pytest.approx(fd, rel=1e-6, abs=1e-9), (p, an, fd)


# ---------------------------------------------------------------------------------------------------------------------------
# Lindblad RB and ORBIT: the project's convention |x0| and the reference's literal |x0|^2
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["default", "reference"])
def test_lindblad_rb_and_orbit_conventions(sq, which):
    """lindbladian_RB_left/right and orbit_infid(lindbladian=True) use the population |(S vec(|0><0|))[0]| (the oracle's
    populations(lindbladian=True)); the reference's own calls square that entry (RB without lindbladian=True, ORBIT
    always): the literal values are the squares of the project's per-sequence populations"""
    cw, words = table(sq, which)
    s = noisy_supers(coherent(2, scale=(3.0, 1.5, 6.0)), 2)
    sd = dev(s)
    kw = dict(min_length=2, max_length=122, num_lengths=5, num_seqs=12)
    for fn in (sq.lindbladian_RB_left, sq.lindbladian_RB_right):
        np.random.seed(51)
        epg, r = fn(sd, clifford_words=cw, return_fit=True, **kw)
        np.random.seed(51)
        seqs = [o.single_length_RB(12, L, 0, words) for L in LENGTHS]
        for p in range(P):
            _, r_o, surv = o.RB(sample(s, p), LENGTHS, seqs, lindbladian=True)
            assert abs(r[p] - r_o) < 1e-6, (p, r[p], r_o)
            literal = np.array([o.rb_pop0(sample(s, p), q) for q in seqs])  # what the reference's RB fits
            assert np.abs(literal - surv**2).max() < 1e-12
    np.random.seed(52)
    seqs = o.single_length_RB(20, 25, 0, words)
    got = sq.orbit_infid(sd, seqs=seqs, lindbladian=True)
    pop = sq.evaluate_sequences_indexed(sd, seqs, "population", superop=True).cpu().numpy()
    for p in range(P):
        assert abs(got[p] - o.orbit_infid(sample(s, p), seqs, lindblad_population=True)) < 1e-12
        assert abs(o.orbit_infid(sample(s, p), seqs) - np.mean(1 - pop[p] ** 2)) < 1e-12
    assert np.all(got > 1e-3)


@pytest.mark.parametrize("which", ["default", "reference"])
def test_depolarizing_populations_are_exact(sq, which):
    """gate-independent depolarizing after ideal generators (M = 4): every sequence of n generators has
    pop_0 = 1/2 + p^n / 2, and the Lindblad EPC is the mean over the words of (1 - p^w) / 2"""
    cw, words = table(sq, which)
    ps = np.array([0.999, 0.99, 0.95])
    v = np.eye(2).reshape(-1)
    sup = {f"{g}[0]": np.stack([(p * np.eye(4) + (1 - p) / 2 * np.outer(v, v)) @ o.tf_super(o.RB_GENERATORS[g]) for p in ps]) for g in GENS}
    sd = dev(sup)
    for L in (1, 7, 60):
        seqs = sq.single_length_RB(15, L, rng=L, clifford_words=cw)
        n = np.array([len(q) for q in seqs])
        pop = sq.evaluate_sequences_indexed(sd, seqs, "population", superop=True).cpu().numpy()
        assert np.abs(pop - (0.5 + 0.5 * ps[:, None] ** n[None])).max() < 1e-13, L
    got = sq.lindbladian_epc_analytical(sd, [0], [2], True, clifford_words=cw)
    want = [np.mean([(1 - p ** len(w)) / 2 for w in words]) for p in ps]
    assert np.abs(got - want).max() < 1e-13


def test_product_mode_matches_oracle_evaluate_sequences(sq):
    """evaluate_sequences_indexed in product mode against the oracle's evaluate_sequences (propagation.py:588-627) on
    name lists that include empty sequences (the identity)"""
    rng = np.random.default_rng(6)
    names = ["a", "b", "c[1]", "d"]
    M = 3
    Us = {}
    for k in names:
        Z_ = rng.normal(size=(P, M, M)) + 1j * rng.normal(size=(P, M, M))
        Us[k] = np.linalg.qr(Z_)[0]
    seqs = [[names[i] for i in rng.integers(0, 4, size=L)] for L in (0, 1, 5, 0, 33, 2)]
    got = sq.evaluate_sequences_indexed(dev(Us), seqs, "product").cpu().numpy()
    for p in range(P):
        want = np.stack(o.evaluate_sequences(sample(Us, p), seqs))
        assert np.abs(got[p] - want).max() < 1e-12
    assert np.array_equal(got[:, 0], np.broadcast_to(np.eye(M), (P, M, M)))
