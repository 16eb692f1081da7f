"""c3p_seq_chain and the sequence fidelities on the GPU, against a numpy loop written here.

Tolerance: a chain of L matrix-vector products of M x M unitaries accumulates at most ~L * M * eps relative rounding
per output entry (each step is M complex multiply-adds of numbers bounded by 1, and unitaries neither grow nor shrink the
error already made), so for L = 1000, M = 9 the Frobenius difference of two correct evaluations (this kernel and the
numpy loop, each within that bound) is at most 2 * 1000 * 9 * 1.1e-16 * sqrt(M) ~ 6e-12 < 1e-11.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def sq(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from c3_amd import sequences

    return sequences


DEV = "cuda:0"
# Fitted decay rates are compared to 1e-6, not to rounding: curve_fit stops at a relative step / cost tolerance of 1e-8, so
# two fits of survival data that agree to 1e-15 can end ~1e-8 apart (seen: 1.8e-8 between |x0| and the square root of |x0|^2).
# The survival data themselves are compared to 1e-12.


def haar(rng, M, n):
    Z = rng.normal(size=(n, M, M)) + 1j * rng.normal(size=(n, M, M))
    Q, R = np.linalg.qr(Z)
    return Q * (np.diagonal(R, axis1=1, axis2=2) / np.abs(np.diagonal(R, axis1=1, axis2=2)))[:, None, :]


def loop_products(G, seqs, lengths):
    """numpy reference: U[p, s] = G[p, i_{L-1}] ... G[p, i_0]"""
    P, M = G.shape[0], G.shape[-1]
    out = np.empty((P, len(lengths), M, M), dtype=np.complex128)
    for p in range(P):
        for s, L in enumerate(lengths):
            U = np.eye(M, dtype=np.complex128)
            for t in range(L):
                U = G[p, seqs[s, t]] @ U
            out[p, s] = U
    return out


def ragged(rng, S, Lmax, n):
    lengths = rng.integers(0, Lmax + 1, size=S).astype(np.int32)
    lengths[:3] = [0, 1, Lmax]
    seqs = rng.integers(0, n, size=(S, Lmax)).astype(np.int32)
    return seqs, lengths


@pytest.mark.parametrize("M", [2, 3, 4, 9, 16, 81])
@pytest.mark.parametrize("shared", [False, True])
def test_three_modes_match_loop(sq, lib, M, shared):
    rng = np.random.default_rng(M + 100 * shared)
    n, P = 5, 3
    S, Lmax = (40, 30) if M <= 16 else (6, 12)
    G = haar(rng, M, n if shared else P * n).reshape((1 if shared else P), n, M, M)
    seqs, lengths = ragged(rng, S, Lmax, n)
    ref = loop_products(np.broadcast_to(G, (P, n, M, M)), seqs, lengths)
    psi = rng.normal(size=M) + 1j * rng.normal(size=M)
    Gt = torch.as_tensor(G[0] if shared else G, device=DEV)
    kw = dict(P=P) if shared else {}
    U = sq.seq_chain(Gt, seqs, lengths, "product", **kw).cpu().numpy()
    assert sq._lib.last_kernel() == "seq"
    assert np.abs(U - ref).max() < 1e-12
    x = sq.seq_chain(Gt, seqs, lengths, "state", torch.as_tensor(psi, device=DEV), **kw).cpu().numpy()
    assert np.abs(x - ref @ psi).max() < 1e-12
    pop = sq.seq_chain(Gt, seqs, lengths, "population", **kw).cpu().numpy()
    assert pop.shape == (P, S)
    assert np.abs(pop - np.abs(ref[..., 0, 0]) ** 2).max() < 1e-12
    assert np.all(pop[:, 0] == 1.0)  # length 0 = identity


@pytest.mark.parametrize("M", [4, 9])
def test_thousand_gate_chains_within_bound(sq, lib, M):
    rng = np.random.default_rng(7)
    P, n, S = 2, 4, 8
    G = haar(rng, M, P * n).reshape(P, n, M, M)
    lengths = np.full(S, 1000, dtype=np.int32)
    seqs = rng.integers(0, n, size=(S, 1000)).astype(np.int32)
    ref = loop_products(G, seqs, lengths)
    U = sq.seq_chain(torch.as_tensor(G, device=DEV), seqs, lengths, "product").cpu().numpy()
    err = np.linalg.norm(U - ref, axis=(-2, -1)).max()
    assert err <= 1e-11, err


def test_product_mode_matches_evaluate_sequences_batch(sq, lib):
    from c3_amd.model_learning import evaluate_sequences_batch

    rng = np.random.default_rng(2)
    P, M = 4, 3
    names = ["rx90p[0]", "rx90m[0]", "ry90p[0]", "ry90m[0]"]
    Us = {k: torch.as_tensor(haar(rng, M, P), device=DEV) for k in names}
    seqs = [[names[i] for i in rng.integers(0, 4, size=L)] for L in [0, 1, 2, 7, 7, 30, 3]]
    a = sq.evaluate_sequences_indexed(Us, seqs, "product").cpu().numpy()
    b = evaluate_sequences_batch(Us, seqs).cpu().numpy()
    assert a.shape == b.shape == (P, len(seqs), M, M)
    assert np.abs(a - b).max() < 1e-12


def test_host_device_and_torch_inputs_agree(sq, lib):
    rng = np.random.default_rng(5)
    P, n, M = 2, 3, 3
    G = haar(rng, M, P * n).reshape(P, n, M, M)
    seqs, lengths = ragged(rng, 20, 15, n)
    ref = loop_products(G, seqs, lengths)
    host = sq.seq_chain(G, seqs, lengths, "product")  # numpy: C3P_HOST_PTRS
    assert isinstance(host, np.ndarray)
    cpu_t = sq.seq_chain(torch.as_tensor(G), torch.as_tensor(seqs), torch.as_tensor(lengths), "product")  # CPU tensors: host path
    dev = sq.seq_chain(torch.as_tensor(G, device=DEV), torch.as_tensor(seqs, device=DEV), torch.as_tensor(lengths, device=DEV), "product")
    assert dev.is_cuda
    for out in (host, np.asarray(cpu_t), dev.cpu().numpy()):
        assert np.abs(out - ref).max() < 1e-12


def test_bad_index_or_length_is_an_error_and_the_next_call_works(sq, lib):
    rng = np.random.default_rng(9)
    G = haar(rng, 3, 4).reshape(1, 4, 3, 3)
    seqs, lengths = ragged(rng, 10, 8, 4)
    bad = seqs.copy()
    bad[4, 0] = 4  # = n_gates
    lengths4 = lengths.copy()
    lengths4[4] = max(lengths4[4], 1)
    neg = lengths.copy()
    neg[2] = -1
    Gd = torch.as_tensor(G, device=DEV)
    for g in (G, Gd):
        for s_, l_ in ((bad, lengths4), (seqs, neg)):
            if torch.is_tensor(g):
                s_, l_ = torch.as_tensor(s_, device=DEV), torch.as_tensor(l_, device=DEV)
            with pytest.raises(sq._lib.C3PropError, match="C3:Error"):
                sq.seq_chain(g, s_, l_, "population")
            ok = sq.seq_chain(g, seqs, lengths, "population")
            ok = ok.cpu().numpy() if torch.is_tensor(ok) else ok
            assert np.abs(ok - np.abs(loop_products(G, seqs, lengths)[..., 0, 0]) ** 2).max() < 1e-12


def ideal_gates(P=1, D=2, err=None):
    """{rx90p[0]: [P,D,D], ...} embedded in D levels (extra levels untouched); err(g) -> [P,2,2] optional left factor"""
    gens = __import__("c3_amd.sequences", fromlist=["x"])._ideal_generators()
    out = {}
    for g, U in gens.items():
        E = np.broadcast_to(np.eye(2), (P, 2, 2)) if err is None else err(g)
        V = np.zeros((P, D, D), dtype=np.complex128)
        V[:, :2, :2] = E @ U
        if D > 2:
            V[:, 2:, 2:] = np.eye(D - 2)
        out[f"{g}[0]"] = V
    return out


def test_ideal_cliffords_survive_and_have_zero_epc(sq, lib):
    for D in (2, 3):
        gates = {k: torch.as_tensor(v, device=DEV) for k, v in ideal_gates(2, D).items()}
        surv = sq.rb_survival(gates, [1, 5, 50, 300], 10, rng=0)
        assert surv.shape == (2, 4, 10)
        assert np.abs(surv - 1).max() < 1e-12
        epc = sq.epc_analytical(gates, [0], [D], True)
        assert epc.shape == (2,) and np.abs(epc).max() < 1e-12
        assert abs(sq.orbit_infid({k: v[0] for k, v in gates.items()}, RB_number=8, RB_length=40, rng=1)) < 1e-12


def over_rotation(eps):
    X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
    return lambda g: np.stack([np.cos(e) * np.eye(2) - 1j * np.sin(e) * X for e in eps])


def numpy_rb_r(sq, gates_np, p, lengths, num_seqs, seed, lindbladian=False):
    """the numpy pipeline with the same sequences: names -> loop products -> population -> the same fit"""
    rng = np.random.default_rng(seed)
    keys = [f"{g}[0]" for g in sq.GENERATORS]
    G = np.stack([gates_np[k][p] for k in keys])[None]
    surv = []
    for L in lengths:
        cl = sq._rb_cliffords(num_seqs, int(L), rng)
        seqs, ln = sq._rb_index_table(cl)
        x0 = loop_products(G, seqs, ln)[0, :, :, 0][:, 0]
        surv.append(np.abs(x0) if lindbladian else np.abs(x0) ** 2)
    return sq.rb_fit(lengths, np.array(surv))[0]


def test_rb_matches_numpy_pipeline_with_coherent_error(sq, lib):
    eps = [0.02, 0.05]
    gates_np = ideal_gates(2, 2, over_rotation(eps))
    gates = {k: torch.as_tensor(v, device=DEV) for k, v in gates_np.items()}
    kw = dict(min_length=5, max_length=200, num_lengths=8, num_seqs=20)
    epg, r = sq.RB(gates, rng=np.random.default_rng(11), return_fit=True, **kw)
    lengths = sq._rb_lengths(5, 200, 8, False)
    for p in range(2):  # the sequences are drawn once and shared by the samples: the same seed gives the same draws
        r_np = numpy_rb_r(sq, gates_np, p, lengths, 20, 11)
        assert abs(r[p] - r_np) < 1e-6, (p, r[p], r_np)  # curve_fit tolerance (see the top of this file)
    assert r[1] < r[0] < 1  # the larger over-rotation decays faster
    assert np.all(epg > 0)


def test_lindblad_variants_match_unitary_ones(sq, lib):
    eps = [0.03, 0.01]
    gates_np = ideal_gates(2, 2, over_rotation(eps))
    supers_np = {k: np.einsum("pij,pkl->pikjl", v, v.conj()).reshape(2, 4, 4) for k, v in gates_np.items()}
    gates = {k: torch.as_tensor(v, device=DEV) for k, v in gates_np.items()}
    supers = {k: torch.as_tensor(v, device=DEV) for k, v in supers_np.items()}
    seqs = sq.single_length_RB(12, 25, rng=4)
    pu = sq.evaluate_sequences_indexed(gates, seqs, "population").cpu().numpy()
    pl = sq.evaluate_sequences_indexed(supers, seqs, "population", superop=True).cpu().numpy()
    assert np.abs(pu - pl).max() < 1e-12
    kw = dict(min_length=5, max_length=150, num_lengths=6, num_seqs=10)
    ru = sq.RB(gates, rng=3, return_fit=True, **kw)[1]
    rl = sq.lindbladian_RB_left(supers, rng=3, return_fit=True, **kw)[1]
    assert np.abs(ru - rl).max() < 1e-6  # curve_fit tolerance (see the top of this file)
    eu = sq.epc_analytical(gates, [0], [2], True)
    el = sq.lindbladian_epc_analytical(supers, [0], [2], True)
    assert np.all(eu > 1e-6) and np.abs(eu - el).max() < 1e-12
    ou = sq.orbit_infid(gates, seqs=seqs)
    ol = sq.orbit_infid(supers, seqs=seqs, lindbladian=True)
    assert np.abs(ou - ol).max() < 1e-12


def test_orbit_infid_against_loop_and_seeded_shots(sq, lib):
    gates_np = ideal_gates(3, 2, over_rotation([0.0, 0.02, 0.04]))
    seqs = sq.single_length_RB(15, 20, rng=8)
    keys = [f"{g}[0]" for g in sq.GENERATORS]
    G = np.stack([gates_np[k] for k in keys], axis=1)
    idx, ln = sq.index_table(seqs, {k: i for i, k in enumerate(keys)})
    ref = 1 - (np.abs(loop_products(G, idx, ln)[..., 0, 0]) ** 2).mean(axis=1)
    got = sq.orbit_infid({k: torch.as_tensor(v, device=DEV) for k, v in gates_np.items()}, seqs=seqs)
    assert np.abs(got - ref).max() < 1e-12 and abs(got[0]) < 1e-12
    a = sq.orbit_infid(gates_np, seqs=seqs, shots=1000, rng=5)
    b = sq.orbit_infid(gates_np, seqs=seqs, shots=1000, rng=5)
    assert np.array_equal(a, b) and np.abs(a - ref).max() < 0.05


@pytest.mark.parametrize("M,n", [(3, 500), (9, 60), (16, 20), (40, 4)])
def test_tables_too_large_for_lds_read_from_global_memory(sq, lib, M, n):
    """n M^2 16 B above the 64 KB LDS budget (M <= 9), or the padded table beside the vectors (M >= 10): the global / L2
    variants of both kernels (seq_lane_kernel<M, false>, seq_wave_kernel<false>), against the loop"""
    from c3_amd import _lib

    rng = np.random.default_rng(M * 1000 + n)
    P, S, Lmax = 2, 24, 40
    G = haar(rng, M, P * n).reshape(P, n, M, M)
    seqs, lengths = ragged(rng, S, Lmax, n)
    ref = loop_products(G, seqs, lengths)
    Gt = torch.as_tensor(G, device=DEV)
    U = sq.seq_chain(Gt, seqs, lengths, "product").cpu().numpy()
    assert "false>" in _lib.last_kernel_detail(), _lib.last_kernel_detail()
    assert np.abs(U - ref).max() < 1e-12
    pop = sq.seq_chain(Gt, seqs, lengths, "population").cpu().numpy()
    assert np.abs(pop - np.abs(ref[..., 0, 0]) ** 2).max() < 1e-12


def test_epc_with_clifford_keys_in_any_numbering(sq, lib):
    """cliffords=True: the C_k are paired with their ideal elements by process fidelity, so a permuted numbering (such as
    the reference's) gives the same EPC as the generator route"""
    gates_np = ideal_gates(2, 3, over_rotation([0.02, 0.05]))
    gates = {k: torch.as_tensor(v, device=DEV) for k, v in gates_np.items()}
    U, ideal = sq.clifford_products(gates)
    Un = U.cpu().numpy()
    want = sq.epc_analytical(gates, [0], [3], True)
    perm = np.random.default_rng(3).permutation(24)
    keyed = {f"C{k + 1}": torch.as_tensor(Un[:, perm[k]], device=DEV) for k in range(24)}
    got = sq.epc_analytical(keyed, [0], [3], True, cliffords=True)
    assert np.all(want > 1e-5) and np.abs(got - want).max() < 1e-13
    S = np.einsum("pkij,pkab->pkiajb", Un, Un.conj()).reshape(2, 24, 9, 9)
    skeyed = {f"C{k + 1}": torch.as_tensor(S[:, perm[k]], device=DEV) for k in range(24)}
    got_l = sq.lindbladian_epc_analytical(skeyed, [0], [3], True, cliffords=True)
    assert np.abs(got_l - want).max() < 1e-12


def test_rb_refits_a_failed_sample_with_longer_sequences(sq, lib, monkeypatch):
    """the reference's retry (fidelities.py:561-584): a sample whose fit fails gets num_lengths longer lengths
    (max_length + min_length .. 2 max_length) and is refitted on all of them; the other samples are untouched"""
    gates = {k: torch.as_tensor(v, device=DEV) for k, v in ideal_gates(2, 2, over_rotation([0.03, 0.04])).items()}
    calls = []
    real_fit = sq.rb_fit

    def flaky(lengths, surv):
        calls.append(np.array(lengths))
        if len(calls) == 2:  # sample 1, first attempt
            raise RuntimeError("Optimal parameters not found")
        return real_fit(lengths, surv)

    monkeypatch.setattr(sq, "rb_fit", flaky)
    kw = dict(min_length=5, max_length=100, num_lengths=6, num_seqs=10)
    epg, r = sq.RB(gates, rng=2, return_fit=True, **kw)
    assert len(calls) == 3
    base = sq._rb_lengths(5, 100, 6, False)
    assert np.array_equal(calls[0], base) and np.array_equal(calls[1], base)
    assert np.array_equal(calls[2], np.append(base, sq._rb_lengths(105, 200, 6, False)))
    assert np.all((r > 0) & (r < 1)) and np.all(epg > 0)
    monkeypatch.setattr(sq, "rb_fit", lambda lengths, surv: (_ for _ in ()).throw(RuntimeError("never fits")))
    with pytest.raises(sq._lib.C3PropError, match="failed after 2 extensions"):
        sq.RB(gates, rng=2, max_retries=2, **kw)
