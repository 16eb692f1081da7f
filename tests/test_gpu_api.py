"""GPU tests of the drop-in surface: providers, tf_utils counterparts, golden fixtures,
edge cases.  Everything goes through the C ABI (libc3prop.so).  -m gpu."""
import numpy as np
import pytest

from oracle import c3_oracle as o
from c3_amd import workloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


class Instr:
    def __init__(self, name, t_start=0.0, t_end=0.0):
        self.name, self.t_start, self.t_end = name, t_start, t_end

    def get_key(self):
        return self.name


def two_transmon_setup(N=60, lind=False):
    m = workloads.ChipModel((3, 3), (5e9, 5.6e9), (-210e6, -240e6), {(0, 1): 20e6}, {"d1": 0, "d2": 1},
                            t1=(27e-6, 23e-6), t2star=(39e-6, 31e-6))
    ts = (np.arange(N) + 0.5) * 1e-11  # centred grid (devices.py:107-121)
    T = N * 1e-11
    env = np.exp(-((ts - T / 2) ** 2) / (2 * (T / 4) ** 2))
    sig = {"g": {"d1": {"values": 2 * np.pi * 4e8 * env * np.cos(2 * np.pi * 5.05e9 * ts), "ts": ts},
                 "d2": {"values": 2 * np.pi * 3e8 * env * np.cos(2 * np.pi * 5.65e9 * ts + 1.0), "ts": ts}}}
    m.set_lindbladian(lind)
    return m, workloads.SignalSource(sig), Instr("g", 0.0, T)


@pytest.mark.parametrize("lind", [False, True])
def test_pwc_provider_matches_oracle_pwc(prop, lind):
    m, gen, instr = two_transmon_setup(N=40 if lind else 120, lind=lind)
    stack = o.compute_folding_stack(len(gen.generate_signals(instr)["d1"]["ts"]))
    got = prop.unitary_provider["pwc"](m, gen, instr, stack, None)
    ref = o.pwc(m, gen, instr, stack, None)
    assert np.linalg.norm(got["U"] - ref["U"]) < 1e-10
    assert np.abs(got["dUs"] - ref["dUs"]).max() < 1e-12
    assert np.array_equal(got["ts"], ref["ts"])


def test_pwc_branch_b_and_excitation_cut(prop):
    m, gen, instr = two_transmon_setup(N=50)
    m.controllability = False  # use_control_fields = False (experiment.py:470)
    m.set_max_excitations(2)
    got = prop.pwc(m, gen, instr, [], 10)
    ref = o.pwc(m, gen, instr, None, 10)
    assert got["U"].shape == (9, 9) and got["dUs"].shape == (50, 9, 9)
    assert np.linalg.norm(got["U"] - ref["U"]) < 1e-10
    assert np.abs(got["dUs"] - ref["dUs"]).max() < 1e-12


@pytest.mark.parametrize("q", ["q1", "q2"])
def test_golden_transmon_expanded_on_device(prop, golden_dir, q):
    """reference test/test_transmon_expanded.py:252-280 through the HIP path (D=24 cut to 14)."""
    t = np.load(golden_dir + "/transmon_expanded.npz")
    cut = o.excitation_cutter((6, 4), 4)
    Hc = np.stack([o.cut_excitations(h, cut) for h in t["hamiltonians_" + q]])
    ts = t["ts_" + q][1:]
    r = prop.propagate_batch(Hc, None, None, ts[1] - ts[0], want_dUs=True)
    U = o.blowup_excitations(np.asarray(r["U"][0]), cut)
    dUs = np.stack([o.blowup_excitations(d, cut) for d in np.asarray(r["dUs"][0])])
    assert np.abs(dUs - t["partial_propagators_" + q]).max() < 1e-12
    assert np.linalg.norm(U - t["propagators_" + q]) < 1e-11


def test_golden_lindblad_two_qubit_on_device(prop, golden_dir):
    g = np.load(golden_dir + "/two_qubit.npz")
    m = workloads.ChipModel((2, 2), (5e9, 5.6e9), (0, 0), {(0, 1): 20e6}, {"d1": 0, "d2": 1}, t1=(20e-6, 20e-6), t2star=(40e-6, 40e-6))
    sig = np.stack([g["sig_d1"], g["sig_d2"]])
    hks = np.stack([g["hk_d1"], g["hk_d2"]])
    r = prop.propagate_batch(g["hdrift"], hks, sig[None], g["ts"][1] - g["ts"][0], col_ops=np.asarray(m.col_ops), lindbladian=True)
    assert np.linalg.norm(np.asarray(r["U"][0]) - g["lindblad_propagator"]) < 1e-11


def test_golden_tf_utils_on_device(prop, golden_dir):
    g = np.load(golden_dir + "/tf_utils.npz")
    for i in range(2):
        np.testing.assert_allclose(prop.tf_kron(g[f"tf_kron_{i}_inA"], g[f"tf_kron_{i}_inB"]), g[f"tf_kron_{i}_desired"], rtol=1e-7)
        np.testing.assert_allclose(prop.tf_spre(g[f"tf_spre_{i}_in"]), g[f"tf_spre_{i}_desired"], rtol=1e-7)
        np.testing.assert_allclose(prop.tf_spost(g[f"tf_spost_{i}_in"]), g[f"tf_spost_{i}_desired"], rtol=1e-7)
        np.testing.assert_allclose(prop.tf_super(g[f"tf_super_{i}_in"]), g[f"tf_super_{i}_desired"], rtol=1e-7)
        np.testing.assert_allclose(prop.Id_like(g[f"Id_like_{i}_in"]), g[f"Id_like_{i}_desired"], rtol=1e-7)


@pytest.mark.parametrize("D", [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 24, 27, 40])
@pytest.mark.parametrize("force_generic", [False, True])
def test_every_dimension_and_kernel(prop, D, force_generic):
    """Each small-D instantiation (2..10), the generic LDS kernel and their hand-over."""
    from c3_amd import _lib

    rng = np.random.default_rng(D)
    B, K, N = 3, 2, 37
    h0 = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    h0 = (h0 + h0.conj().T) * 2e10
    hks = rng.normal(size=(K, D, D)) + 1j * rng.normal(size=(K, D, D))
    hks = hks + np.conj(np.swapaxes(hks, -1, -2))
    sig = rng.normal(size=(B, K, N)) * 1e9
    dt = 1e-11 / max(1.0, D / 8)
    r = prop.propagate_batch(h0, hks, sig, dt, force_generic=force_generic)
    ref = o.propagate_batch(h0, hks, sig, dt)
    assert max(np.linalg.norm(np.asarray(r["U"][b]) - ref[b]) for b in range(B)) < 1e-10
    expect = ("generic_lds" if D <= 37 else "generic_global") if force_generic else ("smalld" if D <= 12 else "mfma")
    assert _lib.last_kernel() == expect


@pytest.mark.parametrize("D", [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 20, 23, 24, 27, 28, 31, 32, 36, 37, 40])
@pytest.mark.parametrize("strength", [1.0, 6.0])
def test_real_hamiltonian_fast_path(prop, D, strength):
    """Real symmetric h0 / hk take the cos / sin path of the small-D (D <= 12) and mid-D (13..40) kernels (every
    template instance, with and without squarings, partial propagators, per-sample operators); one complex hk
    sends the same call back to the complex path -- both must agree with the oracle."""
    rng = np.random.default_rng(100 + D)
    B, K, N = 4, 2, 29

    def sym(n=None):
        a = rng.normal(size=(D, D) if n is None else (n, D, D))
        return a + np.swapaxes(a, -1, -2)

    h0 = sym(B) * 2e10 * strength
    hks = sym(K) + 0j
    sig = rng.normal(size=(B, K, N)) * 1e9
    dt = 1e-11 / max(1.0, D / 8)
    ph = rng.uniform(0, 6, size=(B, D))
    r = prop.propagate_batch(h0, hks, sig, dt, want_dUs=True, fr_phase=ph)
    # The oracle restates TF's expm including its floor(log2) squaring count, which applies Pade-13 up to
    # ||A||_1 = 2 theta_13 = 10.7 and is itself only ~1e-9 accurate there.  In the strong-drive case the
    # per-slice truth is therefore scipy's expm (ceil rule), and the oracle is only required to be close.
    import scipy.linalg as sla

    for b in range(B):
        Xs = -1j * dt * (h0[b][None] + np.einsum("kn,kij->nij", sig[b], hks))
        if strength == 1.0:
            dref = o.tf_propagation_vectorized(h0[b], hks, sig[b], dt)
        else:
            dref = np.stack([sla.expm(x) for x in Xs])
            assert np.abs(o.tf_propagation_vectorized(h0[b], hks, sig[b], dt) - dref).max() < 1e-8
        ref = np.exp(1j * ph[b])[:, None] * o.tf_matmul_left(dref)
        assert np.linalg.norm(np.asarray(r["U"][b]) - ref) < 1e-10
        assert np.abs(np.asarray(r["dUs"][b]) - dref).max() < 1e-12
    # real but NOT symmetric (non-Hermitian) drift: the symmetric shortcut of the fast path must not be taken
    hn = h0[0].copy()
    hn[0, D - 1] += 3e9
    r3 = prop.propagate_batch(hn, hks, sig, dt)
    for b in range(B):
        Xs = -1j * dt * (hn[None] + np.einsum("kn,kij->nij", sig[b], hks))
        ref3 = o.tf_matmul_left(np.stack([sla.expm(x) for x in Xs]))
        assert np.linalg.norm(np.asarray(r3["U"][b]) - ref3) < 1e-10 * max(1.0, np.linalg.norm(ref3))
    hkc = hks.copy()
    hkc[1, 0, 1] += 0.3j
    hkc[1, 1, 0] -= 0.3j
    r2 = prop.propagate_batch(h0[0], hkc, sig, dt)
    for b in range(B):
        Xs = -1j * dt * (h0[0][None] + np.einsum("kn,kij->nij", sig[b], hkc))
        ref2 = o.tf_matmul_left(np.stack([sla.expm(x) for x in Xs]))
        assert np.linalg.norm(np.asarray(r2["U"][b]) - ref2) < 1e-10


@pytest.mark.parametrize("D", [2, 3, 5, 8, 9, 12, 13, 14, 24, 27, 36, 40, 45])
def test_supplied_generators_every_kernel(prop, D):
    """Branch B of pwc (per-slice Hamiltonians, propagation.py:295-308) and c3p_expm on the MFMA kernels
    (small-D <= 12, mid-D 13..40, the tiled path beyond; the generic kernel under FORCE_GENERIC): general complex,
    non-Hermitian generators, shared and per-sample stacks, partial propagators, frame phases."""
    import scipy.linalg as sla
    from c3_amd import _lib

    rng = np.random.default_rng(300 + D)
    B, N = 3, 21
    dt = 1e-11
    H = (rng.normal(size=(B, N, D, D)) + 1j * rng.normal(size=(B, N, D, D))) * (0.9e11 / D)
    H = H + np.conj(np.swapaxes(H, -1, -2))
    ph = rng.uniform(0, 6, size=(B, D))
    want_d = np.stack([[sla.expm(-1j * dt * H[b, n]) for n in range(N)] for b in range(B)])
    want_U = np.stack([np.exp(1j * ph[b])[:, None] * o.tf_matmul_left(want_d[b]) for b in range(B)])
    for gen in (False, True):
        r = prop.propagate_batch(H, None, None, dt, want_dUs=True, fr_phase=ph, force_generic=gen)
        kern = _lib.last_kernel()
        # (D > 40 with per-slice Hamiltonians: the tiled large-matrix path, also reported as "mfma")
        assert kern == (("generic_lds" if D <= 37 else "generic_global") if gen else ("smalld" if D <= 12 else "mfma"))
        assert np.abs(np.asarray(r["dUs"]) - want_d).max() < 1e-12
        assert max(np.linalg.norm(np.asarray(r["U"][b]) - want_U[b]) for b in range(B)) < 1e-10
    r1 = prop.propagate_batch(H[1], None, None, dt)  # one shared stack [N,D,D]
    assert np.linalg.norm(np.asarray(r1["U"][0]) - o.tf_matmul_left(want_d[1])) < 1e-10
    # c3p_expm: arbitrary (non-normal) matrices, norms needing squarings
    A = rng.normal(size=(7, D, D)) + 1j * rng.normal(size=(7, D, D))
    A *= (np.array([0.01, 0.3, 1.0, 2.5, 6.0, 0.0, 1e-9]) / np.maximum(np.abs(A).sum(axis=-2).max(axis=-1), 1e-300))[:, None, None]
    want = np.stack([sla.expm(x) for x in A])
    for gen in (False, True):
        got = np.asarray(prop.expm(A, force_generic=gen))
        assert np.abs(got - want).max() < 1e-12 * np.exp(6.0)


@pytest.mark.parametrize("D,K", [(9, 2), (14, 2), (27, 3), (27, 4), (36, 1)])
def test_mixed_real_and_complex_samples_in_one_launch(prop, D, K):
    """per-sample operators: real symmetric, complex Hermitian and real non-symmetric drifts in ONE batch -- every
    wave (small-D) / workgroup (mid-D: the real and the complex kernel instance share the launch; K = 4 control
    lines exceed the real kernel's register-resident tables and stay on the complex one) picks its path from its
    own sample's flag"""
    import scipy.linalg as sla

    rng = np.random.default_rng(77 + D + K)
    B, N = 6, 41
    a = rng.normal(size=(B, D, D))
    h0 = (a + np.swapaxes(a, -1, -2)).astype(np.complex128) * 2e10
    im = rng.normal(size=(D, D))
    h0[1] += 1j * (im - im.T) * 1e10          # complex Hermitian
    h0[3] += 1j * (im - im.T) * 3e9
    h0[4, 0, D - 1] += 4e9                      # real, not symmetric
    hk = rng.normal(size=(K, D, D))
    hks = (hk + np.swapaxes(hk, -1, -2)).astype(np.complex128)
    sig = rng.normal(size=(B, K, N)) * 1e9
    dt = 1e-11 / max(1.0, D / 8)
    r = prop.propagate_batch(h0, hks, sig, dt, want_dUs=True)
    for b in range(B):
        Xs = -1j * dt * (h0[b][None] + np.einsum("kn,kij->nij", sig[b], hks))
        d = np.stack([sla.expm(x) for x in Xs])
        assert np.abs(np.asarray(r["dUs"][b]) - d).max() < 1e-12
        ref = o.tf_matmul_left(d)
        assert np.linalg.norm(np.asarray(r["U"][b]) - ref) < 1e-10 * max(1.0, np.linalg.norm(ref))


@pytest.mark.parametrize("D", [3, 5, 9, 12, 14, 19, 27, 36, 40])
@pytest.mark.parametrize("nrm", [0.5, 0.80, 0.83, 1.0, 1.12, 1.2, 1.7, 2.4])
def test_real_path_polynomial_variants(prop, D, nrm):
    """the real path (economised cos / sin pairs: degree 6 below a scaled norm of 0.83 on the core + border loop, degree 8 up to
    1.85 everywhere, squarings beyond) at norms on either side of these and of the former Taylor thresholds, against scipy's expm"""
    import scipy.linalg as sla

    rng = np.random.default_rng(1000 + D)
    a = rng.normal(size=(D, D))
    h = a + a.T
    hs = h - np.trace(h) / D * np.eye(D)
    h = h / np.abs(hs).sum(axis=0).max()  # shifted 1-norm = 1
    dt = 1e-11
    h0 = (h * nrm / dt).astype(np.complex128)
    hk = np.zeros((1, D, D), dtype=np.complex128)
    N = 7
    r = prop.propagate_batch(h0, hk, np.zeros((2, 1, N)), dt, want_dUs=True)
    E = sla.expm(-1j * dt * h0)
    assert np.abs(np.asarray(r["dUs"][1, 3]) - E).max() < 5e-15 * max(1.0, nrm)
    assert np.linalg.norm(np.asarray(r["U"][0]) - np.linalg.matrix_power(E, N)) < 1e-12


@pytest.mark.parametrize("D", [41, 48, 49, 64, 77, 92])
def test_big_dimension_classes(prop, D):
    """Every geometry class of the big-D MFMA kernel (41..92), a couple of samples and slices."""
    from c3_amd import _lib

    rng = np.random.default_rng(D)
    B, K, N = 2, 2, 9
    h0 = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    h0 = (h0 + h0.conj().T) * (2e11 / D)
    hks = rng.normal(size=(K, D, D)) + 1j * rng.normal(size=(K, D, D))
    hks = hks + np.conj(np.swapaxes(hks, -1, -2))
    sig = rng.normal(size=(B, K, N)) * 1e9 / D
    r = prop.propagate_batch(h0, hks, sig, 1e-11, want_dUs=True)
    ref = o.propagate_batch(h0, hks, sig, 1e-11)
    assert _lib.last_kernel() == "mfma"
    assert max(np.linalg.norm(np.asarray(r["U"][b]) - ref[b]) for b in range(B)) < 1e-10
    dref = o.tf_propagation_vectorized(h0, hks, sig[1], 1e-11)
    assert np.abs(np.asarray(r["dUs"][1]) - dref).max() < 1e-12


def test_edge_cases(prop):
    wl = workloads.make_workload(2, B=1, N=1)
    r = prop.propagate_batch(wl.h0, wl.hks, wl.signals, wl.dt, want_dUs=True)
    ref = o.propagate_batch(wl.h0, wl.hks, wl.signals, wl.dt)
    assert np.abs(np.asarray(r["U"]) - ref).max() < 1e-13
    assert np.abs(np.asarray(r["dUs"][0, 0]) - ref[0]).max() < 1e-13
    # empty batch: nothing to do, no error
    e = prop.propagate_batch(wl.h0, wl.hks, np.zeros((0, 2, 5)), wl.dt)
    assert tuple(e["U"].shape) == (0, 9, 9)
    # zero Hamiltonian -> identity; huge norm -> squarings
    z = prop.propagate_batch(np.zeros((9, 9)), np.zeros((2, 9, 9)), np.zeros((2, 2, 7)), 1.0)
    assert np.abs(np.asarray(z["U"]) - np.eye(9)).max() == 0.0
    big = prop.propagate_batch(wl.h0 * 40, wl.hks, np.zeros((1, 2, 3)), wl.dt)
    bref = o.propagate_batch(wl.h0 * 40, wl.hks, np.zeros((1, 2, 3)), wl.dt)
    assert np.linalg.norm(np.asarray(big["U"][0]) - bref[0]) < 1e-10
    # ragged segmentation: N prime, B not a multiple of 4
    wl2 = workloads.make_workload(2, B=7, N=211)
    r2 = prop.propagate_batch(wl2.h0, wl2.hks, wl2.signals, wl2.dt, fr_phase=wl2.fr_phase)
    ref2 = o.propagate_batch(wl2.h0, wl2.hks, wl2.signals, wl2.dt, fr_phase=wl2.fr_phase)
    assert max(np.linalg.norm(np.asarray(r2["U"][b]) - ref2[b]) for b in range(7)) < 1e-10


def test_errors_carry_reference_prefix(prop):
    from c3_amd._lib import C3PropError

    wl = workloads.make_workload(1, B=2, N=4)
    with pytest.raises(C3PropError, match="C3:Error"):
        prop.propagate_batch(wl.h0, wl.hks, wl.signals[:, :, :0], wl.dt)  # empty time grid
    with pytest.raises(C3PropError, match="C3:Error"):
        prop.propagate_batch(wl.h0, wl.hks[:0], wl.signals, wl.dt)  # channel mismatch
    with pytest.raises(C3PropError, match="C3:Error"):
        prop.propagate_batch(wl.h0, wl.hks, wl.signals, wl.dt, lindbladian=True)  # no col_ops


def test_per_sample_operators(prop):
    """ModelLearning-style batches: every sample has its own drift/control Hamiltonians."""
    wl = workloads.make_workload(2, B=6, N=45)
    rng = np.random.default_rng(3)
    h0b = np.stack([wl.h0 * (1 + 1e-3 * rng.normal()) for _ in range(6)])
    hkb = np.stack([wl.hks * (1 + 1e-2 * rng.normal()) for _ in range(6)])
    r = prop.propagate_batch(h0b, hkb, wl.signals, wl.dt)
    for b in range(6):
        ref = o.pwc_arrays(h0b[b], hkb[b], wl.signals[b], wl.dt)["U"]
        assert np.linalg.norm(np.asarray(r["U"][b]) - ref) < 1e-10


@pytest.mark.parametrize("D,N", [(3, 1), (9, 2), (9, 700), (14, 33), (27, 12)])
def test_matmul_chain_orders(prop, D, N):
    rng = np.random.default_rng(N)
    M = (rng.normal(size=(2, N, D, D)) + 1j * rng.normal(size=(2, N, D, D))) / np.sqrt(D)
    left = np.asarray(prop.tf_matmul_left(M))
    right = np.asarray(prop.tf_matmul_right(M))
    tree = np.asarray(prop.tf_matmul_n(M[0], o.compute_folding_stack(N)))
    for b in range(2):
        lref, rref = o.tf_matmul_left(M[b]), o.tf_matmul_right(M[b])
        assert np.abs(left[b] - lref).max() < 1e-11 * max(1, np.abs(lref).max())
        assert np.abs(right[b] - rref).max() < 1e-11 * max(1, np.abs(rref).max())
    assert np.abs(tree - o.tf_matmul_n(M[0])).max() < 1e-11 * max(1, np.abs(tree).max())


def test_expm_and_series(prop):
    rng = np.random.default_rng(1)
    for D, nrm in [(3, 0.01), (8, 1.0), (9, 6.0), (20, 2.5)]:
        A = rng.normal(size=(5, D, D)) + 1j * rng.normal(size=(5, D, D))
        A *= (nrm / np.abs(A).sum(axis=-2).max(axis=-1))[:, None, None]
        assert np.abs(np.asarray(prop.expm(A)) - o.expm(A)).max() < 1e-12 * np.exp(nrm)
    # reference test/test_exp.py:9-16: series expm against the closed form
    theta = 0.7
    P = np.kron(np.array([[0, 1], [1, 0]]), np.array([[1, 0], [0, -1]]))
    want = np.cos(theta) * np.eye(4) + 1j * np.sin(theta) * P
    assert np.abs(prop.tf_expm(1j * theta * P, 100) - want).max() < 1e-6
    assert np.abs(prop.tf_expm_dynamic(1j * theta * P, 1e-12) - want).max() < 1e-10
    assert np.abs(np.asarray(prop.expm(1j * theta * P)) - want).max() < 1e-14


def test_rk4_unitary_provider(prop):
    m, gen, instr = two_transmon_setup(N=30)
    got = prop.rk4_unitary(m, gen, instr)
    # oracle: same arrays through the restated gen_u_rk4 / gen_dus_rk4
    d = prop.get_hs_of_t_ts(m, gen, instr, 2)
    ref = o.rk4_unitary_arrays(d["Hs"], d["dt"], 9)
    assert got["U"].shape == (9, 9) and got["dUs"].shape == ref["dUs"].shape
    assert np.abs(got["U"] - ref["U"]).max() < 1e-12
    assert np.abs(got["dUs"] - ref["dUs"]).max() < 1e-12
    assert gen.resolution == 100e9
    # branch B (per-sample Hamiltonians) and the list helpers
    m.controllability = False
    got_b = prop.rk4_unitary(m, gen, instr)
    assert np.abs(got_b["U"] - ref["U"]).max() < 1e-9
    lst = prop.gen_dus_rk4(d["Hs"], d["dt"])
    assert len(lst) == ref["dUs"].shape[0] and np.abs(lst[3] - ref["dUs"][3]).max() < 1e-12
    assert np.abs(prop.gen_u_rk4(d["Hs"], d["dt"], 9) - ref["U"]).max() < 1e-12
    psi = np.zeros(9, complex)
    psi[2] = 1
    assert np.abs(prop.rk4_step(d["Hs"][:3], psi, d["dt"]) - o.rk4_step(d["Hs"][:3], psi, d["dt"])).max() < 1e-13


def test_state_providers(prop):
    m, gen, instr = two_transmon_setup(N=40)
    psi0 = m.get_init_state()
    for solver in ("rk4", "tsit5"):
        got = prop.state_provider["ode_solver"](m, gen, instr, psi0, solver, "schrodinger")
        ref = o.ode_solver(m, gen, instr, psi0, solver, "schrodinger")
        assert np.abs(got["states"] - ref["states"]).max() < 1e-11
        fin = prop.ode_solver_final_state(m, gen, instr, psi0, solver, "schrodinger")
        assert np.abs(fin["states"] - ref["states"][-1]).max() < 1e-11
    m.set_lindbladian(True)
    rho0 = psi0 @ psi0.conj().T
    got = prop.ode_solver(m, gen, instr, rho0, "rk4", "von_neumann")  # forced to lindblad (:693-695)
    ref = o.ode_solver(m, gen, instr, rho0, "rk4", "von_neumann")
    assert np.abs(got["states"] - ref["states"]).max() < 1e-11
    assert abs(np.trace(got["states"][-1]) - 1) < 1e-6


def test_full_size_cfg2_properties(prop):
    """BASELINE cfg2 at full size (B=256, N=1000): size-independent properties + spot parity."""
    import torch

    wl = workloads.make_workload(2)
    dev = torch.device("cuda:0")
    r = prop.propagate_batch(torch.as_tensor(wl.h0, device=dev), torch.as_tensor(wl.hks, device=dev),
                             torch.as_tensor(wl.signals, device=dev), wl.dt, fr_phase=torch.as_tensor(wl.fr_phase, device=dev))
    U = r["U"].cpu().numpy()
    eye = np.eye(9)
    assert max(np.linalg.norm(U[b].conj().T @ U[b] - eye) for b in range(wl.B)) < 1e-11  # unitarity
    ref = o.propagate_batch(wl.h0, wl.hks, wl.signals[[0, 97, 255]], wl.dt, fr_phase=wl.fr_phase[[0, 97, 255]])
    assert max(np.linalg.norm(U[b] - ref[i]) for i, b in enumerate([0, 97, 255])) < 1e-10
    # splitting the time axis: U(0..N) = U(N/2..N) U(0..N/2) (segment associativity)
    a = prop.propagate_batch(wl.h0, wl.hks, wl.signals[:4, :, :500], wl.dt)["U"]
    b = prop.propagate_batch(wl.h0, wl.hks, wl.signals[:4, :, 500:], wl.dt)["U"]
    ph = np.exp(1j * wl.fr_phase[:4])
    comb = ph[:, :, None] * (np.asarray(b) @ np.asarray(a))
    assert max(np.linalg.norm(comb[i] - U[i]) for i in range(4)) < 1e-11


@pytest.mark.parametrize("cfg", [1, 3, 4, 5])
def test_full_size_other_configs_properties(prop, cfg):
    """BASELINE cfg1 / cfg3 / cfg4 / cfg5 at their FULL sizes (B x N = 1 x 200, 4096 x 2000, 512 x 1000
    Lindblad 81 x 81, 8192 x 5000): size-independent properties -- unitarity (trace preservation and
    Hermiticity preservation for the Lindblad superoperator), time-axis splitting, invariance under a
    permutation of the sample axis, bit-reproducibility -- plus spot parity against the oracle."""
    import torch

    wl = workloads.make_workload(cfg)
    dev = torch.device("cuda:0")
    lind = wl.lindblad
    D = wl.D
    Dm = D * D if lind else D
    h0, hks = torch.as_tensor(wl.h0, device=dev), torch.as_tensor(wl.hks, device=dev)
    col = torch.as_tensor(wl.col_ops, device=dev) if lind else None
    B = wl.B
    chunk = 1024  # bounds device memory for the 8192-sample configuration (signals stay on the host)
    U = np.empty((B, Dm, Dm), dtype=np.complex128)
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        r = prop.propagate_batch(h0, hks, torch.as_tensor(wl.signals[sl], device=dev), wl.dt, col_ops=col, lindbladian=lind)
        U[sl] = r["U"].cpu().numpy()
    eye = np.eye(Dm)
    pick = sorted(set([0, B // 3, B - 1]))
    if not lind:
        dev_unit = np.abs(np.einsum("bji,bjk->bik", U.conj(), U) - eye).max()
        assert dev_unit < 1e-10  # unitarity of every propagator of the batch
    else:
        vecI = np.eye(D).reshape(-1)
        assert np.abs(np.einsum("i,bij->bj", vecI, U) - vecI).max() < 1e-10  # trace preservation
        # Hermiticity preservation: S vec(rho^+) = vec((S rho)^+)  <=>  S[(ij),(kl)] = conj(S[(ji),(lk)])
        S4 = U[pick].reshape(len(pick), D, D, D, D)
        assert np.abs(S4 - np.conj(S4.transpose(0, 2, 1, 4, 3))).max() < 1e-10
    ref = o.propagate_batch(wl.h0, wl.hks, wl.signals[pick], wl.dt, col_ops=wl.col_ops, lindbladian=lind)
    assert max(np.linalg.norm(U[b] - ref[i]) for i, b in enumerate(pick)) < 1e-10
    # splitting the time axis, a permutation of the sample axis, and a bit-identical repeat (first samples)
    nb = min(B, 8)
    half = wl.N // 2
    sig = wl.signals[:nb]
    full = np.asarray(prop.propagate_batch(wl.h0, wl.hks, sig, wl.dt, col_ops=wl.col_ops, lindbladian=lind)["U"])
    a = np.asarray(prop.propagate_batch(wl.h0, wl.hks, sig[:, :, :half], wl.dt, col_ops=wl.col_ops, lindbladian=lind)["U"])
    bb = np.asarray(prop.propagate_batch(wl.h0, wl.hks, sig[:, :, half:], wl.dt, col_ops=wl.col_ops, lindbladian=lind)["U"])
    assert max(np.linalg.norm(bb[i] @ a[i] - full[i]) for i in range(nb)) < 1e-10
    assert max(np.linalg.norm(full[i] - U[i]) for i in range(nb)) < 1e-10  # independent of batch size / segmentation
    perm = np.random.default_rng(0).permutation(nb)
    again = np.asarray(prop.propagate_batch(wl.h0, wl.hks, sig[perm], wl.dt, col_ops=wl.col_ops, lindbladian=lind)["U"])
    assert np.array_equal(again, full[perm])  # same plan per sample -> bit-identical


class _PMap:
    def __init__(self, model, generator, instructions):
        self.model, self.generator, self.instructions = model, generator, instructions


def _experiment_setup(N=80, lind=False):
    from c3_amd.experiment import Experiment

    m, gen, _ = two_transmon_setup(N=N, lind=lind)
    T = N * 1e-11
    g = workloads.Gate("g", 0.0, T, ["d1", "d2"], carrier_freqs={"d1": 2 * np.pi * 5.05e9, "d2": 2 * np.pi * 5.65e9},
                       framechanges={"d1": 0.3, "d2": -0.2})
    exp = Experiment(_PMap(m, gen, {"g": g}), sim_res=100e9)
    return exp, m, gen, g


def test_experiment_compute_propagators_contract(prop):
    """experiment.py:440-534: plugin slot, per-gate loop, frame-rotation epilogue, stored partials."""
    exp, m, gen, g = _experiment_setup()
    m.set_FR(True)
    out = exp.compute_propagators()
    assert set(out) == {"g"} and exp.propagators["g"].shape == (9, 9)
    assert exp.partial_propagators["g"].shape[1:] == (9, 9)
    ref = o.pwc(m, gen, g, None, None)
    ph = m.frame_rotation_phases(g.t_end - g.t_start, g.carrier_freqs, g.framechanges)
    want = np.exp(1j * ph)[:, None] * ref["U"]
    assert np.linalg.norm(out["g"] - want) < 1e-10
    # registry names and callables both select the provider
    exp.prop_method = "pwc"
    assert np.linalg.norm(exp.compute_propagators()["g"] - want) < 1e-10
    exp.prop_method = prop.pwc
    assert np.linalg.norm(exp.compute_propagators()["g"] - want) < 1e-10
    # unknown gate -> the reference's message
    exp.set_opt_gates(["nope"])
    with pytest.raises(Exception, match="C3:Error: Gate 'nope' is not defined"):
        exp.compute_propagators()
    # dephasing without lindblad -> ValueError (experiment.py:511-512)
    exp.set_opt_gates(["g"])
    m.dephasing_strength = 0.1
    with pytest.raises(ValueError, match="Dephasing can only be added when lindblad is on"):
        exp.compute_propagators()
    m.dephasing_strength = 0.0


def test_experiment_batch_matches_serial_loop(prop):
    exp, m, gen, g = _experiment_setup(N=64)
    m.set_FR(True)
    rng = np.random.default_rng(0)
    base = np.stack([gen.generate_signals(g)[k]["values"] for k in ("d1", "d2")])
    batch = base[None] * rng.uniform(0.8, 1.2, size=(5, 2, 1))
    U = exp.compute_propagators_batch("g", batch)
    ph = np.exp(1j * m.frame_rotation_phases(g.t_end - g.t_start, g.carrier_freqs, g.framechanges))
    h0, hctrl = m.get_Hamiltonians()
    hks = np.stack([hctrl["d1"], hctrl["d2"]])
    for b in range(5):
        ref = ph[:, None] * o.pwc_arrays(h0, hks, batch[b], 1e-11)["U"]
        assert np.linalg.norm(U[b] - ref) < 1e-10


def test_experiment_lindblad_and_states(prop):
    exp, m, gen, g = _experiment_setup(N=30, lind=True)
    m.set_FR(True)
    out = exp.compute_propagators()["g"]
    ref = o.pwc(m, gen, g, None, None)["U"]
    ph = np.exp(1j * m.frame_rotation_phases(g.t_end - g.t_start, g.carrier_freqs, g.framechanges))
    want = np.kron(ph, ph.conj())[:, None] * ref
    assert out.shape == (81, 81) and np.linalg.norm(out - want) < 1e-10
    m.set_lindbladian(False)
    exp.set_opt_gates(["g", "g"])
    st = exp.compute_states(solver="rk4")
    assert st["states"].shape == (1 + 2 * 30, 9, 1) and st["ts"].shape == (1 + 2 * 30,)
    fin = exp.compute_final_state(solver="rk4")
    assert np.abs(fin["states"] - st["states"][-1]).max() < 1e-12
    rho = exp.compute_final_state(solver="rk4", step_function="von_neumann")["states"]
    assert abs(np.trace(rho) - 1) < 1e-6


def test_long_chain_precision(prop):
    """N = 5000 slices at D = 36 (cfg5 length): phase accumulation and rounding stay << 1e-10."""
    wl = workloads.make_workload(5, B=1, N=5000)
    r = prop.propagate_batch(wl.h0, wl.hks, wl.signals, wl.dt, fr_phase=wl.fr_phase)
    ref = o.propagate_batch(wl.h0, wl.hks, wl.signals, wl.dt, fr_phase=wl.fr_phase)
    assert np.linalg.norm(np.asarray(r["U"][0]) - ref[0]) < 2e-11


def test_fidelity_epilogue(prop):
    """unitary_infid / average_infid (+ _set) on device-resident propagator batches."""
    import torch
    from c3_amd import fidelities as F

    wl = workloads.make_workload(2, B=6, N=50)
    U = prop.propagate_batch(wl.h0, wl.hks, wl.signals, wl.dt, fr_phase=wl.fr_phase)["U"]
    rng = np.random.default_rng(4)
    for index in ([0, 1], [0], [1]):
        L = 2 ** len(index)
        G = np.linalg.qr(rng.normal(size=(L, L)) + 1j * rng.normal(size=(L, L)))[0]
        got_u = np.asarray(F.unitary_infid(G, U, index, [3, 3]))
        got_a = np.asarray(F.average_infid(G, U, index, [3, 3]))
        for b in range(6):
            assert abs(got_u[b] - o.unitary_infid(G, np.asarray(U[b]), index, [3, 3])) < 1e-13
            assert abs(got_a[b] - o.average_infid(G, np.asarray(U[b]), index, [3, 3])) < 1e-13
    # single matrix, device tensors, and the set variants
    G = np.eye(4, dtype=complex)
    one = F.unitary_infid(G, np.asarray(U[0]), [0, 1], [3, 3])
    assert abs(one - o.unitary_infid(G, np.asarray(U[0]), [0, 1], [3, 3])) < 1e-13
    Ud = torch.as_tensor(np.asarray(U), device="cuda:0")
    dev = F.average_infid(torch.as_tensor(G, device="cuda:0"), Ud, [0, 1], [3, 3])
    assert dev.is_cuda and abs(dev[2].item() - o.average_infid(G, np.asarray(U[2]), [0, 1], [3, 3])) < 1e-13
    props = {"a": np.asarray(U[0]), "b": np.asarray(U[1])}
    ideals = {"a": G, "b": G}
    assert abs(F.unitary_infid_set(props, ideals, [0, 1], [3, 3]) - o.unitary_infid_set(props, ideals, [0, 1], [3, 3])) < 1e-13
    assert abs(F.average_infid_set(props, ideals, [0, 1], [3, 3]) - o.average_infid_set(props, ideals, [0, 1], [3, 3])) < 1e-13
    from c3_amd._lib import C3PropError
    with pytest.raises(C3PropError, match="C3:Error"):
        F.unitary_infid(np.eye(2), U, [0, 1], [3, 3])
