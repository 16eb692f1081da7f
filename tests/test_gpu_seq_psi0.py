"""Per-sample start vectors on the indexed sequence chains (C3P_SEQ_PSI0_PER_SAMPLE) and the cotangent of the start vector
(c3p_seq_state_vjp, psi0_bar) on the GPU.

References: numpy loops (the forward chain and the reverse sweep written here; G_bar by tests/test_seq_vjp_host.vjp_loop called per
sample).  Bars: the forward chain atol = 1e-13 L M max|psi0| (L products of rounding ~M eps each on states of norm ~|psi0|, the
derivation of tests/test_gpu_seq_vjp.py); G_bar and psi0_bar that file's close(), for psi0_bar with terms = S (a sum over the S
sequences of a sample)."""
import numpy as np
import pytest

from tests.test_gpu_seq_vjp import close, cot, ragged, unit_table
from tests.test_seq_vjp_host import vjp_loop

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
P = 2
# (M, n_gates): the sizes of test_vjp_matches_reverse_loop, and (16, 12) for the wave instance with the table outside the LDS
SIZES = [(2, 3), (3, 3), (4, 3), (9, 3), (16, 3), (16, 12), (81, 2)]


@pytest.fixture(scope="module")
def sq(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from c3_amd import sequences

    return sequences


def vjp_kernel(M, n):
    """the instance c3p_seq_vjp_plan picks (c3p_seq_vjp.hip): lane per chain, or the workgroup kernel <table in LDS, partial in LDS>"""
    nMM, cs, lds = n * M * M, 16, 64 * 1024
    if M <= 9 and nMM <= 64:
        return f"seq_vjp_lane_kernel<{M}>"
    part = 4 * M * cs + nMM * cs <= lds
    tab = part and 4 * M * cs + nMM * cs + n * M * (M + 1) * cs <= lds
    return f"seq_vjp_wave_kernel<{'true' if tab else 'false'}, {'true' if part else 'false'}>"


def fwd_kernel(M, n):
    if M <= 9:
        return f"seq_lane_kernel<{M}, "
    return "seq_wave_kernel<true>" if 2 * M * 16 + n * M * (M + 1) * 16 <= 64 * 1024 else "seq_wave_kernel<false>"


def problem(M, n, shared):
    rng = np.random.default_rng(1000 * M + 10 * n + shared)
    S, Lmax = (5, 9) if M < 81 else (3, 5)
    G = unit_table(rng, 1 if shared else P, n, M)
    seqs, lengths = ragged(rng, S, Lmax, n)  # lengths 0, 1 and Lmax among them
    psi = rng.normal(size=(P, M)) + 1j * rng.normal(size=(P, M))
    psi /= np.linalg.norm(psi, axis=1, keepdims=True)
    W = cot(rng, "state", P, S, M)
    Gfull = np.broadcast_to(G, (P,) + G.shape[1:]) if shared else G
    return G[0] if shared else G, Gfull, seqs, lengths, psi, W, S, Lmax


def chain_loop(Gfull, seqs, lengths, psi):
    """x_L = G[i_{L-1}] ... G[i_0] psi[p]; psi [P,M]"""
    out = np.zeros((Gfull.shape[0], len(lengths), Gfull.shape[-1]), dtype=np.complex128)
    for p in range(Gfull.shape[0]):
        for s, L in enumerate(lengths):
            x = psi[p].copy()
            for t in range(L):
                x = Gfull[p, seqs[s, t]] @ x
            out[p, s] = x
    return out


def psi0_bar_loop(Gfull, seqs, lengths, W):
    """psi0_bar[p] = sum_s G[p,i_0]^H ... G[p,i_{L-1}]^H W[p,s]"""
    out = np.zeros((Gfull.shape[0], Gfull.shape[-1]), dtype=np.complex128)
    for p in range(Gfull.shape[0]):
        for s, L in enumerate(lengths):
            b = np.array(W[p, s], dtype=np.complex128)
            for t in range(L - 1, -1, -1):
                b = Gfull[p, seqs[s, t]].conj().T @ b
            out[p] += b
    return out


@pytest.mark.parametrize("M,n", SIZES)
@pytest.mark.parametrize("shared", [False, True])
def test_forward_with_per_sample_psi0(sq, M, n, shared):
    from c3_amd import _lib

    G, Gfull, seqs, lengths, psi, W, S, Lmax = problem(M, n, shared)
    got = sq.seq_chain(G, seqs, lengths, "state", psi, P=P)
    assert fwd_kernel(M, n) in _lib.last_kernel_detail(), _lib.last_kernel_detail()
    want = chain_loop(Gfull, seqs, lengths, psi)
    tol = 1e-13 * Lmax * M * np.abs(psi).max()
    err = np.abs(got - want).max()
    print(f"M={M} n={n} shared={shared}: forward max err {err:.3e} (bar {tol:.3e})")
    assert err <= tol
    # the two samples start differently: a kernel that reads psi0[0] for both misses by O(1)
    assert np.abs(chain_loop(Gfull, seqs, lengths, psi[:1].repeat(P, 0)) - want).max() > 1e-3
    # device tensors: the same bits
    t = lambda a: torch.as_tensor(a, device=DEV)
    assert np.array_equal(sq.seq_chain(t(G), t(seqs), t(lengths), "state", t(psi), P=P).cpu().numpy(), got)


@pytest.mark.parametrize("M,n", SIZES)
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("psi_per_sample", [False, True])
def test_gbar_and_psi0_bar(sq, M, n, shared, psi_per_sample):
    from c3_amd import _lib

    G, Gfull, seqs, lengths, psi, W, S, Lmax = problem(M, n, shared)
    psi_arg = psi if psi_per_sample else psi[0]
    psi_full = psi if psi_per_sample else psi[:1].repeat(P, 0)
    scale = np.abs(W).max()
    want_g = np.stack([vjp_loop(Gfull[p : p + 1], seqs, lengths, "state", W[p : p + 1], psi_full[p])[0] for p in range(P)])
    if shared:
        want_g = want_g.sum(axis=0)
    want_p = psi0_bar_loop(Gfull, seqs, lengths, W)
    # G_bar alone (c3p_seq_chain_vjp, with the flag for a per-sample psi0)
    g_only = sq.seq_chain_vjp(G, seqs, lengths, "state", W, psi_arg, P=P)
    assert vjp_kernel(M, n) in _lib.last_kernel_detail(), _lib.last_kernel_detail()
    print(f"M={M} n={n} shared={shared} psi per sample={psi_per_sample}: G_bar max err {np.abs(g_only - want_g).max():.3e}")
    close(g_only, want_g, Lmax, M, S * P, scale)
    # with psi0_bar (c3p_seq_state_vjp): the same G_bar bits, the forward output, and the cotangent of the start vector per sample
    g, out, pbar = sq.seq_chain_vjp(G, seqs, lengths, "state", W, psi_arg, P=P, want_out=True, want_psi0_bar=True)
    detail = _lib.last_kernel_detail()
    assert vjp_kernel(M, n) in detail and "seq_vjp_reduce_kernel" in detail, detail
    assert np.array_equal(g, g_only)
    assert pbar.shape == (P, M)
    print(f"    psi0_bar max err {np.abs(pbar - want_p).max():.3e}, max|want| {np.abs(want_p).max():.3e}")
    close(pbar, want_p, Lmax, M, S, scale)
    assert np.abs(out - chain_loop(Gfull, seqs, lengths, psi_full)).max() <= 1e-13 * Lmax * M * np.abs(psi).max()
    # reproducible: a second call, and device tensors against host arrays, bit for bit
    g2, pbar2 = sq.seq_chain_vjp(G, seqs, lengths, "state", W, psi_arg, P=P, want_psi0_bar=True)
    assert np.array_equal(g2, g) and np.array_equal(pbar2, pbar)
    t = lambda a: torch.as_tensor(a, device=DEV)
    gd, pd = sq.seq_chain_vjp(t(G), t(seqs), t(lengths), "state", t(W), t(psi_arg), P=P, want_psi0_bar=True)
    assert np.array_equal(gd.cpu().numpy(), g) and np.array_equal(pd.cpu().numpy(), pbar)


@pytest.mark.parametrize("M", [3, 16])
@pytest.mark.parametrize("psi_per_sample", [False, True])
def test_psi0_bar_is_the_adjoint_of_the_forward_chain(sq, M, psi_per_sample):
    """The chain is linear in psi0: Re sum conj(psi0_bar) dpsi = Re sum conj(out_bar) (chain(psi0 + dpsi) - chain(psi0)) for any
    dpsi, with no step size; the right-hand side comes from the forward entry point, which shares nothing with the reverse sweep."""
    G, Gfull, seqs, lengths, psi, W, S, Lmax = problem(M, 3, False)
    rng = np.random.default_rng(M)
    dpsi = rng.normal(size=(P, M)) + 1j * rng.normal(size=(P, M))
    psi_arg = psi if psi_per_sample else psi[0]
    _, pbar = sq.seq_chain_vjp(G, seqs, lengths, "state", W, psi_arg, want_psi0_bar=True)
    base = sq.seq_chain(G, seqs, lengths, "state", psi if psi_per_sample else psi[:1].repeat(P, 0))
    moved = sq.seq_chain(G, seqs, lengths, "state", (psi if psi_per_sample else psi[:1].repeat(P, 0)) + dpsi)
    lhs = np.sum(np.conj(pbar) * dpsi, axis=1).real  # [P]
    rhs = np.sum(np.conj(W) * (moved - base), axis=(1, 2)).real
    print(f"M={M}: <psi0_bar, dpsi> = {lhs}, <out_bar, d out> = {rhs}, diff {np.abs(lhs - rhs).max():.3e}")
    close(lhs, rhs, Lmax, M, S, np.abs(W).max())


def test_shapes_flags_and_errors(sq):
    from c3_amd import _lib
    from c3_amd._lib import C3PropError

    G, Gfull, seqs, lengths, psi, W, S, Lmax = problem(4, 3, False)
    with pytest.raises(C3PropError, match="psi0 has shape"):
        sq.seq_chain(G, seqs, lengths, "state", psi[:, :3])
    with pytest.raises(C3PropError, match="psi0 has shape"):
        sq.seq_chain_vjp(G, seqs, lengths, "state", W, np.zeros((3, 4), dtype=complex))
    with pytest.raises(C3PropError, match="state mode"):
        sq.seq_chain_vjp(G, seqs, lengths, "population", np.ones((P, S)), want_psi0_bar=True)
    # the flag outside the state mode is an error of the C ABI, in both entry points
    c = lambda a: np.ascontiguousarray(a)
    Gc, sc, lc = c(G), c(seqs), c(lengths)
    out = np.empty((P, S), dtype=np.float64)
    ptr = lambda a: a.ctypes.data
    fl = _lib.HOST_PTRS | _lib.SEQ_PSI0_PER_SAMPLE
    rc = _lib.load().c3p_seq_chain(ptr(Gc), Gc[0].size, 3, 4, P, ptr(sc), S, Lmax, ptr(lc), 2, None, fl, ptr(out), None)
    assert rc != 0 and b"C3P_SEQ_PSI0_PER_SAMPLE" in _lib.load().c3p_last_error()
    gb = np.empty_like(Gc)
    rc = _lib.load().c3p_seq_chain_vjp(ptr(Gc), Gc[0].size, 3, 4, P, ptr(sc), S, Lmax, ptr(lc), 2, None, ptr(out), fl, ptr(gb), None, None)
    assert rc != 0 and b"C3P_SEQ_PSI0_PER_SAMPLE" in _lib.load().c3p_last_error()
    # no sequence at all: zero cotangents
    g, pbar = sq.seq_chain_vjp(G, seqs[:0], lengths[:0], "state", W[:, :0], psi, want_psi0_bar=True)
    assert not np.any(g) and not np.any(pbar) and pbar.shape == (P, 4)
    # the next valid call works
    _, pbar = sq.seq_chain_vjp(G, seqs, lengths, "state", W, psi, want_psi0_bar=True)
    close(pbar, psi0_bar_loop(Gfull, seqs, lengths, W), Lmax, 4, S, np.abs(W).max())
