"""c3p_seq_chain and c3p_seq_chain_vjp at the kernel variants and plan branches the other sequence tests do not reach:
every lane instantiation (M = 1, 5, 6, 7, 8), the 64 KiB LDS budgets at exactly the budget and one gate over, the
lane / workgroup switch of the VJP, rows per lane around M = 64, the grid-stride walk of the VJP (nblk smaller than the
number of chains) and the P = 65535 limit.  Each case asserts the kernel that ran (and, for the VJP, the reported
checkpoint interval and workgroup count) and compares against the numpy loops of tests/test_gpu_sequences.py and
tests/test_seq_vjp_host.py, or a vectorised form of the reverse loop below.

Tolerances: forward as tests/test_gpu_sequences.py (1e-12 absolute for products of unitaries of L <= 40 steps).  VJP:
the near-unitary tables of tests/test_gpu_seq_vjp.py keep every chain O(1), so each chain is compared on its own with
the relative bound 1e-14 L M of test_checkpoint_segment_edges (times P where a shared table sums P copies); sums over
many chains use the absolute bound of tests/test_gpu_seq_vjp.py, 1e-13 L M (number of terms) max|out_bar|.
"""
import re

import numpy as np
import pytest

from tests.test_gpu_seq_vjp import cot, unit_table
from tests.test_gpu_sequences import haar, loop_products, ragged
from tests.test_seq_vjp_host import vjp_loop

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"


@pytest.fixture(scope="module")
def sq(lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from c3_amd import sequences

    return sequences


def detail():
    from c3_amd import _lib

    return _lib.last_kernel_detail()


def plan():
    """(C, nblk) the last c3p_seq_chain_vjp call reported"""
    m = re.search(r"checkpoint interval C=(\d+) nblk=(\d+)", detail())
    assert m, detail()
    return int(m.group(1)), int(m.group(2))


def forward_case(sq, M, n, shared, kernel, P=2, S=12, Lmax=30, modes=("product", "state", "population"), seed=0):
    rng = np.random.default_rng(seed + 1000 * M + n)
    G = haar(rng, M, n if shared else P * n).reshape((1 if shared else P), n, M, M)
    seqs, lengths = ragged(rng, S, Lmax, n)
    ref = loop_products(np.broadcast_to(G, (P, n, M, M)), seqs, lengths)
    psi = rng.normal(size=M) + 1j * rng.normal(size=M)
    Gt = torch.as_tensor(G[0] if shared else G, device=DEV)
    kw = dict(P=P) if shared else {}
    for mode in modes:
        out = sq.seq_chain(Gt, seqs, lengths, mode, torch.as_tensor(psi, device=DEV) if mode == "state" else None, **kw).cpu().numpy()
        assert kernel in detail(), (kernel, detail())
        want = {"product": ref, "state": ref @ psi, "population": np.abs(ref[..., 0, 0]) ** 2}[mode]
        assert np.abs(out - want).max() < 1e-12, mode


def vjp_case(sq, M, n, shared, kernel, P=2, S=5, Lmax=17, modes=("product", "state", "population"), seed=0, per_chain=True):
    """all chains in one call (kernel, plan and sum checked), then every chain alone against the reverse loop"""
    rng = np.random.default_rng(seed + 7 * M + n)
    G = unit_table(rng, 1 if shared else P, n, M)
    seqs, lengths = ragged(rng, S, Lmax, n)
    lengths[1] = max(lengths[1], 2)
    psi = rng.normal(size=M) + 1j * rng.normal(size=M)
    psi /= np.linalg.norm(psi)
    Gfull = np.broadcast_to(G, (P,) + G.shape[1:])
    Gin = torch.as_tensor(G[0] if shared else G, device=DEV)
    kw = dict(P=P) if shared else {}
    C_want = int(np.ceil(np.sqrt(Lmax)))
    for mode in modes:
        p0 = psi if mode == "state" else None
        pt = torch.as_tensor(psi, device=DEV) if mode == "state" else None
        W = cot(rng, mode, P, S, M)
        if mode == "population":  # away from 0, so that every chain's reference is O(1)
            W = np.sign(W) * (0.5 + np.abs(W))
        got, out = sq.seq_chain_vjp(Gin, seqs, lengths, mode, torch.as_tensor(W, device=DEV), pt, want_out=True, **kw)
        assert kernel in detail(), (kernel, detail())
        C, nblk = plan()
        assert C == C_want and nblk >= 1
        want = vjp_loop(Gfull, seqs, lengths, mode, W, p0)
        if shared:
            want = want.sum(axis=0)
        ref = np.max(np.abs(want))
        terms = S * P * (M if mode == "product" else 1)
        assert ref > 0.05 and np.max(np.abs(got.cpu().numpy() - want)) <= 1e-13 * Lmax * M * terms * np.abs(W).max(), mode
        fwd = sq.seq_chain(Gin, seqs, lengths, mode, pt, **kw).cpu().numpy()
        assert np.abs(out.cpu().numpy() - fwd).max() <= 1e-13 * max(1.0, np.abs(fwd).max())
        if not per_chain:
            continue
        for s, L in enumerate(lengths):
            if L == 0:
                continue
            Ws = W[:, s : s + 1]
            got = sq.seq_chain_vjp(Gin, seqs[s : s + 1], lengths[s : s + 1], mode, torch.as_tensor(Ws, device=DEV), pt, **kw).cpu().numpy()
            want = vjp_loop(Gfull, seqs[s : s + 1], lengths[s : s + 1], mode, Ws, p0)
            if shared:
                want = want.sum(axis=0)
            ref = np.max(np.abs(want))
            assert ref > 1e-3, (s, L, mode, ref)
            assert np.max(np.abs(got - want)) <= 1e-14 * L * M * P * ref, (s, L, mode)


# ---------------------------------------------------------------------------------------------------------------------------
# lane instantiations M = 1, 5, 6, 7, 8
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 6, 7, 8])
@pytest.mark.parametrize("shared", [False, True])
def test_forward_lane_instantiations(sq, M, shared):
    forward_case(sq, M, 5, shared, f"seq_lane_kernel<{M}, true>")


@pytest.mark.parametrize("M,n", [(1, 3), (5, 2), (6, 1), (7, 1), (8, 1)])
@pytest.mark.parametrize("shared", [False, True])
def test_vjp_lane_instantiations(sq, M, n, shared):
    """n M^2 <= 64; M = 8 with one gate needs 66,560 B of LDS (the table and 64 partial copies), above the 64 KiB default"""
    vjp_case(sq, M, n, shared, f"seq_vjp_lane_kernel<{M}>")


# ---------------------------------------------------------------------------------------------------------------------------
# LDS budgets: exactly at the budget, then one gate more
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(
    "M,n,kernel",
    [
        (8, 64, "seq_lane_kernel<8, true>"),  # 64 * 64 * 16 B = 65,536 B
        (8, 65, "seq_lane_kernel<8, false>"),
        (2, 1024, "seq_lane_kernel<2, true>"),  # 1024 * 4 * 16 B = 65,536 B
        (2, 1025, "seq_lane_kernel<2, false>"),
        (10, 37, "seq_wave_kernel<true>"),  # 32 M + 16 n M (M + 1) = 65,440 B
        (10, 38, "seq_wave_kernel<false>"),  # 67,200 B
        (16, 14, "seq_wave_kernel<true>"),  # 61,440 B
        (16, 15, "seq_wave_kernel<false>"),  # 65,792 B
    ],
)
def test_forward_lds_budget_edges(sq, M, n, kernel):
    forward_case(sq, M, n, False, kernel, S=10, Lmax=25, modes=("product", "population"))


@pytest.mark.parametrize(
    "M,n,kernel",
    [
        (1, 64, "seq_vjp_lane_kernel<1>"),  # n M^2 = 64: one lane per chain
        (1, 65, "seq_vjp_wave_kernel<true, true>"),
        (2, 16, "seq_vjp_lane_kernel<2>"),
        (2, 17, "seq_vjp_wave_kernel<true, true>"),
        (4, 4, "seq_vjp_lane_kernel<4>"),
        (4, 5, "seq_vjp_wave_kernel<true, true>"),
        # c3p_seq_vjp_plan, wave kernel: PART_LDS when 4 M 16 + n M^2 16 <= 65,536 B, TAB_LDS when n M (M + 1) 16 more fits
        (1, 1364, "seq_vjp_wave_kernel<true, true>"),  # 64 + 21,824 + 43,648 = 65,536 B exactly
        (1, 1365, "seq_vjp_wave_kernel<false, true>"),
        (4, 255, "seq_vjp_wave_kernel<false, true>"),  # 256 + 65,280 = 65,536 B exactly
        (4, 256, "seq_vjp_wave_kernel<false, false>"),
        (10, 19, "seq_vjp_wave_kernel<true, true>"),  # 640 + 30,400 + 33,440 = 64,480 B
        (10, 20, "seq_vjp_wave_kernel<false, true>"),
        (10, 40, "seq_vjp_wave_kernel<false, true>"),  # 640 + 64,000 = 64,640 B
        (10, 41, "seq_vjp_wave_kernel<false, false>"),
    ],
)
def test_vjp_budget_edges(sq, M, n, kernel):
    vjp_case(sq, M, n, False, kernel, S=5, Lmax=17, modes=("state", "population"))


# ---------------------------------------------------------------------------------------------------------------------------
# rows per lane: from M = 65 on, lanes of the workgroup kernels own rows r and r + 64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [10, 63, 64, 65, 80])
def test_forward_rows_per_lane(sq, M):
    forward_case(sq, M, 2, False, "seq_wave_kernel<", S=5, Lmax=12)


@pytest.mark.parametrize("M", [10, 63, 64, 65, 80])
def test_vjp_rows_per_lane(sq, M):
    vjp_case(sq, M, 2, False, "seq_vjp_wave_kernel<", S=4, Lmax=10)


# ---------------------------------------------------------------------------------------------------------------------------
# the grid-stride walk: fewer workgroups (or lanes) than chains
# ---------------------------------------------------------------------------------------------------------------------------
def pop_vjp_vec(G, seqs, lengths, W):
    """the reverse loop of tests/test_seq_vjp_host.py in population mode, vectorised over (sample, chain):
    G [P,n,M,M], W [P,S] -> (Gbar [P,n,M,M], pop [P,S])"""
    P, n, M = G.shape[0], G.shape[1], G.shape[-1]
    S, Lmax = seqs.shape
    pi = np.arange(P)[:, None]
    X = np.zeros((Lmax + 1, P, S, M), dtype=np.complex128)
    X[0, :, :, 0] = 1
    for t in range(Lmax):
        act = (t < lengths)[None, :, None]
        X[t + 1] = np.where(act, np.einsum("psij,psj->psi", G[pi, seqs[None, :, t]], X[t]), X[t])
    x0 = X[-1, :, :, 0]  # inactive steps carry the state: X[Lmax] = x_L for every chain
    B = np.zeros((P, S, M), dtype=np.complex128)
    B[..., 0] = 2.0 * W * x0
    Gbar = np.zeros_like(G)
    for t in range(Lmax - 1, -1, -1):
        act = t < lengths
        idx = np.broadcast_to(seqs[None, :, t], (P, S))
        Gt = G[pi, idx]
        contrib = B[..., :, None] * X[t].conj()[..., None, :] * act[None, :, None, None]
        np.add.at(Gbar, (np.broadcast_to(pi, (P, S)), idx), contrib)
        B = np.where(act[None, :, None], np.einsum("psij,psi->psj", Gt.conj(), B), B)
    return Gbar, np.abs(x0) ** 2


def test_pop_vjp_vec_is_the_reverse_loop():
    rng = np.random.default_rng(0)
    G = unit_table(rng, 3, 4, 3)
    seqs, lengths = ragged(rng, 7, 9, 4)
    W = rng.normal(size=(3, 7))
    got, pop = pop_vjp_vec(G, seqs, lengths, W)
    assert np.abs(got - vjp_loop(G, seqs, lengths, "population", W)).max() < 1e-13
    assert np.abs(pop - np.abs(loop_products(G, seqs, lengths)[..., 0, 0]) ** 2).max() < 1e-13


@pytest.mark.parametrize(
    "M,n,P,S,Lmax,shared,kernel,nblk",
    [
        (10, 2, 64, 300, 20, True, "seq_vjp_wave_kernel<true, true>", 128),  # nblk = 8192 / P
        (10, 2, 64, 300, 20, False, "seq_vjp_wave_kernel<true, true>", 128),
        (81, 4, 64, 12, 6, True, "seq_vjp_wave_kernel<false, false>", 9),  # slab: 256 MB / (64 * 4 * 81^2 * 16 B)
        (2, 4, 4096, 200, 400, True, "seq_vjp_lane_kernel<2>", 1),  # checkpoints: 4096 * 64 lanes * 40 * 2 * 16 B > 256 MB
    ],
)
def test_vjp_walks_several_chains_per_workgroup(sq, M, n, P, S, Lmax, shared, kernel, nblk):
    """the reported nblk is below the number of chains (workgroups, or 64 lanes each, walk several); for a shared table
    the fixed-order reduction sums over samples and workgroups.  The forward output of the same pass is checked for
    every chain and sample (a chain the walk skipped would leave it unwritten); the plan depends on the shapes only, so
    cotangents that are zero but for one (sample, chain) isolate that chain's gradient within the same walk, and the
    first chain, the first chain a worker reaches on its second round and the last chain are each checked on their own"""
    rng = np.random.default_rng(M * 100 + P + shared)
    G = unit_table(rng, 1 if shared else P, n, M)
    seqs, lengths = ragged(rng, S, Lmax, n)
    lengths[-1] = max(lengths[-1], 1)
    lengths[min(S - 2, 64 if "lane" in kernel else nblk)] = Lmax // 2  # the chains checked alone below are not empty
    W = rng.normal(size=(P, S))
    Gt = torch.as_tensor(G[0] if shared else G, device=DEV)
    kw = dict(P=P) if shared else {}
    got, out = sq.seq_chain_vjp(Gt, seqs, lengths, "population", torch.as_tensor(W, device=DEV), want_out=True, **kw)
    assert kernel in detail(), detail()
    C, nb = plan()
    workers = nb * 64 if "lane" in kernel else nb
    assert nb == nblk and C == int(np.ceil(np.sqrt(Lmax))) and workers < S
    if shared:  # every sample runs the same chains: the population cotangent is linear in W, so sum W over the samples
        want, pop = pop_vjp_vec(G, seqs, lengths, W.sum(axis=0)[None])
        want, pop = want[0], np.broadcast_to(pop, (P, S))
    else:
        want, pop = pop_vjp_vec(G, seqs, lengths, W)
    out = out.cpu().numpy()
    assert np.all(np.abs(out - pop) <= 1e-14 * Lmax * M * np.maximum(pop, 1e-2)), np.abs(out - pop).max()
    assert np.max(np.abs(got.cpu().numpy() - want)) <= 1e-13 * Lmax * M * P * S * np.abs(W).max()
    for p, s in ((0, 2), (P - 1, workers), (P // 2, S - 1)):  # ragged(): chain 2 has length Lmax
        Wp = np.zeros((P, S))
        Wp[p, s] = 1.0
        g1 = sq.seq_chain_vjp(Gt, seqs, lengths, "population", torch.as_tensor(Wp, device=DEV), **kw)
        assert plan() == (C, nb)
        L = max(int(lengths[s]), 1)
        one, _ = pop_vjp_vec(G[:1] if shared else G[p : p + 1], seqs[s : s + 1], lengths[s : s + 1], np.ones((1, 1)))
        g1_all = g1.cpu().numpy()
        g1 = g1_all if shared else g1_all[p]
        ref = np.abs(one[0]).max()
        assert ref > 1e-6 and np.abs(g1 - one[0]).max() <= 1e-14 * L * M * ref, (p, s, L)
        if not shared:  # and nothing lands on the other samples
            assert not np.any(np.delete(g1_all, p, axis=0))


# ---------------------------------------------------------------------------------------------------------------------------
# P = 65535, the grid.y limit
# ---------------------------------------------------------------------------------------------------------------------------
def test_largest_sample_count_and_the_refusal_above_it(sq):
    from c3_amd._lib import C3PropError

    rng = np.random.default_rng(3)
    M, n, S, Lmax = 2, 3, 3, 5
    G = unit_table(rng, 1, n, M)
    seqs, lengths = ragged(rng, S, Lmax, n)
    Gt = torch.as_tensor(G[0], device=DEV)
    P = 65535
    pop = sq.seq_chain(Gt, seqs, lengths, "population", P=P).cpu().numpy()
    want = np.abs(loop_products(G, seqs, lengths)[0, :, 0, 0]) ** 2
    assert pop.shape == (P, S) and np.abs(pop - want).max() < 1e-13
    W = rng.normal(size=(P, S))
    got, out = sq.seq_chain_vjp(Gt, seqs, lengths, "population", torch.as_tensor(W, device=DEV), want_out=True, P=P)
    assert "seq_vjp_lane_kernel<2>" in detail()
    assert np.abs(out.cpu().numpy() - want).max() < 1e-13
    gw, _ = pop_vjp_vec(G, seqs, lengths, W.sum(axis=0)[None])
    assert np.abs(got.cpu().numpy() - gw[0]).max() <= 1e-14 * Lmax * M * P * S * np.abs(gw).max()
    with pytest.raises(C3PropError, match="C3:Error.*65535"):
        sq.seq_chain(Gt, seqs, lengths, "population", P=P + 1)
    with pytest.raises(C3PropError, match="C3:Error.*65535"):
        sq.seq_chain_vjp(Gt, seqs, lengths, "population", torch.zeros((P + 1, S), dtype=torch.float64, device=DEV), P=P + 1)
    small = sq.seq_chain(Gt, seqs, lengths, "population", P=2).cpu().numpy()
    assert np.abs(small - want).max() < 1e-13
    g2 = sq.seq_chain_vjp(Gt, seqs, lengths, "population", torch.as_tensor(W[:2], device=DEV), P=2).cpu().numpy()
    assert np.abs(g2 - pop_vjp_vec(G, seqs, lengths, W[:2].sum(axis=0)[None])[0][0]).max() < 1e-12
