"""Host side of the sequence-chain gradient (c3p_seq_chain_vjp): the ABI declaration, the likelihood's derivative, and
the numpy reverse-mode loop that tests/test_gpu_seq_vjp.py uses as its reference, checked here against central
differences of a numpy forward loop."""
import os

import numpy as np
import pytest

from c3_amd import _lib
from c3_amd import model_learning as ml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# numpy references (imported by tests/test_gpu_seq_vjp.py)
# ---------------------------------------------------------------------------------------------------------------------------
def _starts(mode, M, psi0):
    if mode == "state":
        return np.asarray(psi0, dtype=np.complex128).reshape(M, 1)
    if mode == "population":
        return np.eye(M, dtype=np.complex128)[:, :1]
    return np.eye(M, dtype=np.complex128)


def fwd_loop(G, seqs, lengths, mode, psi0=None, superop=False):
    """c3p_seq_chain in numpy: G [P,n,M,M] -> [P,S,M,M] / [P,S,M] / [P,S]."""
    P, M = G.shape[0], G.shape[-1]
    S = len(lengths)
    X0 = _starts(mode, M, psi0)
    out = []
    for p in range(P):
        row = []
        for s in range(S):
            X = X0.copy()
            for t in range(lengths[s]):
                X = G[p, seqs[s, t]] @ X
            if mode == "product":
                row.append(X)
            elif mode == "state":
                row.append(X[:, 0])
            else:
                q = abs(X[0, 0]) ** 2
                row.append(np.sqrt(q) if superop else q)
        out.append(row)
    return np.array(out)


def vjp_loop(G, seqs, lengths, mode, out_bar, psi0=None, superop=False):
    """The reverse-mode loop: every state of the chain stored, then Gbar[i_t] += xbar_{t+1} x_t^H and
    xbar_t = G[i_t]^H xbar_{t+1} from the end (d loss = Re sum conj(out_bar) d out).  Returns Gbar [P,n,M,M]."""
    P, n, M = G.shape[0], G.shape[1], G.shape[-1]
    X0 = _starts(mode, M, psi0)
    Gbar = np.zeros_like(G)
    for p in range(P):
        for s in range(len(lengths)):
            xs = [X0.copy()]
            for t in range(lengths[s]):
                xs.append(G[p, seqs[s, t]] @ xs[-1])
            xL = xs[-1]
            if mode == "product":
                B = np.array(out_bar[p, s], dtype=np.complex128)
            elif mode == "state":
                B = np.array(out_bar[p, s], dtype=np.complex128).reshape(M, 1)
            else:
                B = np.zeros((M, 1), dtype=np.complex128)
                x0 = xL[0, 0]
                if superop:
                    B[0, 0] = out_bar[p, s] * x0 / abs(x0) if abs(x0) > 0 else 0.0
                else:
                    B[0, 0] = 2.0 * out_bar[p, s] * x0
            for t in range(lengths[s] - 1, -1, -1):
                g = seqs[s, t]
                Gbar[p, g] += B @ xs[t].conj().T
                B = G[p, g].conj().T @ B
    return Gbar


def random_table(rng, P, n, M, scale=0.6):
    """non-unitary gate tables (neither isometries nor invertible by their adjoint)"""
    return scale * (rng.normal(size=(P, n, M, M)) + 1j * rng.normal(size=(P, n, M, M))) / np.sqrt(M)


def _scalar(out, W, mode):
    """a real scalar of the forward output: Re sum conj(W) out"""
    return float(np.sum(np.conj(W) * out).real) if mode != "population" else float(np.sum(W * out))


# ---------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_seq_chain_vjp():
    with open(os.path.join(ROOT, "include", "c3prop.h")) as f:
        h = f.read()
    assert "int c3p_seq_chain_vjp(" in h
    assert "#define C3P_KERNEL_SEQ_VJP 10" in h
    assert _lib.KERNEL_NAMES[10] == "seq_vjp"
    assert "c3p_seq_chain_vjp" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["c3p_seq_chain_vjp"][1]) == 16


def test_g_LL_prime_grad_matches_central_differences():
    rng = np.random.default_rng(1)
    S = 7
    m = rng.uniform(0.05, 0.95, S)
    s = rng.uniform(0.1, 0.9, S)
    shots = rng.integers(100, 2000, S).astype(float)
    g = ml.g_LL_prime_grad(m, s, None, shots)
    for j in range(S):
        h = 1e-6 * s[j]
        sp, sm = s.copy(), s.copy()
        sp[j] += h
        sm[j] -= h
        fd = (ml.g_LL_prime(m, sp, None, shots) - ml.g_LL_prime(m, sm, None, shots)) / (2 * h)
        assert g[j] == pytest.approx(fd, rel=1e-7)


def test_dv_g_LL_prime_is_the_reference_formula():
    rng = np.random.default_rng(2)
    gs = rng.normal(size=3)
    dv = rng.normal(size=(3, 5))
    w = [2, 5, 3]
    want = (2 * dv[0] + 5 * dv[1] + 3 * dv[2]) / 10
    assert np.allclose(ml.dv_g_LL_prime(gs, dv, w), want, rtol=1e-15, atol=0)


@pytest.mark.parametrize("mode,superop", [("product", False), ("state", False), ("population", False), ("population", True)])
def test_reverse_loop_matches_central_differences(mode, superop):
    """Re <Gbar, E> of the reverse loop against (f(G + hE) - f(G - hE)) / 2h of the forward loop, on non-unitary tables,
    f = Re sum conj(W) out.  Truncation error O(h^2 |f'''|) ~ 1e-10 relative at h = 1e-5."""
    rng = np.random.default_rng(3 + 10 * superop + len(mode))
    P, n, M, S, Lmax = 2, 3, 3, 5, 7
    G = random_table(rng, P, n, M, 0.9)
    seqs = rng.integers(0, n, size=(S, Lmax)).astype(np.int32)
    lengths = np.array([0, 1, 7, 4, 6], dtype=np.int32)
    psi0 = rng.normal(size=M) + 1j * rng.normal(size=M)
    out = fwd_loop(G, seqs, lengths, mode, psi0, superop)
    W = rng.normal(size=out.shape) + (1j * rng.normal(size=out.shape) if mode != "population" else 0)
    Gbar = vjp_loop(G, seqs, lengths, mode, W, psi0, superop)
    for _ in range(3):
        E = rng.normal(size=G.shape) + 1j * rng.normal(size=G.shape)
        h = 1e-5
        fp = _scalar(fwd_loop(G + h * E, seqs, lengths, mode, psi0, superop), W, mode)
        fm = _scalar(fwd_loop(G - h * E, seqs, lengths, mode, psi0, superop), W, mode)
        fd = (fp - fm) / (2 * h)
        an = float(np.sum(np.conj(Gbar) * E).real)
        assert an == pytest.approx(fd, rel=1e-7, abs=1e-9)
    # sequences of length 0 add nothing; gates never used get zero
    unused = sorted(set(range(n)) - set(int(seqs[s, t]) for s in range(S) for t in range(lengths[s])))
    for g in unused:
        assert not np.any(Gbar[:, g])


def test_reverse_loop_superop_zero_population_gives_zero():
    G = np.zeros((1, 1, 4, 4), dtype=np.complex128)
    G[0, 0, 1, 0] = 1.0  # moves everything out of entry 0: x_L[0] = 0
    seqs = np.zeros((1, 2), dtype=np.int32)
    Gbar = vjp_loop(G, seqs, np.array([2], dtype=np.int32), "population", np.ones((1, 1)), superop=True)
    assert np.all(np.isfinite(Gbar)) and not np.any(Gbar)
