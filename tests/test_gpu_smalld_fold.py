"""The fused tail of the small-D chain kernel (c3p_smalld.hip, smalld_chain_kernel): the fold of a wave's four segments, the
scaled partial products handed to wave 0 of the workgroup-per-sample mode as LDS images, the final fold and store --
over every number of waves per sample, both real loops, the complex loop, the tile classes and the supplied-generator mode.

Every case is checked like tests/test_gpu_round4.py::test_smalld_core_plus_border_form: |U - U_oracle|_F < 1e-10 per sample,
|U U^+ - 1| < 1e-10, the workgroup-per-sample result against the one-wave (no_mw) result to 1e-11, and two identical calls bit
for bit.  The oracle's own expm is accurate only while ||dt H||_1 < theta_13 = 5.37 (tests/test_gpu_smalld_real_loop.py), so
that condition and the oracle's unitarity are checked for every input on the CPU first."""
import functools

import numpy as np
import pytest

from oracle import c3_oracle as o

TOL = 1e-10      # against the oracle, Frobenius norm per sample, and unitarity
TOL_PATHS = 1e-11  # between two variants of one path
DT = 1e-11
KERNEL = "c3p_smalld.hip: smalld_chain_kernel<%d, false, false, %s, %s, %s>"


def rsym(rng, D, scale):
    a = rng.normal(size=(D, D))
    return (scale * (a + a.T) / 2).astype(complex)


def operators(rng, D, K, amp, B, N, h0s):
    """real symmetric operators and amplitudes as test_smalld_core_plus_border_form generates them (h0s = 6e10 there)"""
    h0 = rsym(rng, D, h0s)
    hks = np.stack([rsym(rng, D, 1.0) for _ in range(K)]) if K else np.zeros((0, D, D), complex)
    sig = rng.normal(size=(B, K, N)) * 2e9 * amp
    return h0, hks, sig


def make_case(D=9, K=2, N=131, B=2, S=32, amp=1.0, h0s=6e10, phase=True, seed=0, kind="real", opts=None, form=None):
    rng = np.random.default_rng(9000 + seed)
    h0, hks, sig = operators(rng, D, K, amp, B, N, h0s)
    dt = DT
    if kind == "trace":
        # a drift with a large trace: the sample's phase winds many times, every slice stays inside the oracle's range
        h0 = h0 + 1.2e11 * np.eye(D)
        hks = hks + 0.5 * np.eye(D)
    elif kind == "per_sample":
        # operators per sample with different traces: a phase applied to the wrong sample cannot pass
        h0 = np.stack([h0 + t * np.eye(D) for t in (0.0, 0.5e11, -0.4e11)][:B])
    elif kind == "complex":
        up = np.triu(hks[1].real, 1)
        hks[1] = hks[1] + 0.3j * (up - up.T)  # Hermitian, complex: the sample takes the complex loop
    elif kind == "mixed":
        hks = np.stack([hks] * B)
        up = np.triu(hks[1, 1].real, 1)
        hks[1, 1] = hks[1, 1] + 0.3j * (up - up.T)  # sample 1 complex, its neighbours real
    elif kind == "given":
        # supplied generators (branch B): Hermitian Hamiltonians per slice, no tables and no signals
        hs = np.stack([[rsym(rng, D, h0s) + 1j * (lambda a: 2e10 * (a - a.T))(rng.normal(size=(D, D))) for _ in range(N)] for _ in range(B)])
        h0, hks, sig = hs, None, None
    ph = rng.uniform(0, 6, size=(B, D)) if phase else None
    return dict(D=D, K=K, N=N, B=B, S=S, h0=h0, hks=hks, sig=sig, dt=dt, ph=ph, kind=kind, opts=opts or {}, form=form)


CASES = {
    # ---- waves per sample: eight, four and two; unequal chains, equal chains, one slice per chain (the fold does all the work)
    "w8_n131": dict(N=131, S=32, seed=1),
    "w8_n70": dict(N=70, S=32, seed=2),
    "w8_n32": dict(N=32, S=32, seed=3),
    "w4_n67": dict(N=67, S=16, seed=4),
    "w2_n45": dict(N=45, S=8, seed=5),
    # ---- phase handling
    "trace": dict(N=131, S=32, seed=6, kind="trace", amp=0.5, h0s=4e10),
    "per_sample_traces": dict(N=131, S=32, B=3, seed=7, kind="per_sample", h0s=4e10),
    # ---- both polynomial forms and squarings.  Rows 1, 4 and 5 of test_smalld_core_plus_border_form have the amplitudes 1, 2.6
    # and 14 on a drift of ||dt h0||_1 ~ 5: every one of them takes the degree-8 pair behind two squarings, and at 14 a slice leaves
    # the oracle's range (||dt H||_1 up to 7).  Rows 1 and 4 are kept (the default drift of this file; "amp26"); the three forms of
    # the kernel come from smaller drifts, their segment bounds asserted on the CPU.
    "amp26": dict(N=131, S=32, seed=8, amp=2.6),
    "deg6": dict(N=131, S=32, seed=30, amp=0.4, h0s=5e9, form="deg6"),
    "deg8": dict(N=131, S=32, seed=31, amp=0.7, h0s=1.5e10, form="deg8"),
    "squarings": dict(N=131, S=32, seed=32, amp=6.0, h0s=1.5e10, form="squarings"),
    # ---- compile-time and run-time table loops
    "k0": dict(N=131, S=32, K=0, seed=10),
    "k1": dict(N=131, S=32, K=1, seed=11),
    "k3": dict(N=131, S=32, K=3, seed=12),
    # ---- the complex loop through the same tail
    # (at N = 131 both splits give long segments of five slices; at N = 160 the complex sample re-splits on the device, 7 -> 6)
    "complex": dict(N=131, S=32, seed=13, kind="complex"),
    "complex_resplit": dict(N=160, S=32, seed=21, kind="complex"),
    "mixed_real_complex": dict(N=131, S=32, B=3, seed=14, kind="mixed"),
    # ---- other tile classes, eight waves per sample
    "d5": dict(D=5, N=131, S=32, seed=15),
    "d3": dict(D=3, N=131, S=32, seed=16),
    "d12": dict(D=12, N=131, S=32, seed=17, h0s=4e10),
    "d9_padded": dict(N=131, S=32, seed=18, opts=dict(no_split81=1)),
    # ---- supplied generators: one-wave workgroups, the ticket path of the fused tail
    "given": dict(D=9, K=0, N=40, S=8, seed=19, kind="given", h0s=4e10),
    # ---- one sample
    "b1": dict(N=131, S=32, B=1, seed=20),
}


# every case runs with fr_phase present and absent
CASES.update({name + "_nophase": dict(kw, phase=False) for name, kw in list(CASES.items())})


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of a case and the oracle's propagators, computed once and shared"""
    c = make_case(**CASES[name])
    B = c["B"]
    if c["kind"] == "given":
        Hs = c["h0"]
        ref = []
        for b in range(B):
            U = np.eye(c["D"], dtype=complex)
            for n in range(c["N"]):
                U = o.expm(-1j * c["dt"] * Hs[b, n]) @ U
            ref.append(np.exp(1j * c["ph"][b])[:, None] * U if c["ph"] is not None else U)
        c["H"] = Hs
    else:
        per = lambda x, b, nd: x[b] if x.ndim == nd + 1 else x
        ref = []
        H = []
        for b in range(B):
            h0, hks = per(c["h0"], b, 2), per(c["hks"], b, 3)
            ph = None if c["ph"] is None else c["ph"][b : b + 1]
            ref.append(o.propagate_batch(h0, hks, c["sig"][b : b + 1], c["dt"], fr_phase=ph)[0])
            H.append(h0[None] + np.einsum("kn,kij->nij", c["sig"][b], hks))
        c["H"] = np.stack(H)
    c["ref"] = np.stack(ref)
    return c


def segment_lengths(N, S, per_mille):
    """slices per chain as launch_chain_t / split_segments deal them"""
    if S == 32 and N >= 4 * S:
        h = S // 2
        la = max(1, (N * per_mille) // (500 * S))
        if h * la > N - h:
            la = (N - h) // h
        rest = N - h * la
        edge = lambda g: g * la if g <= h else h * la + ((g - h) * rest) // h
    else:
        edge = lambda g: (g * N) // S
    return [edge(g + 1) - edge(g) for g in range(S)]


def segment_bounds(c, per_mille=700):
    """the kernel's bound per segment: ||G0||_1 + sum_k max_t |c_k(t)| ||G_k||_1 of the trace-shifted generators"""
    D = c["D"]
    one = lambda h: np.abs(c["dt"] * (h - np.trace(h) / D * np.eye(D))).sum(axis=0).max()
    edges = np.cumsum([0] + segment_lengths(c["N"], c["S"], per_mille))
    return np.array([one(c["h0"]) + sum(np.abs(c["sig"][b, k, n0:n1]).max() * one(c["hks"][k]) for k in range(c["K"]))
                     for b in range(c["B"]) for n0, n1 in zip(edges, edges[1:])])


def test_shapes_take_the_paths_they_are_meant_for():
    lens = segment_lengths(131, 32, 700)
    waves = [lens[4 * w : 4 * w + 4] for w in range(8)]
    assert sum(lens) == 131 and max(lens) > min(lens) and any(min(w) < max(w) for w in waves)  # unequal chains, padded slots
    assert segment_lengths(160, 32, 640)[0] == 6 and segment_lengths(160, 32, 700)[0] == 7  # the complex loop's own split differs
    assert sorted(set(segment_lengths(70, 32, 700))) == [2, 3]
    assert set(segment_lengths(32, 32, 700)) == {1}
    for name, kw in CASES.items():
        c = make_case(**kw)
        assert c["B"] <= 4 and c["N"] <= 200, name


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_meets_the_bars_on_every_input(name):
    """no GPU: every slice inside the range where the oracle's expm is accurate, and the oracle's propagators unitary to the bar"""
    c = case(name)
    nrm = np.abs(c["dt"] * c["H"]).sum(axis=-2).max()
    assert nrm < o.PADE_THETA[4], nrm
    R = c["ref"]
    assert np.abs(R @ R.conj().transpose(0, 2, 1) - np.eye(c["D"])).max() < TOL / 10
    if c["form"] is not None:
        bd = segment_bounds(c)
        lo, hi = {"deg6": (0.0, 0.81), "deg8": (0.81, 1.85), "squarings": (1.85, np.inf)}[c["form"]]  # radii of c3p_common.h
        assert lo < bd.min() and bd.max() <= hi, (bd.min(), bd.max())
    if c["kind"] == "trace":
        D = c["D"]
        tr = lambda h: np.trace(h).real / D
        total = c["dt"] * (c["N"] * tr(c["h0"]) + sum(c["sig"][:, k, :].sum(axis=1) * tr(c["hks"][k]) for k in range(c["K"])))
        assert np.abs(total).min() > 10 * 2 * np.pi, total
    if c["kind"] == "per_sample":
        tr = [np.trace(h).real for h in c["h0"]]
        assert len(set(np.round(tr, 3))) == c["B"]


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_fused_tail(prop, name):
    from c3_amd import _lib

    c = case(name)
    D, B = c["D"], c["B"]

    def run(**more):
        with _lib.options(smalld_segments=c["S"], **c["opts"], **more):
            U = np.asarray(prop.propagate_batch(c["h0"], c["hks"], c["sig"], c["dt"], fr_phase=c["ph"])["U"])
        return U, _lib.last_kernel_detail()

    U, detail = run()
    U2, _ = run()
    V, detail1 = run(no_mw=1)
    given = c["kind"] == "given"
    split = "true" if D in (5, 9) and not c["opts"].get("no_split81") and not given else "false"
    xg = "true" if given else "false"
    # (the launch log may name other kernels in front of the chain kernel: the pre-pass of the supplied generators)
    assert detail.endswith(KERNEL % (D, xg, "false" if given else "true", split)), detail
    assert detail1.endswith(KERNEL % (D, xg, "false", split)), detail1
    err = [np.linalg.norm(U[b] - c["ref"][b]) for b in range(B)]
    err1 = [np.linalg.norm(V[b] - c["ref"][b]) for b in range(B)]
    uni = np.abs(U @ U.conj().transpose(0, 2, 1) - np.eye(D)).max()
    dif = np.abs(U - V).max()
    print(f"{name}: |U - U_ref|_F {max(err):.3e} (one-wave mode {max(err1):.3e}), |U U^+ - 1| {uni:.3e}, |U_mw - U_1w| {dif:.3e}")
    assert max(err) < TOL and max(err1) < TOL
    assert uni < TOL
    assert dif < TOL_PATHS
    assert np.array_equal(U, U2)
