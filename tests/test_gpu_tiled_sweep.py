"""The tiled path (c3_amd/csrc/c3p_tiled.hip: c3p_tiled_run, c3p_tiled_vjp_run) on the code that production batches run.

The tile rule of the backward sweep, tile32 = DPC / 64 * DPR / 32 * nb * 2 < 1024, is true for every small shape (Dm = 81 would need
86 samples, Dm = 257 twelve), and the sample chunks come from a 24 GB budget: with the shapes a test can afford, the 64 x 64 batched
kernel (tg_gemm_tasks_kernel), the first form of the sweep (tiled_no_batch: one launch per product, `Add` aliasing `C`) and the
b0 > 0 turn of both chunk loops never ran.  Here the options tiled_tile32, tiled_no_batch and tiled_chunk pin each form, and
which one ran is asserted from the launch log (_lib.last_kernel_detail()) by kernel name and launch count.

Launch counts, per chunk of samples, with N slices and s squarings (worked out from c3p_tiled_run / c3p_tiled_vjp_run):
  forward     tg_gemm_kernel        N (5 + s) + N - 1       T18 is five products, s squarings, one chain product from slice 1 on
  sweep       tg_gemm_kernel        N (5 + s) + 3 (N - 1)   forward half as above; backward slices N-1 .. 1: Ebar = Lambda B^H and
                                                            Lambda <- E^H Lambda (slice 0 has neither)
              tg_gemm_tasks[32]     N (5 + s)               one launch per dependency level (value + derivative)
  no_batch    tg_gemm_kernel        4 N (5 + s) + 3 (N - 1) every level as three launches
              tg_adjoint_kernel     1 + (N if N > 1 else 0) the tables (where the chunk builds them), one store slot per forward slice
              tg_count_kernel       2 + 2 odd + 2 pairs     odd = (N - 1) % 2 single slices, pairs = (N - 1) // 2, forward and backward
The squaring count is never predicted for an assertion: sum_of_norms() below only AIMS dt at the middle of an interval
(theta_18 2^(s-1), theta_18 2^s]; what the library chose is read back from these counts.

References: oracle/c3_oracle.py.  Bars: gradients max|g - want| < 1e-10 max|want| per sample (tests/test_gradient.py); forward U
Frobenius distance < 1e-10 per sample (tests/test_gpu_round2.py); two forms of the same sweep on the same inputs 1e-12 of the largest
entry (test_lindblad_vjp_sample_chunks).  Every comparison prints `TILEDERR <case> <form> <ratio>`; DESIGN.md 5.6 has the worst per
family of one run.  The operators are those of tests/test_gpu_smalld_grad_segments.py (unitary_case: mostly diagonal drift,
off-diagonal drives, a little identity on every operator so that the trace-shift term tau of tg_ubar_kernel is live, complex
Hermitian, dense complex Ubar); the CPU tests at the end hold the references to finite differences, to an eigen-decomposition form
and to a floor, as there.  Draws changed to meet them: none."""
import functools
import itertools
import re

import numpy as np
import pytest

from norm_bound_model import column_sums
from oracle import c3_oracle as o
from test_gpu_smalld_grad_segments import _fd_check, _floor_ok, _fro, _frozen, _hb, lindblad_case, per_slice_case, spectral_signal_gradient, unitary_case

BAR, BAR_U, BAR_FORMS = 1e-10, 1e-10, 1e-12
T18_THETA = 1.13  # c3p_common.h
FORMS = {"tile32": {"tiled_tile32": 1}, "tile64": {"tiled_tile32": 0}, "no_batch": {"tiled_no_batch": 1}}
TASKS32, TASKS64, GEMM = "tg_gemm_tasks32_kernel", "tg_gemm_tasks_kernel", "tg_gemm_kernel"


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import _lib, propagation

    _lib.require_gpu()
    return propagation


# ------------------------------------------------------------------------------------------------------------------------------
# aiming dt
# ------------------------------------------------------------------------------------------------------------------------------
def squarings(bound):
    s, p = 0, T18_THETA
    while p < bound:
        p, s = 2 * p, s + 1
    return s


def _margin(bound):
    """distance, in octaves, of a bound from the nearest theta_18 2^j"""
    x = np.log2(bound / T18_THETA)
    return float(min(x - np.floor(x), np.ceil(x) - x))


def place(unit_bounds, want):
    """dt at which the bounds dt * unit_bounds[i] call for want[i] squarings, each as far from a threshold as they can all be; at
    least a tenth of an octave (7 %), where the model below and the device differ by rounding"""
    best = None
    for dt in np.geomspace(1e-3, 1e2, 5001):
        bs = [dt * u for u in unit_bounds]
        if [squarings(b) for b in bs] == list(want):
            m = min(_margin(b) for b in bs)
            if best is None or m > best[0]:
                best = (m, float(dt))
    assert best is not None and best[0] > 0.1, (unit_bounds, want, best)
    return best[1]


def sum_of_norms(h0, hks, sig, samples):
    """at dt = 1, over the samples of one chunk: max_b ||G_0||_1 + sum_k max_{b,n} |c_k| ||G_k||_1, G = -i (h - Re tr h / D) -- the
    kind of bound the tiled host code forms per chunk.  Used to aim dt only."""
    samples = list(samples)
    n0 = max(column_sums(_hb(h0, b), hks, 1.0)[0].max() for b in samples)
    nk = column_sums(_hb(h0, samples[0]), hks, 1.0)[1:].max(axis=1)
    return float(n0 + np.abs(sig[samples]).max(axis=(0, 2)) @ nk)


def lindblad_sum_of_norms(h0, hks, col, sig, samples):
    """the same for Lindblad generators clp - i (h (x) 1 - 1 (x) h^T), the dissipator in the drift table"""
    samples = list(samples)
    D = h0.shape[-1]
    I, Im = np.eye(D), np.eye(D * D)
    sup = lambda h: -1j * (np.kron(h, I) - np.kron(I, h.T))
    n1 = lambda G: np.abs(G - 1j * np.trace(G).imag / (D * D) * Im).sum(axis=0).max()
    n0 = max(n1(sup(h0) + o.lindblad_dissipator(col[b] if col.ndim == 4 else col)) for b in samples)
    return float(n0 + np.abs(sig[samples]).max(axis=(0, 2)) @ np.array([n1(sup(h)) for h in hks]))


def _groups(nb, chunk):
    """the sample chunks of a tiled_chunk = chunk run, then the whole batch"""
    if chunk is None:
        return [range(nb)]
    return [range(b0, min(b0 + chunk, nb)) for b0 in range(0, nb, chunk)] + [range(nb)]


# ------------------------------------------------------------------------------------------------------------------------------
# inputs and references (cached: pure functions of the key, shared by the GPU tests and the CPU checks)
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ucase(D, K, nb, n, s, phase, per_sample=False, strong=(), chunk=None):
    """(h0, hks, sig, dt, Ubar, ph): the operators of unitary_case, complex Hermitian; the amplitudes of the samples `strong` times
    four; dt aimed at s squarings -- an int, or with `chunk` one count per chunk of that many samples and one for the whole batch"""
    h0, hks, sig, _, Ubar, ph = unitary_case(D, "complex", 1.0, per_sample, nb, n, K=K, phase=phase)
    if strong:
        amp = np.ones(nb)
        amp[list(strong)] = 4.0
        sig = _frozen(sig * amp[:, None, None])
    dt = place([sum_of_norms(h0, hks, sig, g) for g in _groups(nb, chunk)], (s,) if chunk is None else s)
    return h0, hks, sig, dt, Ubar, ph


def _rows(x, samples):
    return None if x is None else x[list(samples)]


@functools.lru_cache(maxsize=None)
def uwant(key, samples=None):
    """oracle gradients of the samples (all of them by default), stacked in that order"""
    h0, hks, sig, dt, Ubar, ph = ucase(*key)
    samples = range(sig.shape[0]) if samples is None else samples
    return _frozen(np.stack([o.pwc_signal_gradient(_hb(h0, b), hks, sig[b], dt, Ubar[b], None if ph is None else ph[b]) for b in samples]))


@functools.lru_cache(maxsize=None)
def fwd_want(key, samples=None):
    """oracle propagators (shared operators)"""
    h0, hks, sig, dt, _, ph = ucase(*key)
    samples = range(sig.shape[0]) if samples is None else samples
    return _frozen(o.propagate_batch(h0, hks, sig[list(samples)], dt, fr_phase=_rows(ph, samples)))


@functools.lru_cache(maxsize=None)
def lcase(D, C, nb, n, K, per_sample_col, s=None, chunk=None):
    """lindblad_case with collapse operators of scale 0.2 and frame phases; with `s`, dt aimed as in ucase (else the 0.3 of that case)"""
    h0, hks, sig, dt, col, Ubar, ph = lindblad_case(D, C, True, n, 0.2, per_sample_col, K, nb, True)
    if s is not None:
        dt = place([lindblad_sum_of_norms(h0, hks, col, sig, g) for g in _groups(nb, chunk)], (s,) if chunk is None else s)
    return h0, hks, sig, dt, col, Ubar, ph


def _cb(col, b):
    return col[b] if col.ndim == 4 else col


@functools.lru_cache(maxsize=None)
def lwant(key):
    h0, hks, sig, dt, col, Ubar, ph = lcase(*key)
    return _frozen(np.stack([o.pwc_lindblad_signal_gradient(h0, hks, _cb(col, b), sig[b], dt, Ubar[b], ph[b]) for b in range(sig.shape[0])]))


@functools.lru_cache(maxsize=None)
def lfwd_want(key):
    """row phases exp(i ph) over the Dm rows of the superoperator, as the library applies them"""
    h0, hks, sig, dt, col, _, ph = lcase(*key)
    return _frozen(np.stack([np.exp(1j * ph[b])[:, None] * o.propagate_batch(h0, hks, sig[b : b + 1], dt, col_ops=_cb(col, b), lindbladian=True)[0]
                             for b in range(sig.shape[0])]))


PER_SLICE_KEY = (70, False, 2, 4, 0.3)  # D, lossy and non-normal, B, N, the loss of test_per_slice_vjp_on_chip_sweeps


@functools.lru_cache(maxsize=None)
def xwant(key):
    Hs, dt, Ubar, ph = per_slice_case(*key)
    return _frozen(np.stack([o.pwc_per_slice_hamiltonian_cotangents(Hs[b], dt, Ubar[b], ph[b]) for b in range(Hs.shape[0])]))


# the cases: (D, K, B, N, s, fr_phase, per-sample h0, strong samples, chunk)
EDGE_D = (65, 96, 97, 129)  # (DPR, DPC) = (96, 128), (96, 128: exact rows), (128, 128), (160, 192: five 64-row tiles, ten of 32 rows)
edge_key = lambda D: (D, 2, 2, 5, 2, D != 96)
SQUARINGS = (0, 1, 2, 3, 4)
sq_key = lambda D, s: (D, 2, 2, 4, s, (s + D) % 2 == 0)
SLICES = (1, 2, 3, 4, 7)
slice_key = lambda n: (65, 2, 2, n, 2, n % 2 == 0)
KEY257 = (257, 1, 12, 3, 2, True)  # the rule's threshold: 5 x 9 x nb x 2 < 1024 up to nb = 11
KEY257_SAMPLES = (0, 5, 10, 11)
KEY_7A = (65, 2, 5, 3, (1, 3, 1, 3), True, False, (2, 3), 2)   # chunks of 2, 2, 1: the second plans two squarings more
KEY_7B = (65, 2, 5, 3, (2, 2, 2, 2), False, True, (), 2)       # per-sample h0, amplitudes alike
KEY_7C = (93, 1, 5, 3, (1, 3, 1, 3), True, False, (2, 3), 2)   # forward
CHUNK_SAMPLES = (0, 2, 4)  # one of each chunk
LKEY_5 = (10, 2, 2, 4, 2, False)
LKEY_7D = (10, 1, 3, 3, 2, True, (2, 2, 2), 2)  # B = 3: chunks of 2 and 1; the third sample's dissipator is 16 times the first's


# ------------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ------------------------------------------------------------------------------------------------------------------------------
def launches():
    """{kernel name: launches} of the last call"""
    from c3_amd import _lib

    out = {}
    for item in _lib.last_kernel_detail().split("; "):
        name = item.split(": ", 1)[1]
        m = re.fullmatch(r"(.+) x(\d+)", name)
        name, cnt = (m.group(1), int(m.group(2))) if m else (name, 1)
        out[name] = out.get(name, 0) + cnt
    return out


def assert_form(L, form):
    if form == "tile32":
        assert TASKS32 in L and TASKS64 not in L, L
    elif form == "tile64":
        assert TASKS64 in L and TASKS32 not in L, L
    else:
        assert TASKS64 not in L and TASKS32 not in L and GEMM in L, L


forward_gemms = lambda N, ss: sum(N * (5 + s) + N - 1 for s in ss)
sweep_gemms = lambda N, ss, no_batch=False: sum((4 if no_batch else 1) * N * (5 + s) + 3 * (N - 1) for s in ss)
sweep_tasks = lambda N, ss: sum(N * (5 + s) for s in ss)


def assert_sweep_counts(L, form, N, ss):
    """the squaring counts ss (one per chunk) from the sweep's own launches"""
    assert L[GEMM] == sweep_gemms(N, ss, form == "no_batch"), (form, N, ss, L)
    if form != "no_batch":
        assert L[TASKS32 if form == "tile32" else TASKS64] == sweep_tasks(N, ss), (form, N, ss, L)


def sweep_squarings(L, N):
    """one chunk: s read from the batched launches"""
    tasks = L.get(TASKS32, 0) + L.get(TASKS64, 0)
    assert tasks % N == 0 and tasks // N >= 5, L
    return tasks // N - 5


def check(got, want, bar, case, form):
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = max(np.abs(got[b] - want[b]).max() / np.abs(want[b]).max() for b in range(want.shape[0]))
    print(f"TILEDERR {case} {form} {err:.3e}")
    assert err < bar, (case, form, err)
    return got


def check_fro(got, want, bar, case, form):
    """Frobenius distance per sample (propagators)"""
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = max(_fro(got[b] - want[b]) for b in range(want.shape[0]))
    print(f"TILEDERR {case} {form} {err:.3e}")
    assert err < bar, (case, form, err)
    return got


def uvjp(prop, case, **opts):
    from c3_amd import _lib

    h0, hks, sig, dt, Ubar, ph = case
    with _lib.options(**opts):
        g = np.asarray(prop.propagate_batch_vjp(h0, hks, sig, dt, Ubar, fr_phase=ph))
        return g, launches()


def lvjp(prop, case, **opts):
    from c3_amd import _lib

    h0, hks, sig, dt, col, Ubar, ph = case
    with _lib.options(**opts):
        g = np.asarray(prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph))
        return g, launches()


def three_forms(run, want, case, N, s=None):
    """every form against the oracle and against the other two; -> the squaring count"""
    got = {}
    for form, opts in FORMS.items():
        g, L = run(**opts)
        assert_form(L, form)
        s = sweep_squarings(L, N) if s is None else s
        assert_sweep_counts(L, form, N, [s])
        got[form] = check(g, want, BAR, case, form)
    for a, b in itertools.combinations(FORMS, 2):
        check(got[a], got[b], BAR_FORMS, case, f"{a}~{b}")
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("D", EDGE_D)
def test_three_forms_at_the_padding_edges(prop, D):
    """case 1: B = 2, K = 2, N = 5, two squarings"""
    key = edge_key(D)
    three_forms(lambda **opts: uvjp(prop, ucase(*key), **opts), uwant(key), f"edge/D={D}", 5, s=2)


@pytest.mark.gpu
@pytest.mark.parametrize("s", SQUARINGS)
def test_squaring_count_and_its_parity(prop, s):
    """case 2: N = 4.  At D = 93 the forward path is tiled too: its launch count N (5 + s) + N - 1 says which s the library chose for
    this recipe, and the sweep's own counts say the same for D = 93 and for D = 65 (forward on the on-chip kernels)."""
    key = sq_key(93, s)
    h0, hks, sig, dt, Ubar, ph = ucase(*key)
    r = prop.propagate_batch(h0, hks, sig, dt, fr_phase=ph)
    assert launches()[GEMM] == forward_gemms(4, [s]), (s, launches())
    check_fro(r["U"], fwd_want(key), BAR_U, f"squarings/D=93/s={s}", "forward")
    for D in (93, 65):
        key = sq_key(D, s)
        got = {}
        for form in ("tile64", "tile32"):
            g, L = uvjp(prop, ucase(*key), **FORMS[form])
            assert_form(L, form)
            assert_sweep_counts(L, form, 4, [s])
            got[form] = check(g, uwant(key), BAR, f"squarings/D={D}/s={s}", form)
        check(got["tile32"], got["tile64"], BAR_FORMS, f"squarings/D={D}/s={s}", "tile32~tile64")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SLICES)
def test_slice_count(prop, n):
    """case 3, D = 65: N = 1 writes no store slot, N = 2 takes the single odd slice and no pair, N = 3 one pair, N = 4 the odd slice
    and a pair, N = 7 three pairs"""
    key = slice_key(n)
    got = {}
    for form in ("tile64", "tile32"):
        g, L = uvjp(prop, ucase(*key), **FORMS[form])
        assert_form(L, form)
        assert_sweep_counts(L, form, n, [2])
        assert L["tg_adjoint_kernel"] == 1 + (n if n > 1 else 0), L
        assert L["tg_count_kernel"] == 2 + 2 * ((n - 1) % 2) + 2 * ((n - 1) // 2), L
        got[form] = check(g, uwant(key), BAR, f"slices/N={n}", form)
    check(got["tile32"], got["tile64"], BAR_FORMS, f"slices/N={n}", "tile32~tile64")


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [11, 12])
def test_default_rule_on_both_sides_of_its_threshold(prop, nb):
    """case 4: D = 257 (DPR 288, DPC 320: 5 x 9 tiles), K = 1, N = 3, no option set: eleven samples on the 32 x 32 form, twelve on
    the 64 x 64 form.  Eleven = the first eleven of the twelve."""
    h0, hks, sig, dt, Ubar, ph = ucase(*KEY257)
    case = (h0, hks, sig[:nb], dt, Ubar[:nb], ph[:nb])
    mine, other = ("tile32", "tile64") if nb == 11 else ("tile64", "tile32")
    g, L = uvjp(prop, case)
    assert_form(L, mine)
    assert_sweep_counts(L, mine, 3, [2])
    rows = [KEY257_SAMPLES.index(b) for b in (0, 5, nb - 1)]
    check(g[[0, 5, nb - 1]], uwant(KEY257, KEY257_SAMPLES)[rows], BAR, f"threshold/B={nb}", f"default({mine})")
    g2, L = uvjp(prop, case, **FORMS[other])
    assert_form(L, other)
    check(g2[[0, 5, nb - 1]], uwant(KEY257, KEY257_SAMPLES)[rows], BAR, f"threshold/B={nb}", other)
    check(g, g2, BAR_FORMS, f"threshold/B={nb}", "tile32~tile64")


@pytest.mark.gpu
def test_lindblad_on_the_tiled_sweep(prop):
    """case 5: D = 10 (Dm = 100), two dense collapse operators, B = 2, N = 4, frame phases"""
    s = three_forms(lambda **opts: lvjp(prop, lcase(*LKEY_5), **opts), lwant(LKEY_5), "lindblad/D=10", 4)
    print("lindblad/D=10 squarings", s)


@pytest.mark.gpu
def test_per_slice_generators(prop):
    """case 6: branch B, D = 70, lossy non-normal slices"""
    from c3_amd import _lib

    Hs, dt, Ubar, ph = per_slice_case(*PER_SLICE_KEY)
    got = {}
    for form in ("tile64", "tile32"):
        with _lib.options(**FORMS[form]):
            z = np.asarray(prop.propagate_per_slice_vjp(Hs, dt, Ubar, fr_phase=ph))
            L = launches()
        assert_form(L, form)
        assert_sweep_counts(L, form, 4, [sweep_squarings(L, 4)])
        got[form] = check(z, xwant(PER_SLICE_KEY), BAR, "per-slice/D=70", form)
    check(got["tile32"], got["tile64"], BAR_FORMS, "per-slice/D=70", "tile32~tile64")


@pytest.mark.gpu
@pytest.mark.parametrize("sub", ["a", "b"])
def test_sample_chunks_of_the_sweep(prop, sub):
    """case 7 (a), (b): B = 5 in chunks of 2, 2, 1 (tiled_chunk = 2), D = 65, N = 3.  (a) shared operators, the second chunk at four
    times the amplitudes: it plans three squarings, the others one, the one-chunk run three for everybody -- so the two runs
    differ by more than the last bits and are held to the oracle bar; (b) per-sample h0, amplitudes alike: 1e-12."""
    key = KEY_7A if sub == "a" else KEY_7B
    ss = list(key[4])
    one, L = uvjp(prop, ucase(*key))
    assert_form(L, "tile32")
    assert_sweep_counts(L, "tile32", 3, ss[3:])
    assert L["tg_ubar_kernel"] == 1 and L["tg_meta_kernel"] == 1, L
    many, L = uvjp(prop, ucase(*key), tiled_chunk=2)
    assert_sweep_counts(L, "tile32", 3, ss[:3])
    assert L["tg_ubar_kernel"] == 3 and L["tg_meta_kernel"] == (1 if sub == "a" else 3), L  # shared tables: built by the first chunk only
    many64, L = uvjp(prop, ucase(*key), tiled_chunk=2, tiled_tile32=0)
    assert_form(L, "tile64")
    assert_sweep_counts(L, "tile64", 3, ss[:3])
    name = "chunks/" + ("shared" if sub == "a" else "per-sample")
    check(many, one, BAR if sub == "a" else BAR_FORMS, name, "chunked~one")
    check(many64, many, BAR_FORMS, name, "tile64~tile32")
    want = uwant(key, CHUNK_SAMPLES)
    check(one[list(CHUNK_SAMPLES)], want, BAR, name, "one")
    check(many[list(CHUNK_SAMPLES)], want, BAR, name, "chunked")


@pytest.mark.gpu
def test_sample_chunks_of_the_forward_pass(prop):
    """case 7 (c): D = 93, K = 1, N = 3, frame phases, want_dUs; the second chunk plans three squarings, the others one"""
    from c3_amd import _lib

    h0, hks, sig, dt, _, ph = ucase(*KEY_7C)
    ss = list(KEY_7C[4])
    one = prop.propagate_batch(h0, hks, sig, dt, fr_phase=ph, want_dUs=True)
    L = launches()
    assert L[GEMM] == forward_gemms(3, ss[3:]) and L["tg_meta_kernel"] == 1, L
    with _lib.options(tiled_chunk=2):
        many = prop.propagate_batch(h0, hks, sig, dt, fr_phase=ph, want_dUs=True)
        L = launches()
    assert L[GEMM] == forward_gemms(3, ss[:3]) and L["tg_meta_kernel"] == 1, L
    assert L["tg_out_kernel"] == 3 * (3 + 1), L  # per chunk: N slice propagators and U
    check_fro(many["U"], np.asarray(one["U"]), BAR_U, "chunks/forward", "U chunked~one")
    check_fro(np.asarray(many["dUs"]).reshape(15, 93, 93), np.asarray(one["dUs"]).reshape(15, 93, 93), BAR_U, "chunks/forward", "dUs chunked~one")
    want = fwd_want(KEY_7C, CHUNK_SAMPLES)
    dus = np.stack([o.expm(-1j * dt * (h0 + sig[b, 0, n] * hks[0])) for b in CHUNK_SAMPLES for n in range(3)])
    for r, tag in ((one, "one"), (many, "chunked")):
        check_fro(np.asarray(r["U"])[list(CHUNK_SAMPLES)], want, BAR_U, "chunks/forward", "U " + tag)
        check_fro(np.asarray(r["dUs"])[list(CHUNK_SAMPLES)].reshape(9, 93, 93), dus, BAR_U, "chunks/forward", "dUs " + tag)


@pytest.mark.gpu
def test_sample_chunks_lindblad_per_sample_collapse_operators(prop):
    """case 7 (d): D = 10, B = 3 in chunks of 2 and 1, per-sample col_ops, forward and gradient; both chunks and the whole batch plan
    the same squarings (aimed, and asserted from the counts): 1e-12 between the runs"""
    from c3_amd import _lib

    h0, hks, sig, dt, col, Ubar, ph = case = lcase(*LKEY_7D)
    s = LKEY_7D[6][0]
    fwd = lambda: np.asarray(prop.propagate_batch(h0, hks, sig, dt, col_ops=col, lindbladian=True, fr_phase=ph)["U"])
    one = fwd()
    L = launches()
    assert L[GEMM] == forward_gemms(3, [s]) and L["tg_meta_kernel"] == 1, L
    with _lib.options(tiled_chunk=2):
        many = fwd()
        L = launches()
    assert L[GEMM] == forward_gemms(3, [s, s]) and L["tg_meta_kernel"] == 2 and L["tg_out_kernel"] == 2, L
    check(many, one, BAR_FORMS, "chunks/lindblad", "U chunked~one")
    check_fro(one, lfwd_want(LKEY_7D), BAR_U, "chunks/lindblad", "U one")
    check_fro(many, lfwd_want(LKEY_7D), BAR_U, "chunks/lindblad", "U chunked")
    g1, L = lvjp(prop, case)
    assert_sweep_counts(L, "tile32", 3, [s])
    gm, L = lvjp(prop, case, tiled_chunk=2)
    assert_sweep_counts(L, "tile32", 3, [s, s])
    assert L["tg_ubar_kernel"] == 2 and L["tg_meta_kernel"] == 2, L
    check(gm, g1, BAR_FORMS, "chunks/lindblad", "chunked~one")
    check(g1, lwant(LKEY_7D), BAR, "chunks/lindblad", "one")
    check(gm, lwant(LKEY_7D), BAR, "chunks/lindblad", "chunked")


@pytest.mark.gpu
def test_workspace_residue(prop):
    """case 8: D = 129, then D = 65 and D = 97 in the workspace the larger call has written: the smaller layouts' pad rows and
    columns lie where it left matrix entries"""
    for form in ("tile32", "tile64"):
        for D in (129, 65, 97):
            key = edge_key(D)
            g, L = uvjp(prop, ucase(*key), **FORMS[form])
            assert_form(L, form)
            check(g, uwant(key), BAR, f"residue/D={D}", form)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU part: the inputs and the references
# ------------------------------------------------------------------------------------------------------------------------------
def _unitary_refs():
    """(key, samples) of every unitary reference of this module"""
    refs = [(edge_key(D), None) for D in EDGE_D] + [(sq_key(D, s), None) for D in (93, 65) for s in SQUARINGS]
    refs += [(slice_key(n), None) for n in SLICES]
    return refs + [(KEY257, KEY257_SAMPLES), (KEY_7A, CHUNK_SAMPLES), (KEY_7B, CHUNK_SAMPLES)]


def test_the_oracle_itself_is_two_orders_below_the_bar():
    """every unitary reference against spectral_signal_gradient: 1e-12 of the largest entry per sample"""
    for key, samples in _unitary_refs():
        h0, hks, sig, dt, Ubar, ph = ucase(*key)
        want = uwant(key, samples)
        for i, b in enumerate(range(sig.shape[0]) if samples is None else samples):
            g = spectral_signal_gradient(_hb(h0, b), hks, sig[b], dt, Ubar[b], None if ph is None else ph[b])
            assert np.abs(g - want[i]).max() < 1e-12 * np.abs(want[i]).max(), (key, b)


def test_reference_gradients_are_not_at_roundoff_level():
    """the FLOOR rule of tests/test_gpu_smalld_grad_segments.py on every reference of this module"""
    for key, samples in _unitary_refs():
        h0, hks, sig, dt, Ubar, ph = ucase(*key)
        bs = range(sig.shape[0]) if samples is None else samples
        assert _floor_ok(uwant(key, samples), [_fro(Ubar[b]) for b in bs], dt * max(_fro(h) for h in hks)), key
    for key in (LKEY_5, LKEY_7D):
        h0, hks, sig, dt, col, Ubar, ph = lcase(*key)
        I = np.eye(h0.shape[-1])
        gen = dt * max(_fro(np.kron(h, I) - np.kron(I, h.T)) for h in hks)
        assert _floor_ok(lwant(key), [_fro(u) for u in Ubar], gen), key
    Hs, dt, Ubar, ph = per_slice_case(*PER_SLICE_KEY)
    assert _floor_ok(xwant(PER_SLICE_KEY), [_fro(u) for u in Ubar], dt)


def test_references_match_finite_differences_of_the_oracle_propagator():
    """one sample per case family"""
    rng = np.random.default_rng(2)
    for key, samples, b in [(edge_key(65), None, 1), (KEY_7B, CHUNK_SAMPLES, 2), (KEY_7A, CHUNK_SAMPLES, 2)]:
        h0, hks, sig, dt, Ubar, ph = ucase(*key)
        loss = lambda s: np.real(np.vdot(Ubar[b], o.propagate_batch(_hb(h0, b), hks, s[None], dt, fr_phase=None if ph is None else ph[b : b + 1])[0]))
        _fd_check(uwant(key, samples)[b if samples is None else samples.index(b)], loss, sig[b], rng, 1e-5)
    for key, b in [(LKEY_5, 0), (LKEY_7D, 2)]:
        h0, hks, sig, dt, col, Ubar, ph = lcase(*key)
        loss = lambda s: np.real(np.vdot(Ubar[b], np.exp(1j * ph[b])[:, None] * o.propagate_batch(h0, hks, s[None], dt, col_ops=_cb(col, b), lindbladian=True)[0]))
        _fd_check(lwant(key)[b], loss, sig[b], rng, 1e-5)
    Hs, dt, Ubar, ph = per_slice_case(*PER_SLICE_KEY)  # (the rule of test_oracle_per_slice_cotangents_match_finite_differences)
    want = xwant(PER_SLICE_KEY)[1]

    def loss(H):
        U = np.eye(H.shape[-1], dtype=complex)
        for n in range(H.shape[0]):
            U = o.expm(-1j * dt * H[n]) @ U
        return np.real(np.vdot(Ubar[1], np.exp(1j * ph[1])[:, None] * U))

    for _ in range(2):
        dH = rng.normal(size=Hs[1].shape) + 1j * rng.normal(size=Hs[1].shape)
        fd = (loss(Hs[1] + 1e-6 * dH) - loss(Hs[1] - 1e-6 * dH)) / 2e-6
        assert abs(fd - np.real(np.sum(np.conj(want) * dH))) < 1e-8 * max(1.0, abs(fd))


def test_the_cases_are_what_the_gpu_tests_take_them_for():
    """the tile rule at the shapes of case 4, the padded sizes of case 1, and every dt aimed (place() asserts its margin)"""
    pad = lambda D: ((D + 31) // 32 * 32, (D + 63) // 64 * 64)
    assert [pad(D) for D in EDGE_D] == [(96, 128), (96, 128), (128, 128), (160, 192)] and pad(257) == (288, 320)
    tiles = (320 // 64) * (288 // 32)
    assert tiles * 11 * 2 < 1024 <= tiles * 12 * 2
    for key, _ in _unitary_refs() + [(KEY_7C, None)]:
        h0, hks, sig, dt, Ubar, ph = ucase(*key)
        assert (ph is not None) == bool(key[5]) and sig.shape == (key[2], key[1], key[3])
    assert sum(bool(key[5]) for key, _ in _unitary_refs()) * 2 >= len(_unitary_refs())  # frame phases in at least half the cases
    for key in (KEY_7A, KEY_7C):  # the strong chunk
        sig = ucase(*key)[2]
        assert np.abs(sig[2:4]).min() > np.abs(sig[[0, 1, 4]]).max()
    assert lcase(*LKEY_7D)[4].shape == (3, 1, 10, 10) and lcase(*LKEY_5)[4].shape == (2, 10, 10)
