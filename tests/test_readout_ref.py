"""Pins tests/readout_ref.py -- the numpy restatement the GPU read-out tests compare against -- without a GPU:

* its confusion matrix against an explicit loop over basis states (unequal row lengths catch a transposed Kronecker order);
* every estimator against a literal one-line transcription of c3/libraries/estimators.py;
* its long-double reverse mode against long-double central differences along random directions of x, of every confusion row and
  of scale and offset;
* g_LL_prime through it, without confusion and rescale, against model_learning.g_LL_prime / g_LL_prime_grad;
* the host layer of c3_amd/readout.py that needs no device: confusion_matrix, confusion_matrix_vjp, label_weights.
"""
import itertools

import numpy as np
import pytest

from tests import readout_ref as rr

LD = np.longdouble


@pytest.mark.parametrize("dims", [(2,), (3,), (3, 3), (3, 2)])
def test_confusion_matrix_against_basis_state_loop(dims):
    """Entry [(a_0..a_Q-1), (n_0..n_Q-1)] is prod_q (row_q[n_q] if a_q == 0 else 1 - row_q[n_q]): the probability of reading
    the bits a from the basis state n, first subsystem slowest in both indices (tf_kron order, model.py:158-159)."""
    rng = np.random.default_rng(3)
    rows = [rng.uniform(0, 1, size=d) for d in dims]
    want = np.zeros((2 ** len(dims), int(np.prod(dims))))
    for ia, a in enumerate(itertools.product(*[[0, 1]] * len(dims))):
        for i_n, n in enumerate(itertools.product(*[range(d) for d in dims])):
            want[ia, i_n] = np.prod([rows[q][n[q]] if a[q] == 0 else 1 - rows[q][n[q]] for q in range(len(dims))])
    got = rr.confusion_matrix(rows, np.float64)
    assert got.shape == want.shape
    assert np.allclose(got, want, rtol=0, atol=4 * np.finfo(float).eps)
    assert np.allclose(got.sum(0), 1.0, rtol=0, atol=8 * np.finfo(float).eps)  # every state is read as something
    from c3_amd import readout as ro

    assert np.array_equal(ro.confusion_matrix(rows), got)
    per_set = [np.stack([r, r[::-1]]) for r in rows]
    got2 = ro.confusion_matrix(per_set)
    assert got2.shape == (2,) + want.shape and np.array_equal(got2[0], got)
    assert np.array_equal(got2, rr.confusion_matrix(per_set, np.float64))
    mixed = ro.confusion_matrix([per_set[0]] + rows[1:])
    assert np.array_equal(mixed[0], got) and mixed.shape == (2,) + want.shape


TRANSCRIPTIONS = {
    # estimators.py, with tf.* read as np.* and the Normal log-density written out
    "rms_dist": lambda m, s, e, n: np.sqrt(np.mean(np.abs(m - s) ** 2)),
    "rms_sim_stds_dist": lambda m, s, e, n: np.sqrt(np.mean((np.abs(m - s) / np.sqrt(s * (1 - s) / n)) ** 2)),
    "rms_exp_stds_dist": lambda m, s, e, n: np.sqrt(np.mean((np.abs(m - s) / e) ** 2)),
    "g_LL_prime": lambda m, s, e, n: np.mean(((m - s) ** 2 / np.sqrt(s * (1 - s) / n) ** 2 - 1) / 2),
    "neg_loglkh_gauss": lambda m, s, e, n: -np.mean(-0.5 * ((m - s) / np.sqrt(s * (1 - s) / n)) ** 2 - np.log(np.sqrt(s * (1 - s) / n)) - 0.5 * np.log(2 * np.pi)),
    "neg_loglkh_gauss_norm": lambda m, s, e, n: -np.mean(-0.5 * ((m - s) / np.sqrt(s * (1 - s) / n)) ** 2),
    "neg_loglkh_gauss_norm_sum": lambda m, s, e, n: -np.sum(-0.5 * ((m - s) / np.sqrt(s * (1 - s) / n)) ** 2),
}


@pytest.mark.parametrize("name", rr.ESTIMATORS)
def test_estimator_against_transcription(name):
    rng = np.random.default_rng(5)
    s = rng.uniform(0.05, 0.95, size=(17, 3))
    m = s + rng.uniform(-0.05, 0.05, size=s.shape)
    e = rng.uniform(0.01, 0.05, size=s.shape)
    n = rng.integers(500, 2001, size=s.shape).astype(float)
    want = TRANSCRIPTIONS[name](m, s, e, n)
    got = rr.estimator(name, m, s, e, n, np.float64)
    # the same formula in the same precision; only log(std) + log(2 pi) / 2 may be associated differently
    assert got == pytest.approx(want, rel=16 * np.finfo(float).eps)
    assert set(TRANSCRIPTIONS) == set(rr.ESTIMATORS)


CASES = [(2, 0, "none", "none", "one"), (3, 1, "shared", "shared", "none"), (6, 0, "perset", "perset", "repeated"), (6, 1, "shared", "perset", "one"),
         (9, 1, "perset", "shared", "none"), (3, 0, "none", "perset", "repeated")]


@pytest.mark.parametrize("name", rr.ESTIMATORS)
@pytest.mark.parametrize("D,density,conf,rescale,labels", CASES)
def test_reverse_mode_against_long_double_differences(name, D, density, conf, rescale, labels):
    """Central differences in long double (eps = 2^-63 on x86; the formulas below use whatever np.finfo reports).  With step h the
    truncation error is h^2 |f'''| / 6 and the rounding error eps |f| / h; h = eps^(1/3) balances them at eps^(2/3) (|f''' / 6| +
    |f|).  The goal is a smooth function of O(1) inputs whose derivatives grow like powers of 1 / (s (1 - s)) <= 21 and of
    shots (m - s)^2 / (s (1 - s)) <= 2000 * 0.0025 * 21 ~ 1e2 per order: |f'''| / |f'| <~ 1e6 is generous, so the tolerance is
    1e6 eps^(2/3) relative to the largest directional derivative of the case plus the rounding term eps^(2/3) |f|.  With
    eps = 1.1e-19 that is 2.3e-7 relative -- six digits, against reverse-mode formulas that are wrong by O(1) if wrong at all."""
    eps = float(np.finfo(LD).eps)
    h = LD(eps ** (1.0 / 3.0))
    c = rr.make_case(11, D, density, 3, 7, conf, rescale, labels)
    rev = rr.run_case(c, name, LD)
    rng = np.random.default_rng(17)

    def goal(x=None, rows=None, scale=None, offset=None):
        x = c["x"].astype(np.clongdouble) if x is None else x
        rows = c["rows"] if rows is None else rows
        cm = None if rows is None else rr.confusion_matrix(rows, LD)
        f = rr.forward(x, D, cm, c["label_w"], c["scale"] if scale is None else scale, c["offset"] if offset is None else offset, c["meas"], c["stds"],
                       c["shots"], name, LD)
        return np.sum(np.asarray(c["weights"], dtype=LD) * f["goals"])

    f0 = abs(goal())
    checks = []
    # x
    E = (rng.normal(size=c["x"].shape) + 1j * rng.normal(size=c["x"].shape)).astype(np.clongdouble)
    xl = c["x"].astype(np.clongdouble)
    checks.append(("x", (goal(x=xl + h * E) - goal(x=xl - h * E)) / (2 * h), np.sum((np.conj(rev["x_bar"]) * E).real)))
    # every confusion row (per set where the rows are)
    if c["rows"] is not None:
        rows_bar = rr.confusion_rows_bar(c["rows"], rev["conf_bar"], LD)
        for q, r in enumerate(c["rows"]):
            Er = rng.normal(size=r.shape).astype(LD)
            rp = [a.astype(LD) + (h * Er if k == q else 0) for k, a in enumerate(c["rows"])]
            rm = [a.astype(LD) - (h * Er if k == q else 0) for k, a in enumerate(c["rows"])]
            an = np.sum(rows_bar[q] * Er) if r.ndim == 2 else np.sum(rows_bar[q].sum(0) * Er)
            checks.append((f"row{q}", (goal(rows=rp) - goal(rows=rm)) / (2 * h), an))
    if c["scale"] is not None:
        sc, of = np.asarray(c["scale"], dtype=LD), np.asarray(c["offset"], dtype=LD)
        Es, Eo = rng.normal(size=sc.shape).astype(LD), rng.normal(size=of.shape).astype(LD)
        bar = rev["rescale_bar"]
        an_s = np.sum(bar[:, 0] * Es) if sc.ndim else np.sum(bar[:, 0]) * Es
        an_o = np.sum(bar[:, 1] * Eo) if of.ndim else np.sum(bar[:, 1]) * Eo
        checks.append(("scale", (goal(scale=sc + h * Es) - goal(scale=sc - h * Es)) / (2 * h), an_s))
        checks.append(("offset", (goal(offset=of + h * Eo) - goal(offset=of - h * Eo)) / (2 * h), an_o))
    top = max(abs(fd) for _, fd, _ in checks)
    tol = eps ** (2.0 / 3.0) * (1e6 * float(top) + float(f0))
    for what, fd, an in checks:
        assert abs(float(fd - an)) <= tol, (what, float(fd), float(an), tol)
    assert float(top) > 1e3 * tol  # the check can fail


def test_g_ll_prime_reproduces_model_learning():
    from c3_amd import model_learning as ml

    c = rr.make_case(23, 3, 0, 2, 9, "none", "none", "one")
    weights = np.array([1.0, 0.0])
    rev = rr.reverse(c["x"], 3, None, c["label_w"], None, None, c["meas"], c["stds"], c["shots"], "g_LL_prime", weights, np.float64)
    sim = rev["sim"][0, :, 0]
    want = ml.g_LL_prime(c["meas"][0, :, 0], sim, c["stds"][0, :, 0], c["shots"][0, :, 0])
    assert rev["goals"][0] == pytest.approx(want, rel=32 * np.finfo(float).eps)  # sqrt(.)^2 against the variance itself
    dg = ml.g_LL_prime_grad(c["meas"][0, :, 0], sim, c["stds"][0, :, 0], c["shots"][0, :, 0])
    assert np.allclose(rev["sim_bar"][0, :, 0], dg, rtol=64 * np.finfo(float).eps, atol=0)
    assert np.all(rev["sim_bar"][1] == 0)


def test_split_constants_and_ids_mirror_the_headers():
    """The S boundaries of tests/test_gpu_readout.py come from c3_amd/readout.py: they must be the kernels' own numbers."""
    import os
    import re

    from c3_amd import _lib, readout as ro

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "c3_amd", "csrc", "c3p_readout.h")).read()
    assert int(re.search(r"#define C3P_READOUT_SEQ_BLOCK (\d+)", h).group(1)) == ro.SEQ_BLOCK
    assert int(re.search(r"#define C3P_READOUT_THREADS (\d+)", h).group(1)) == ro.REDUCE_THREADS
    api = open(os.path.join(root, "include", "c3prop.h")).read()
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define C3P_EST_(\w+) (\d+)", api)}
    assert ids == {k.lower(): v for k, v in ro.ESTIMATORS.items()}
    assert re.search(r"#define C3P_KERNEL_READOUT 14\b", api) and re.search(r"#define C3P_KERNEL_READOUT_VJP 15\b", api)
    assert _lib.KERNEL_NAMES[14] == "readout" and _lib.KERNEL_NAMES[15] == "readout_vjp"
    import __graft_entry__ as g

    assert "c3p_readout.hip" in g.HIP_SOURCES


def test_label_weights_and_rows_vjp_host_layer():
    from c3_amd import readout as ro
    from c3_amd._lib import C3PropError

    assert np.array_equal(ro.label_weights((3, 2), [(0, 1), (1, 1), (0, 1)], True), [0, 2, 0, 1])
    assert np.array_equal(ro.label_weights((3, 2), [(2, 1)], False), np.eye(6)[5])
    assert np.array_equal(ro.label_weights((3, 2), [(0, 1)], True), rr.label_weights((3, 2), [(0, 1)], True))
    with pytest.raises(C3PropError, match=r"C3:ERROR:State \(2, 0\) not defined. Available are:"):
        ro.label_weights((3, 2), [(2, 0)], True)
    assert set(ro.ESTIMATORS) == set(rr.ESTIMATORS)
    with pytest.raises(C3PropError, match="not served"):
        ro.estimator_id("median_dist")
    rng = np.random.default_rng(2)
    for rows in ([rng.uniform(size=(4, 3)), rng.uniform(size=(4, 2))], [rng.uniform(size=3), rng.uniform(size=(4, 3))], [rng.uniform(size=(4, 2))]):
        D = int(np.prod([r.shape[-1] for r in rows]))
        cb = rng.normal(size=(4, 2 ** len(rows), D))
        got = ro.confusion_matrix_vjp(rows, cb)
        want = rr.confusion_rows_bar(rows, cb, np.float64)
        for g, w in zip(got, want):
            assert g.shape == w.shape == (4, g.shape[1])
            assert np.allclose(g, w, rtol=0, atol=1e-14 * np.max(np.abs(cb)) * D)
