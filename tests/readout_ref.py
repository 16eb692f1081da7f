"""numpy restatement of the read-out epilogue and of its reverse mode, in a chosen precision (np.float64 or np.longdouble).

Written from the reference's formulas, one step per function:

  populations     |x_n|^2 for kets; Re x[n (D + 1)], the diagonal of vec_to_dm(x), for density vectors (c3/experiment.py:619-622)
  confusion       ConfusionMatrix.confuse (c3/libraries/tasks.py:122-128): kron over the subsystems of [[row], [1 - row]], then
                  conf_matrix @ pops
  selection       Experiment.process (c3/experiment.py:380-402): the sum over the listed labels (a label listed twice counts
                  twice), or every value
  rescale         MeasurementRescale.rescale (tasks.py:175-178): pop * meas_scale + meas_offset
  estimators      c3/libraries/estimators.py:34-37 (rms_dist), :49-53 (rms_sim_stds_dist), :64-67 (rms_exp_stds_dist),
                  :108-119 (neg_loglkh_gauss), :123-135 (.._norm), :139-151 (.._norm_sum), :155-157 (g_LL_prime); the Normal
                  log-density is -((x - mu) / sigma)^2 / 2 - log(sigma) - log(2 pi) / 2

`forward` runs them in that order; `reverse` is the hand-derived reverse mode of the same chain for the combined goal
sum_p goal_weights[p] goals[p].  tests/test_readout_ref.py pins both without a GPU.
"""
import itertools

import numpy as np

ESTIMATORS = ("g_LL_prime", "neg_loglkh_gauss", "neg_loglkh_gauss_norm", "neg_loglkh_gauss_norm_sum", "rms_dist", "rms_exp_stds_dist",
              "rms_sim_stds_dist")


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def populations(x, D, dtype):
    """[..., D] from states [..., M], M = D (kets) or D^2 (density vectors)."""
    x = np.asarray(x)
    re, im = x.real.astype(dtype), x.imag.astype(dtype)
    if x.shape[-1] == D:
        return re * re + im * im
    assert x.shape[-1] == D * D
    return re[..., :: D + 1]


def confusion_matrix(rows, dtype):
    """tasks.py:122-127.  rows[q] [d_q] or [P,d_q] -> [2^Q,D] or [P,2^Q,D]."""
    rows = [np.asarray(r, dtype=dtype) for r in rows]
    per_set = any(r.ndim == 2 for r in rows)
    if per_set:
        P = next(r.shape[0] for r in rows if r.ndim == 2)
        return np.stack([confusion_matrix([r[p] if r.ndim == 2 else r for r in rows], dtype) for p in range(P)])
    mat = np.ones((1, 1), dtype=dtype)
    for row1 in rows:
        row2 = np.ones_like(row1) - row1
        mat = np.kron(mat, np.stack([row1, row2]))
    return mat


def label_weights(dims, labels, computational):
    """experiment.py:380-400 as a weight vector over comp_state_labels / state_labels (model.py:147-159)."""
    space = list(itertools.product(*[[0, 1] if computational else list(range(d)) for d in dims]))
    w = np.zeros(len(space))
    for label in labels:
        w[space.index(tuple(label))] += 1
    return w


def estimator(name, m, s, e, sh, dtype):
    """The goal of one set over all its values."""
    half = dtype(1) / 2
    if name == "rms_dist":
        return np.sqrt(np.mean(np.abs(m - s) ** 2))
    if name == "rms_exp_stds_dist":
        return np.sqrt(np.mean((np.abs(m - s) / e) ** 2))
    std = np.sqrt(s * (1 - s) / sh)
    if name == "rms_sim_stds_dist":
        return np.sqrt(np.mean((np.abs(m - s) / std) ** 2))
    if name == "g_LL_prime":
        return np.mean(((m - s) ** 2 / std**2 - 1) / 2)
    logp = lambda y: -half * ((y - s) / std) ** 2 - np.log(std) - half * np.log(2 * _pi(dtype))
    if name == "neg_loglkh_gauss":
        return -np.mean(logp(m))
    if name == "neg_loglkh_gauss_norm":
        return -np.mean(logp(m) - logp(s))
    if name == "neg_loglkh_gauss_norm_sum":
        return -np.sum(logp(m) - logp(s))
    raise KeyError(name)


def estimator_grad(name, m, s, e, sh, dtype):
    """d estimator / d s, element-wise.  r = m - s, var = s (1 - s) / sh, q = r^2 / var:
    dq/ds = -(2 r / var + q (1 - 2 s) / (s (1 - s))), d log(var)/ds = (1 - 2 s) / (s (1 - s)); a root of a mean g = sqrt(mean t)
    has dg = dt / (2 g n)."""
    n = dtype(s.size)
    r = m - s
    if name == "rms_dist":
        return -2 * r / (2 * estimator(name, m, s, e, sh, dtype) * n)
    if name == "rms_exp_stds_dist":
        return -2 * r / e**2 / (2 * estimator(name, m, s, e, sh, dtype) * n)
    v = s * (1 - s)
    var = v / sh
    slope = (1 - 2 * s) / v
    dq = -(2 * r / var + r * r / var * slope)
    if name == "rms_sim_stds_dist":
        return dq / (2 * estimator(name, m, s, e, sh, dtype) * n)
    if name in ("g_LL_prime", "neg_loglkh_gauss_norm"):
        return dq / 2 / n
    if name == "neg_loglkh_gauss_norm_sum":
        return dq / 2
    if name == "neg_loglkh_gauss":
        return (dq / 2 + slope / 2) / n
    raise KeyError(name)


def _per_set(a, P, ndim):
    """a shared ([...]) or per set ([P,...]) -> [P,...]."""
    a = np.asarray(a)
    return np.broadcast_to(a, (P,) + a.shape) if a.ndim == ndim else a


def forward(x, D, conf, label_w, scale, offset, meas, stds, shots, name, dtype):
    """x [P,S,M]; conf None, [R,D] or [P,R,D]; label_w None or [R]; scale / offset None, scalars or [P]; meas, stds, shots [P,S,V].
    Returns pop [P,S,D], c [P,S,R], raw [P,S,V], sim [P,S,V], goals [P]."""
    P = x.shape[0]
    pop = populations(x, D, dtype)
    if conf is None:
        c = pop
    else:
        cm = _per_set(np.asarray(conf, dtype=dtype), P, 2)
        c = np.einsum("prn,psn->psr", cm, pop)
    raw = c if label_w is None else np.einsum("r,psr->ps", np.asarray(label_w, dtype=dtype), c)[..., None]
    if scale is None and offset is None:
        sim = raw
    else:
        sc = _per_set(np.asarray(1 if scale is None else scale, dtype=dtype), P, 0)
        of = _per_set(np.asarray(0 if offset is None else offset, dtype=dtype), P, 0)
        sim = raw * sc[:, None, None] + of[:, None, None]
    m, e, sh = (np.asarray(a, dtype=dtype) for a in (meas, stds, shots))
    goals = np.array([estimator(name, m[p], sim[p], e[p], sh[p], dtype) for p in range(P)], dtype=dtype)
    return {"pop": pop, "c": c, "raw": raw, "sim": sim, "goals": goals}


def reverse(x, D, conf, label_w, scale, offset, meas, stds, shots, name, goal_weights, dtype):
    """Cotangents of sum_p goal_weights[p] goals[p]: x_bar [P,S,M] (d loss = Re sum conj(x_bar) dx), conf_bar [P,R,D],
    rescale_bar [P,2] (scale, offset), pop_bar [P,S,D], sim_bar [P,S,V]; plus everything `forward` returns."""
    P = x.shape[0]
    f = forward(x, D, conf, label_w, scale, offset, meas, stds, shots, name, dtype)
    m, e, sh = (np.asarray(a, dtype=dtype) for a in (meas, stds, shots))
    gw = np.asarray(goal_weights, dtype=dtype)
    sim_bar = np.stack([gw[p] * estimator_grad(name, m[p], f["sim"][p], e[p], sh[p], dtype) for p in range(P)])
    rescaled = not (scale is None and offset is None)
    sc = _per_set(np.asarray(1 if scale is None else scale, dtype=dtype), P, 0)
    raw_bar = sim_bar * sc[:, None, None] if rescaled else sim_bar
    rescale_bar = np.stack([np.sum(sim_bar * f["raw"], axis=(1, 2)), np.sum(sim_bar, axis=(1, 2))], -1)
    c_bar = raw_bar if label_w is None else raw_bar * np.asarray(label_w, dtype=dtype)  # [P,S,1] * [R]
    if conf is None:
        pop_bar = c_bar
        conf_bar = np.einsum("psr,psn->prn", c_bar, f["pop"])
    else:
        cm = _per_set(np.asarray(conf, dtype=dtype), P, 2)
        pop_bar = np.einsum("prn,psr->psn", cm, c_bar)
        conf_bar = np.einsum("psr,psn->prn", c_bar, f["pop"])
    x = np.asarray(x)
    cdt = np.clongdouble if dtype is np.longdouble else np.complex128
    if x.shape[-1] == D:
        x_bar = 2 * pop_bar * x.astype(cdt)
    else:
        x_bar = np.zeros(x.shape, dtype=cdt)
        x_bar[..., :: D + 1] = pop_bar
    out = dict(f)
    out.update({"x_bar": x_bar, "conf_bar": conf_bar, "rescale_bar": rescale_bar, "pop_bar": pop_bar, "sim_bar": sim_bar})
    return out


def confusion_rows_bar(rows, conf_bar, dtype):
    """Cotangent of every row [P,d_q] from conf_bar [P,R,D], by the product rule over the Kronecker factors."""
    rows = [np.asarray(r, dtype=dtype) for r in rows]
    P = conf_bar.shape[0]
    rows = [np.broadcast_to(r, (P,) + r.shape) if r.ndim == 1 else r for r in rows]
    out = [np.zeros(r.shape, dtype=dtype) for r in rows]
    for p in range(P):
        for q in range(len(rows)):
            for j in range(rows[q].shape[1]):
                unit = np.zeros((2, rows[q].shape[1]), dtype=dtype)
                unit[0, j], unit[1, j] = 1, -1
                mat = np.ones((1, 1), dtype=dtype)
                for k, r in enumerate(rows):
                    mat = np.kron(mat, unit if k == q else np.stack([r[p], 1 - r[p]]))
                out[q][p, j] = np.sum(mat * conf_bar[p])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# test problems (tests/test_readout_ref.py, tests/test_gpu_readout.py)
# ---------------------------------------------------------------------------------------------------------------------------
DIMS = {2: (2,), 3: (3,), 6: (3, 2), 9: (3, 3)}


def make_case(seed, D, density, P, S, conf, rescale, labels):
    """One read-out problem in float64.  `conf` / `rescale`: "none", "shared" or "perset"; `labels`: "one", "repeated" or "none".

    Populations sum to 1 per sequence and lean towards state 0 (weights (5,1,..) for D <= 3, (2,1,..) above, each within 10 %), so
    that every simulated value -- a single population of nine, or a label counted twice -- stays inside [0.05, 0.95]; confusion rows
    in the reference's bounds (entry 0 in 0.8-1.0, the others in 0-0.2, test/test_model.py:88-92); scale in [0.9, 1.1], offset in
    [-0.02, 0.02]; measured values within 0.05 of the simulated ones, 500-2000 shots."""
    rng = np.random.default_rng(seed)
    dims = DIMS[D]
    base = np.ones(D)
    base[0] = 5.0 if D <= 3 else 2.0
    pop = base * rng.uniform(0.9, 1.1, size=(P, S, D))
    pop /= pop.sum(-1, keepdims=True)
    if density:  # rho = sum_n pop_n |n><n| + a Hermitian off-diagonal part (which the read-out must ignore)
        A = rng.normal(size=(P, S, D, D)) + 1j * rng.normal(size=(P, S, D, D))
        rho = 0.05 * (A + np.conj(np.swapaxes(A, -1, -2)))
        idx = np.arange(D)
        rho[..., idx, idx] = pop
        x = np.swapaxes(rho, -1, -2).reshape(P, S, D * D)
    else:
        x = np.sqrt(pop) * np.exp(1j * rng.uniform(0, 2 * np.pi, size=(P, S, D)))
    rows = None
    if conf != "none":
        rows = []
        for d in dims:
            shape = (P, d) if conf == "perset" else (d,)
            r = rng.uniform(0.0, 0.2, size=shape)
            r[..., 0] = rng.uniform(0.8, 1.0, size=shape[:-1])
            rows.append(r)
    R = D if rows is None else 2 ** len(dims)
    scale = offset = None
    if rescale != "none":
        n = P if rescale == "perset" else 1
        scale, offset = rng.uniform(0.9, 1.1, size=n), rng.uniform(-0.02, 0.02, size=n)
        if rescale == "shared":
            scale, offset = float(scale[0]), float(offset[0])
    idx = {"one": [1], "repeated": [R - 1, 0, R - 1][:: 2], "none": None}[labels]  # (repeated: the last row, twice)
    label_w = None
    if idx is not None:
        label_w = np.zeros(R)
        np.add.at(label_w, idx, 1.0)
    V = 1 if idx is not None else R
    cm = None if rows is None else confusion_matrix(rows, np.float64)
    sim = forward(x, D, cm, label_w, scale, offset, np.zeros((P, S, V)), np.ones((P, S, V)), np.ones((P, S, V)), "rms_dist", np.float64)["sim"]
    meas = sim + rng.uniform(-0.05, 0.05, size=sim.shape)
    stds = rng.uniform(0.01, 0.05, size=sim.shape)
    shots = rng.integers(500, 2001, size=sim.shape).astype(np.float64)
    weights = rng.uniform(0.5, 1.5, size=P)
    return {"D": D, "dims": dims, "x": np.ascontiguousarray(x.astype(np.complex128)), "rows": rows, "conf": cm, "label_idx": idx, "label_w": label_w, "scale": scale,
            "offset": offset, "meas": meas, "stds": stds, "shots": shots, "weights": weights / weights.sum(), "sim64": sim, "R": R, "V": V}


def run_case(c, name, dtype):
    """`reverse` on a case of `make_case`, with the confusion matrix formed in `dtype`."""
    cm = None if c["rows"] is None else confusion_matrix(c["rows"], dtype)
    return reverse(c["x"], c["D"], cm, c["label_w"], c["scale"], c["offset"], c["meas"], c["stds"], c["shots"], name, c["weights"], dtype)
