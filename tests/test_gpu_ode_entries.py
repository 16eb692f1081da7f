"""The three ODE entries (`c3p_ode_solve`, `c3p_ode_solve_vjp`, `c3p_rk4_unitary`) pinned to recorded runs: for every route
of the host layer, on host and on device pointers, the launch log, the kernel id and the sha256 of every output equal what
tests/golden/ode_entries.json holds (written by tests/golden/make_golden_ode_entries.py from the library before the entries
were given one call record and one route).  The ODE kernels and the vjp use no atomics, so the bits repeat.  The shapes are the
smallest at which each branch of the route is still taken.  A second test holds the timing event pair to every route.  -m gpu."""
import ctypes
import hashlib
import json

import numpy as np
import pytest

ROUTES = ("host", "device")

# what a route leaves in the launch log and reports as its kernel: (kernel id, kernels present, kernels absent)
SIGNS = {
    "row": ("ode_row", (), ("ode_identity_kernel", "ode_kernel", "ode_assemble_hs_kernel")),
    "row_seg": ("ode_row", ("ode_identity_kernel", "ode_vec_kernel", "ode_apply_kernel"), ("ode_starts_kernel", "ode_rhoq_kernel")),
    "row_traj": ("ode_row", ("ode_identity_kernel", "ode_vec_kernel", "ode_starts_kernel"), ("ode_apply_kernel", "ode_rhoq_kernel")),
    "row_hs": ("ode_row", ("ode_assemble_hs_kernel", "ode_vec_kernel"), ("ode_kernel",)),
    "row_or_wg": ("ode_row_or_wg", ("ode_mat_kernel", "ode_kernel"), ()),
    "row_no_split": ("ode_row", ("ode_mat_kernel",), ("ode_kernel",)),
    "rowq": ("ode_row", ("ode_vecq_kernel",), ("ode_identity_kernel", "ode_rhoq_kernel")),
    "mfma_seg": ("ode_mfma", ("ode_identity_kernel", "ode_rhoq_kernel", "ode_apply_kernel"), ("ode_vecq_kernel",)),
    "mfma_traj": ("ode_row", ("ode_identity_kernel", "ode_rhoq_kernel", "ode_starts_kernel", "ode_vecq_kernel"), ()),
    "rhoq": ("ode_mfma", ("ode_rhoq_kernel",), ("ode_identity_kernel", "ode_vecq_kernel")),
    "wg": ("ode_wg", ("ode_kernel",), ("ode_vec_kernel", "ode_mat_kernel", "ode_vecq_kernel", "ode_rhoq_kernel")),
    # c3p_rk4_unitary launches the identity itself on every route
    "u_row": ("ode_row", ("ode_identity_kernel", "ode_vec_kernel"), ("ode_apply_kernel", "midd", "smalld")),
    "u_row_seg": ("ode_row", ("ode_identity_kernel", "ode_vec_kernel", "smalld"), ("ode_apply_kernel",)),
    "u_rhoq": ("ode_mfma", ("ode_rhoq_kernel",), ("midd", "ode_vecq_kernel")),
    "u_mfma_seg": ("ode_mfma", ("ode_rhoq_kernel", "midd"), ("ode_vecq_kernel",)),
    "u_rowq": ("ode_row", ("ode_vecq_kernel",), ("ode_rhoq_kernel",)),
    "u_wg": ("ode_wg", ("ode_kernel",), ("ode_vec_kernel", "ode_vecq_kernel", "ode_rhoq_kernel")),
    "vjp_row": ("ode_vjp", ("ode_vjp_row_kernel", "checkpoint interval"), ("ode_vjp_wg_kernel",)),
    "vjp_wg": ("ode_vjp", ("ode_vjp_wg_kernel", "checkpoint interval"), ("ode_vjp_row_kernel",)),
}

# c3p_ode_solve through ode_solve_batch: name -> (route, step, D, B, N, K, C, final_only, solver, per-sample init, options)
SOLVE = {
    "row-schrodinger": ("row", "schrodinger", 3, 5, 20, 2, 0, False, "rk4", False, {}),  # a ragged wave of four rows
    "row-von_neumann": ("row", "von_neumann", 4, 3, 12, 2, 0, False, "rk4", True, {}),
    "row-lindblad": ("row", "lindblad", 3, 3, 12, 2, 1, False, "rk4", False, {}),  # the aux slot
    "row_seg-rk4": ("row_seg", "schrodinger", 3, 2, 256, 2, 0, True, "rk4", False, {}),  # the cost model picks S = 8
    "row_seg-tsit5": ("row_seg", "schrodinger", 3, 2, 256, 2, 0, True, "tsit5", False, {}),  # the other `fixed` term
    "row_traj-rk4": ("row_traj", "schrodinger", 3, 2, 256, 2, 0, False, "rk4", False, {}),
    "row_traj-tsit5": ("row_traj", "schrodinger", 3, 2, 256, 2, 0, False, "tsit5", False, {}),
    "row_hs-k5": ("row_hs", "schrodinger", 4, 3, 12, 5, 0, False, "rk4", False, {}),
    "row_or_wg-k5": ("row_or_wg", "von_neumann", 4, 3, 12, 5, 0, False, "rk4", False, {}),
    "row_no_split-k5": ("row_no_split", "von_neumann", 4, 3, 12, 5, 0, False, "rk4", False, {"ode_no_split": 1}),
    "rowq-d17": ("rowq", "schrodinger", 17, 3, 12, 2, 0, False, "rk4", False, {}),
    "mfma_seg-d17": ("mfma_seg", "schrodinger", 17, 1, 64, 2, 0, True, "rk4", False, {}),  # S = 4
    "mfma_traj-d17": ("mfma_traj", "schrodinger", 17, 1, 64, 2, 0, False, "rk4", False, {}),  # S = 4
    "rhoq-von_neumann": ("rhoq", "von_neumann", 17, 2, 8, 2, 0, False, "rk4", False, {}),
    "rhoq-lindblad": ("rhoq", "lindblad", 17, 2, 8, 2, 1, False, "rk4", False, {}),
    "wg-d29-lds": ("wg", "von_neumann", 29, 2, 4, 2, 0, False, "rk4", False, {"ode_wg": 1}),  # 11 * 29^2 = 9251 elements <= 9600
    "wg-d30-global": ("wg", "von_neumann", 30, 2, 4, 2, 0, False, "rk4", False, {"ode_wg": 1}),  # 9900 elements
    "wg-d49": ("wg", "schrodinger", 49, 2, 4, 2, 0, False, "rk4", False, {}),
}

# c3p_rk4_unitary: name -> (route, D, B, Ns, K, supplied hs, dUs wanted, options)
RK4 = {
    "u_row-dus": ("u_row", 3, 2, 9, 2, False, True, {}),
    "u_row-nodus": ("u_row", 3, 2, 9, 2, False, False, {}),
    "u_row_seg-ns513": ("u_row_seg", 3, 1, 513, 2, False, False, {}),
    "u_row-hs": ("u_row", 3, 2, 9, 0, True, True, {}),
    "u_rhoq-dus": ("u_rhoq", 17, 2, 9, 2, False, True, {}),
    "u_mfma_seg-ns129": ("u_mfma_seg", 17, 1, 129, 2, False, True, {}),  # S = 4; the per-step pass is not segmented
    "u_rowq-prop_rows": ("u_rowq", 17, 2, 9, 2, False, True, {"ode_prop_rows": 1}),
    "u_wg-hs": ("u_wg", 17, 2, 9, 0, True, True, {}),
    "u_wg-d29-lds": ("u_wg", 29, 1, 5, 2, False, True, {"ode_wg": 1}),
    "u_wg-d30-global": ("u_wg", 30, 1, 5, 2, False, True, {"ode_wg": 1}),
}

# c3p_ode_solve_vjp: name -> (route, step, D, B, N, K, C, what is given: "bar" | "bar_all" | "target")
VJP = {
    f"{plan}-{step}-{given}": (plan, step, D, 3, 12, 2, C, given)
    for plan, step, D, C, givens in (
        ("vjp_row", "schrodinger", 3, 0, ("bar", "bar_all", "target")),
        ("vjp_wg", "schrodinger", 17, 0, ("bar", "bar_all", "target")),
        ("vjp_wg", "lindblad", 3, 1, ("bar",)),  # (rho-valued adjoints run on the workgroup kernel)
    )
    for given in givens
}

CASE_IDS = [f"{name}-{r}" for table in (SOLVE, RK4, VJP) for name in table for r in ROUTES]


def _hermitian(rng, *lead, D):
    a = rng.normal(size=lead + (D, D)) + 1j * rng.normal(size=lead + (D, D))
    return (a + np.conj(np.swapaxes(a, -1, -2))) / (2 * np.sqrt(D))


def _operators(name, table, D, B, N, K):
    """(rng, h0 [D,D], hks [K,D,D], signals [B,K,N]) from a generator seeded per case"""
    rng = np.random.default_rng(2300 + list(table).index(name))
    return rng, _hermitian(rng, D=D), _hermitian(rng, K, D=D), rng.uniform(-1, 1, (B, K, N))


def _state(rng, lead, D, M):
    if M == 1:
        psi = rng.normal(size=lead + (D, 1)) + 1j * rng.normal(size=lead + (D, 1))
        return psi / np.linalg.norm(psi, axis=-2, keepdims=True)
    a = rng.normal(size=lead + (D, D)) + 1j * rng.normal(size=lead + (D, D))
    rho = a @ np.conj(np.swapaxes(a, -1, -2))
    return rho / np.trace(rho, axis1=-2, axis2=-1)[..., None, None]


def _rk4_unitary(lib, torch, route, h0, hks, sig, hs, B, K, Ns, D, want_dUs):
    """c3p_rk4_unitary on host arrays (flag C3P_HOST_PTRS) or on device tensors of the current stream -> [U, dUs?]"""
    n_steps = (Ns - 1) // 2
    if route == "host":
        keep = [None if a is None else np.ascontiguousarray(a) for a in (h0, hks, sig, hs)]
        outs = [np.zeros((B, D, D), complex)] + ([np.zeros((B, n_steps, D, D), complex)] if want_dUs else [])
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        flags, stream = 1, None
    else:
        dev = torch.device("cuda:0")
        keep = [None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (h0, hks, sig, hs)]
        outs = [torch.zeros((B, D, D), dtype=torch.complex128, device=dev)]
        outs += [torch.zeros((B, n_steps, D, D), dtype=torch.complex128, device=dev)] if want_dUs else []
        p = lambda a: None if a is None else a.data_ptr()
        flags, stream = 0, torch.cuda.current_stream(dev).cuda_stream
    hs_bstride = 0 if hs is None else Ns * D * D
    rc = lib.c3p_rk4_unitary(p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), hs_bstride, 0.05, B, K, Ns, D, flags, p(outs[0]),
                             p(outs[1]) if want_dUs else None, stream)
    assert rc == 0, lib.c3p_last_error()
    return outs


def run_cases(propagation, _lib):
    """Every case once -> {case id: {"log": launch log, "kernel": last_kernel(), "sha256": [digest of each output, in the order
    returned]}}.  `propagation` and `_lib` are the modules of the library under test (the golden script hands over those of
    another tree).  Every case must take the route it is named after."""
    import torch

    dev = torch.device("cuda:0")
    lib = _lib.load()
    out = {}

    def record(case, route, sign, res):
        log, kernel = _lib.last_kernel_detail(), _lib.last_kernel()
        arrays = [np.ascontiguousarray(r.cpu().numpy() if route == "device" else r) for r in res if r is not None]
        assert all(np.isfinite(a).all() for a in arrays) and all(a.any() for a in arrays), case
        want_kernel, present, absent = SIGNS[sign]
        assert kernel == want_kernel and all(s in log for s in present) and not any(s in log for s in absent), (case, kernel, log)
        out[f"{case}-{route}"] = {"log": log, "kernel": kernel, "sha256": [hashlib.sha256(a.tobytes()).hexdigest() for a in arrays]}

    for name, (sign, step, D, B, N, K, C, final_only, solver, per_sample, opts) in SOLVE.items():
        rng, h0, hks, sig = _operators(name, SOLVE, D, B, N, K)
        init = _state(rng, (B,) if per_sample else (), D, 1 if step == "schrodinger" else D)
        col = 0.3 * (rng.normal(size=(C, D, D)) + 1j * rng.normal(size=(C, D, D))) / np.sqrt(D) if C else None
        for route in ROUTES:
            up = (lambda a: None if a is None else torch.as_tensor(a, device=dev)) if route == "device" else (lambda a: a)
            with _lib.options(**opts):
                res = propagation.ode_solve_batch(up(h0), up(hks), up(sig), 0.02, up(init), solver, step, col_ops=up(col), final_only=final_only)
                record(name, route, sign, [res])

    for name, (sign, D, B, Ns, K, supplied, want_dUs, opts) in RK4.items():
        rng, h0, hks, sig = _operators(name, RK4, D, B, Ns, K)
        hs = _hermitian(rng, B, Ns, D=D) if supplied else None
        for route in ROUTES:
            with _lib.options(**opts):
                res = _rk4_unitary(lib, torch, route, *((None, None, None, hs) if supplied else (h0, hks, sig, None)), B, K, Ns, D, want_dUs)
                record(name, route, sign, res)

    for name, (sign, step, D, B, N, K, C, given) in VJP.items():
        rng, h0, hks, sig = _operators(name, VJP, D, B, N, K)
        M = 1 if step == "schrodinger" else D
        init = _state(rng, (B,), D, M)
        col = 0.3 * (rng.normal(size=(C, D, D)) + 1j * rng.normal(size=(C, D, D))) / np.sqrt(D) if C else None
        cot = rng.normal(size=(B, N, D, M)) + 1j * rng.normal(size=(B, N, D, M))
        for route in ROUTES:
            up = (lambda a: None if a is None else torch.as_tensor(a, device=dev)) if route == "device" else (lambda a: a)
            args = (up(h0), up(hks), up(sig), 0.02, up(init))
            if given == "target":
                r = propagation.ode_goal_vjp(*args, up(_state(np.random.default_rng(7), (), D, 1)), "rk4", step, col_ops=up(col))
            else:
                r = propagation.ode_solve_batch_vjp(*args, up(cot if given == "bar_all" else cot[:, -1]), "rk4", step, col_ops=up(col))
            record(name, route, sign, [r["grad_signals"], r["init_bar"], r["goal"], r["states"]])
    return out


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(golden_dir + "/ode_entries.json"))["cases"]


@pytest.fixture(scope="module")
def results(lib):
    from c3_amd import _lib, propagation

    _lib.require_gpu()
    return run_cases(propagation, _lib)


def test_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(CASE_IDS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASE_IDS)
def test_entry_is_the_recorded_one(results, golden, case):
    """the same kernels in the same order, the same kernel id, and the same bits in every output"""
    got, want = results[case], golden[case]
    assert got["log"] == want["log"]
    assert got["kernel"] == want["kernel"]
    assert got["sha256"] == want["sha256"]


@pytest.mark.gpu
def test_every_route_records_its_own_time(lib):
    """With profiling armed, c3p_rk4_unitary (no route of which recorded anything before) and the workgroup route of c3p_ode_solve
    bracket their launches with the event pair: after a long PWC call, c3p_last_kernel_ms() is the short call's own time, not the
    PWC call's value left in place.  The PWC shape is chosen at least ten times as long as either (profiles/r23/README.md)."""
    import torch

    from c3_amd import _lib, propagation

    _lib.require_gpu()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(23)
    up = lambda a: torch.as_tensor(a, device=dev)
    D, B, N = 9, 256, 8000
    pwc = (up(_hermitian(rng, D=D)), up(_hermitian(rng, 2, D=D)), up(rng.uniform(-1, 1, (B, 2, N))), 0.01)
    h0, hks, sig = _hermitian(rng, D=3), _hermitian(rng, 2, D=3), rng.uniform(-1, 1, (1, 2, 5))
    solve = (up(_hermitian(rng, D=4)), up(_hermitian(rng, 2, D=4)), up(rng.uniform(-1, 1, (2, 2, 8))), 0.02, up(_state(rng, (), 4, 4)))

    def ms():
        torch.cuda.synchronize()
        return lib.c3p_last_kernel_ms()

    def short_call(short):
        if short == "rk4_unitary":
            _rk4_unitary(lib, torch, "device", h0, hks, sig, None, 1, 2, 5, 3, True)
            assert _lib.last_kernel() == "ode_row"
        else:
            with _lib.options(ode_wg=1):
                propagation.ode_solve_batch(*solve, "rk4", "von_neumann")
            assert _lib.last_kernel() == "ode_wg"

    assert lib.c3p_set_profiling(1) == 0
    try:
        for short in ("rk4_unitary", "ode_solve under ode_wg"):
            propagation.propagate_batch(*pwc)  # (once unmeasured: a kernel's first launch loads its code object)
            short_call(short)
            propagation.propagate_batch(*pwc)
            t_pwc = ms()
            short_call(short)
            t_short = ms()
            print(f"[event pair] pwc D={D} B={B} N={N}: {t_pwc:.4f} ms; {short}: {t_short:.4f} ms")
            assert 0 < t_short < t_pwc, (short, t_short, t_pwc)
    finally:
        lib.c3p_set_profiling(0)
