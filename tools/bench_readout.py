#!/usr/bin/env python3
"""One `goal_run_batched_with_grad` evaluation with `device=` set: the host epilogue (sim.cpu(), g_LL_prime and its gradient in numpy,
the cotangent copied back) against the device epilogue (`readout=Readout()`: c3p_readout_goal_vjp between c3p_seq_chain and
c3p_seq_chain_vjp).

  python tools/bench_readout.py [--runs 20] [--warmup 3] [--shapes closed,open] [--only host|device] [--out FILE]

One JSON line per shape (GPU required); cfg2's model (two qutrits, D = 9, K = 2), P = 256 parameter sets, three gates, S = 64
sequences of length 20, labels [1, 4], g_LL_prime, the same data for both routes:
  closed:  N = 1000 slices, kets (M = 9)
  open:    N = 100 slices, one collapse operator per qutrit, density vectors (M = 81)
  eval_host_ms, eval_device_ms          wall time of the whole evaluation, torch.cuda.synchronize() before and after, median of
                                        --runs after --warmup evaluations, the two routes alternating
  epilogue_host_ms, epilogue_device_ms  the epilogue alone on the sequence states of the last evaluation, timed the same way:
                                        for the host route the statements of model_learning between evaluate_sequences_indexed
                                        and evaluate_sequences_indexed_vjp, for the device route `readout_goal_vjp`
--only restricts the run to one route (for a profiler run: `rocprofv3 --kernel-trace --stats -- python tools/bench_readout.py --only device`).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from c3_amd import workloads  # noqa: E402

P, S, L = 256, 64, 20
LABELS = [1, 4]


def problem(kind):
    N = 1000 if kind == "closed" else 100
    w = workloads.make_workload(2, B=P, N=N)
    rng = np.random.default_rng(19)
    gates = {"rx90p[0]": w.signals, "ry90p[1]": w.signals[::-1].copy() * 0.7, "cr[0,1]": rng.normal(size=w.signals.shape) * 2e8}
    names = list(gates)
    seqs = [[names[i] for i in rng.integers(0, len(names), size=L)] for _ in range(S)]
    psi0 = np.zeros(w.D, dtype=np.complex128)
    psi0[0] = 1.0
    col = None
    if kind == "open":
        a = workloads.annihilators(w.dims)
        T = workloads.dressing_transform(workloads.bare_drift(w.dims, workloads._FREQS[:2], workloads._ANHARS[:2], {(0, 1): workloads._G}))
        col = np.stack([workloads.dress(workloads.qubit_collapse_op(x, 30e-6, 20e-6), T) for x in a])
    return w, gates, seqs, psi0, col


def wall_ms(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="closed,open")
    ap.add_argument("--only", choices=["host", "device"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from c3_amd import _lib, model_learning as ml, propagation, readout as ro, sequences as sq

    assert torch.cuda.is_available(), "bench_readout.py needs a GPU"
    dev = "cuda:0"
    out = open(a.out, "w") if a.out else None
    for kind in a.shapes.split(","):
        w, gates, seqs, psi0, col = problem(kind)
        D = w.D
        # the data: the simulated values of this model, moved by up to 0.02
        dummy = [{"seqs": seqs, "results": np.full(S, 0.5), "results_std": np.full(S, 0.02), "shots": np.full(S, 1000.0)} for _ in range(P)]
        sim = ml.goal_run_batched(w.h0, w.hks, gates, w.dt, dummy, psi0, LABELS, device=dev, col_ops=col, readout=ro.Readout())["sim_vals"]
        rng = np.random.default_rng(23)
        data = [{"seqs": seqs, "results": np.clip(sim[p] + rng.uniform(-0.02, 0.02, size=S), 0.01, 0.99), "results_std": np.full(S, 0.02), "shots": np.full(S, 1000.0)}
                for p in range(P)]
        routes = {"host": None, "device": ro.Readout()}
        if a.only:
            routes = {a.only: routes[a.only]}
        run = {k: (lambda rd=rd: ml.goal_run_batched_with_grad(w.h0, w.hks, gates, w.dt, data, psi0, LABELS, device=dev, col_ops=col, readout=rd)) for k, rd in routes.items()}
        res = {}
        for _ in range(a.warmup):
            for k, fn in run.items():
                res[k] = fn()
        ts = {k: [] for k in run}
        for _ in range(a.runs):
            for k, fn in run.items():
                ts[k].append(wall_ms(fn, torch))
        line = {"shape": kind, "P": P, "S": S, "L": L, "D": D, "M": D if col is None else D * D, "N": w.N, "runs": a.runs, "warmup": a.warmup}
        for k in run:
            line[f"eval_{k}_ms"], line[f"eval_{k}_ms_runs"] = statistics.median(ts[k]), ts[k]
        if len(run) == 2:
            line["goal_host"], line["goal_device"] = float(res["host"]["goal"]), float(res["device"]["goal"])
            g0, g1 = res["host"]["grad_h0"].cpu().numpy(), res["device"]["grad_h0"].cpu().numpy()
            line["grad_h0_rel_diff"] = float(np.max(np.abs(g0 - g1)) / np.max(np.abs(g0)))
        # the epilogue alone, on the sequence states of this problem
        if col is None:
            x = ml._closed_system_states(w.h0, w.hks, gates, w.dt, P, seqs, psi0, None, dev)[2]
        else:
            x = ml._open_system_states(w.h0, w.hks, gates, w.dt, col, P, seqs, psi0, None, dev)[4]
        stacked = ro.stack_data(data, dev)
        weights = torch.full((P,), 1.0 / P, dtype=torch.float64, device=dev)

        def epilogue_device():
            return ro.readout_goal_vjp(x, ro.Readout(), stacked, LABELS, "g_LL_prime", weights, dim=D)["x_bar"]

        def epilogue_host():
            pops = x.real**2 + x.imag**2 if col is None else x[..., :: D + 1].real
            s = ml.process_batch(pops, LABELS)
            s_h = s.cpu().numpy()
            goals = np.array([ml.g_LL_prime(d["results"], s_h[p], d["results_std"], d["shots"]) for p, d in enumerate(data)])
            dgs = [ml.g_LL_prime_grad(d["results"], s_h[p], d["results_std"], d["shots"]) for p, d in enumerate(data)]
            sim_bar = np.stack([g / P for g in dgs])
            rows = np.zeros(D)
            np.add.at(rows, LABELS, 1.0)
            pop_bar = sim_bar[..., None] * rows
            if col is None:
                return goals, 2.0 * torch.as_tensor(pop_bar, device=dev) * x
            xb = np.zeros(pop_bar.shape[:-1] + (D * D,), dtype=np.complex128)
            xb[..., :: D + 1] = pop_bar
            return goals, torch.as_tensor(xb, device=dev)

        for k, fn in (("host", epilogue_host), ("device", epilogue_device)):
            if a.only and a.only != k:
                continue
            for _ in range(a.warmup):
                fn()
            t = [wall_ms(fn, torch) for _ in range(a.runs)]
            line[f"epilogue_{k}_ms"], line[f"epilogue_{k}_ms_runs"] = statistics.median(t), t
            if k == "device":
                line["epilogue_device_kernels"] = _lib.last_kernel_detail()
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()


if __name__ == "__main__":
    main()
