#!/usr/bin/env python3
"""The device dressing step (c3p_dress, c3p_dress_vjp) against the only alternative, the host route, and against the propagation
call it feeds.

  python tools/bench_dress.py [--runs 20] [--warmup 3] [--workers 16] [--out FILE] [--only dress|dress_vjp] [--skip-host] [--skip-prop]

One JSON line per shape (GPU required):
  cfg2:  P = 256,  D = 9  (two qutrits), M = 2 control Hamiltonians, feeds propagate_batch at B = 256, N = 1000
  cfg5:  P = 1024, D = 36 (dims 3, 3, 4), M = 3,                      feeds propagate_batch at B = 1024, N = 5000
Set p shifts the first frequency by 10 kHz p, so that no two matrices are the same.
  dress_ms, dress_vjp_ms    device time between two events around the C call, device-resident inputs and outputs, median of
                            --runs after --warmup calls (the VJP with cotangents of h0 and of the dressed operators, bare
                            operators shared: the layout model learning uses)
  host_1_ms, host_N_ms      workloads.dressing_transform + dress for every set and operator, one thread, and process-parallel
                            on --workers processes (measured before the GPU is touched; BLAS threads of a worker: 1)
  propagate_ms              the propagation of the same P sets
  sweeps                    Jacobi sweeps to convergence of set 0 (the numpy restatement of the kernel's loop below)
--only restricts the device part to one call (for a profiler run over a single kernel).
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")  # the host route is measured per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from c3_amd import workloads  # noqa: E402

SHAPES = {"cfg2": dict(cfg=2, P=256), "cfg5": dict(cfg=5, P=1024)}


def models(cfg, P):
    c = workloads.CONFIGS[cfg]
    dims, nq = c["dims"], len(c["dims"])
    a = workloads.annihilators(dims)
    H0 = workloads.bare_drift(dims, workloads._FREQS[:nq], workloads._ANHARS[:nq], {(i, j): workloads._G for i in range(nq) for j in range(i + 1, nq)})
    n0 = 2 * np.pi * (a[0].conj().T @ a[0])
    H = np.stack([H0 + 1e4 * p * n0 for p in range(P)])
    ops = np.stack([x + x.conj().T for x in a])
    return H, ops


def host_route(args):
    H, ops = args
    out = []
    for h in H:
        T = workloads.dressing_transform(h)
        out.append((workloads.dress(h, T), [workloads.dress(A, T) for A in ops]))
    return len(out)


def time_host(H, ops, workers, reps=3):
    one = []
    for _ in range(reps):
        t0 = time.perf_counter()
        host_route((H, ops))
        one.append(time.perf_counter() - t0)
    import multiprocessing as mp

    chunks = [(c, ops) for c in np.array_split(H, workers) if len(c)]
    par = []
    with mp.get_context("fork").Pool(workers) as pool:
        pool.map(host_route, chunks)  # start the workers
        for _ in range(reps):
            t0 = time.perf_counter()
            pool.map(host_route, chunks)
            par.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(one), 1e3 * statistics.median(par)


def jacobi_sweeps(H):
    """Sweeps of the kernel's loop on one matrix: cyclic Jacobi, round-robin pairs, converged at off(A) <= D 2^-52 ||A||_F."""
    D = H.shape[0]
    A = np.tril(H) + np.tril(H, -1).conj().T
    thr2 = (D * 2.0**-52) ** 2 * np.sum(np.abs(A) ** 2)
    n = D + (D & 1)
    for sweep in range(31):
        if np.sum(np.abs(A - np.diag(A.diagonal())) ** 2) <= thr2:
            return sweep
        for r in range(n - 1):
            rots = []
            for k in range(n // 2):
                a, b = (n - 1, r) if k == 0 else ((r + k) % (n - 1), (r - k + n - 1) % (n - 1))
                p, q = min(a, b), max(a, b)
                ab = abs(A[p, q]) if q < D else 0.0
                if ab == 0:
                    continue
                tau = (A[q, q].real - A[p, p].real) / (2 * ab)
                t = (1.0 if tau >= 0 else -1.0) / (abs(tau) + np.hypot(1.0, tau))
                c = 1 / np.sqrt(1 + t * t)
                rots.append((p, q, c, t * c * A[p, q] / ab, A[p, p].real - t * ab, A[q, q].real + t * ab))
            for p, q, c, s, _, _ in rots:
                x, y = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * x - np.conj(s) * y, s * x + c * y
            for p, q, c, s, app, aqq in rots:
                x, y = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * x - s * y, np.conj(s) * x + c * y
                A[p, p], A[q, q], A[p, q], A[q, p] = app, aqq, 0, 0
    return -1


def device_ms(fn, torch, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--shapes", default="cfg2,cfg5")
    ap.add_argument("--only", choices=["dress", "dress_vjp"], default=None)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-prop", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    shapes = {k: SHAPES[k] for k in a.shapes.split(",")}
    data = {k: models(s["cfg"], s["P"]) for k, s in shapes.items()}
    # the host route first: worker processes are forked before this process opens the GPU
    host = {k: (None, None) if a.skip_host else time_host(*data[k], a.workers) for k in shapes}

    import torch

    from c3_amd import _lib, propagation

    assert torch.cuda.is_available(), "bench_dress.py needs a GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    out = open(a.out, "w") if a.out else None
    for name, s in shapes.items():
        H, ops = data[name]
        P, D, M = H.shape[0], H.shape[-1], ops.shape[0]
        Hd, od = torch.as_tensor(H, device=dev), torch.as_tensor(ops, device=dev)
        eig = torch.empty((P, D), dtype=torch.float64, device=dev)
        T, h0, gH = (torch.empty((P, D, D), dtype=torch.complex128, device=dev) for _ in range(3))
        G = torch.empty((P, M, D, D), dtype=torch.complex128, device=dev)
        gA = torch.empty((M, D, D), dtype=torch.complex128, device=dev)
        st = torch.empty((P,), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def fwd():
            _lib.check(lib.c3p_dress(Hd.data_ptr(), od.data_ptr(), 0, P, M, D, 0, eig.data_ptr(), T.data_ptr(), h0.data_ptr(), G.data_ptr(), st.data_ptr(), stream))

        def vjp():
            _lib.check(lib.c3p_dress_vjp(T.data_ptr(), eig.data_ptr(), od.data_ptr(), 0, P, M, D, 0, None, h0.data_ptr(), G.data_ptr(), None, gH.data_ptr(), gA.data_ptr(),
                                         st.data_ptr(), stream))

        line = {"shape": name, "P": P, "D": D, "M": M, "runs": a.runs, "warmup": a.warmup, "sweeps": jacobi_sweeps(H[0].copy())}
        fwd()
        if a.only != "dress_vjp":
            line["dress_ms"], line["dress_ms_runs"] = device_ms(fwd, torch, a.warmup, a.runs)
            line["dress_kernels"] = _lib.last_kernel_detail()
            line["status_max"] = int(st.max().item())
        if a.only != "dress":
            line["dress_vjp_ms"], line["dress_vjp_ms_runs"] = device_ms(vjp, torch, a.warmup, a.runs)
            line["dress_vjp_kernels"] = _lib.last_kernel_detail()
        if not a.skip_host:
            line["host_1_ms"], line["host_N_ms"], line["host_workers"] = host[name][0], host[name][1], a.workers
        if not a.skip_prop and a.only is None:
            w = workloads.make_workload(s["cfg"], B=P)
            sig = torch.as_tensor(w.signals, device=dev)
            hk = G.clone()
            h0c = h0.clone()
            prop = lambda: propagation.propagate_batch(h0c, hk, sig, w.dt)
            line["propagate_ms"], line["propagate_ms_runs"] = device_ms(prop, torch, a.warmup, max(3, a.runs // 4))
            line["propagate_N"] = w.N
            line["propagate_kernel"] = _lib.last_kernel()
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()


if __name__ == "__main__":
    main()
