"""Per-call time of the ODE entries where the host layer shows: D = 3, B = 4, N = 32 on device tensors, a call of a few
microseconds of kernel time.  Cases: `ode_solve_batch` final state only and whole trajectory, `ode_solve_batch_vjp`, and the
rk4 gate helper (`c3p_rk4_unitary`, Ns = 33, with dUs).

    python tests/perf/bench_ode_host.py [--tree PATH] [--out FILE]

`--tree PATH` times another built checkout (the parent commit, say) with this script: A/B of a host-layer change runs one
process per library, alternating, and compares the medians of the new processes with the min - max range of the old ones.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

D, B, K, N = 3, 4, 2, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ramp-ms", type=float, default=60.0)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), help="the built checkout whose c3_amd is timed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    from c3_amd import _lib, propagation as prop

    assert os.path.abspath(_lib.LIB_PATH).startswith(os.path.abspath(args.tree) + os.sep), _lib.LIB_PATH
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(23)

    def herm(*lead):
        a = rng.normal(size=lead + (D, D)) + 1j * rng.normal(size=lead + (D, D))
        return torch.as_tensor((a + np.conj(np.swapaxes(a, -1, -2))) / 2, device=dev)

    h0, hks = herm(), herm(K)
    sig = torch.as_tensor(rng.uniform(-1, 1, (B, K, N)), device=dev)
    psi = np.zeros((D, 1), complex)
    psi[0] = 1
    psi = torch.as_tensor(psi, device=dev)
    bar = torch.as_tensor(rng.normal(size=(B, D, 1)) + 1j * rng.normal(size=(B, D, 1)), device=dev)
    sig1 = rng.uniform(-1, 1, (K, N + 1))  # (the helper takes one gate's samples from the host)
    calls = {
        "ode_solve_batch final": lambda: prop.ode_solve_batch(h0, hks, sig, 0.02, psi, final_only=True),
        "ode_solve_batch trajectory": lambda: prop.ode_solve_batch(h0, hks, sig, 0.02, psi),
        "ode_solve_batch_vjp": lambda: prop.ode_solve_batch_vjp(h0, hks, sig, 0.02, psi, bar),
        "rk4 gate helper": lambda: prop._rk4_unitary_device(h0=h0, hks=hks, signals=sig1, dt=0.02),
    }

    def window_ms(f, n):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(n):
            f()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    def time_us(f):
        """ramp, a probe, then one window of back-to-back calls between two HIP events: microseconds per call"""
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.ramp_ms:
            for _ in range(16):
                f()
            torch.cuda.synchronize()
        n = max(args.calls, int(np.ceil(args.window_ms / (window_ms(f, args.calls) / args.calls))))
        return 1e3 * window_ms(f, n) / n

    series, kernels = {}, {}
    for key, f in calls.items():
        time_us(f)  # discarded
        kernels[key] = _lib.last_kernel_detail()
    for _ in range(args.rounds):
        for key, f in calls.items():
            series.setdefault(key, []).append(time_us(f))
    res = {"what": "ODE entries at D=%d B=%d K=%d N=%d, device pointers: microseconds per call by HIP events over a window of %g ms after a "
                   "%g ms ramp, cases alternating, %d rounds" % (D, B, K, N, args.window_ms, args.ramp_ms, args.rounds),
           "tree": os.path.abspath(args.tree), "library": _lib.LIB_PATH, "kernels": kernels, "series_us": series,
           "median_us": {k: float(np.median(v)) for k, v in series.items()},
           "min_max_us": {k: [float(min(v)), float(max(v))] for k, v in series.items()}}
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
