#!/usr/bin/env python3
"""What the segments that take the degree-8 pair cost the headline launch (cfg2: D = 9, K = 2, N = 1000, B = 256).

By the sum of norms three samples of `workloads.make_workload(2, B=256)` (47, 74, 149) have a wave whose bound exceeds the radius of
the degree-6 pair (tests/test_norm_bound.py), and the launch ends with its slowest workgroup.  This script times
`BatchPropagator.run` with HIP events after a clock ramp,

  (a) on the workload as it is,
  (b) with the control samples of those three samples overwritten by those of sample 0 (every workgroup on the degree-6 pair),

alternating, `--rounds` times each.  With `--skews 672,700,704` it times the workload as it is at each value of the `mw_skew`
option instead (long segments of 42, 43 and 44 slices), alternating as well.

    python tests/perf/bench_norm_bound.py --out norm_bound.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HOT = (47, 74, 149)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ramp-ms", type=float, default=60.0)
    ap.add_argument("--skews", default=None, help="comma-separated mw_skew values (per mille) to alternate instead of (a) / (b)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from c3_amd import _lib, propagation, workloads

    _lib.require_gpu()
    dev = torch.device("cuda:0")
    wl = workloads.make_workload(2, B=256)
    sig_b = wl.signals.copy()
    for b in HOT:
        sig_b[b] = wl.signals[0]

    def propagator(sig):
        return propagation.BatchPropagator(torch.as_tensor(wl.h0, device=dev), torch.as_tensor(wl.hks, device=dev), torch.as_tensor(sig, device=dev),
                                           wl.dt, fr_phase=torch.as_tensor(wl.fr_phase, device=dev))

    out = torch.zeros((wl.B, wl.D, wl.D), dtype=torch.complex128, device=dev)

    def time_us(bp):
        """ramp, then `launches` launches between two HIP events: microseconds per launch"""
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.ramp_ms:
            for _ in range(16):
                bp.run(out=out)
            torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(args.launches):
            bp.run(out=out)
        ev1.record()
        torch.cuda.synchronize()
        return 1e3 * ev0.elapsed_time(ev1) / args.launches

    series = {}
    if args.skews:
        bp = propagator(wl.signals)
        skews = [int(s) for s in args.skews.split(",")]
        for _ in range(args.rounds):
            for s in skews:
                with _lib.options(mw_skew=s):
                    series.setdefault(f"mw_skew={s}", []).append(time_us(bp))
    else:
        variants = {"a: workload as it is": propagator(wl.signals), "b: samples 47, 74, 149 take the controls of sample 0": propagator(sig_b)}
        time_us(variants["a: workload as it is"])  # discarded
        for _ in range(args.rounds):
            for name, bp in variants.items():
                series.setdefault(name, []).append(time_us(bp))
    res = {"what": "cfg2 BatchPropagator.run, microseconds per launch by HIP events over %d launches after a %g ms ramp, alternating" % (args.launches, args.ramp_ms),
           "kernel": _lib.last_kernel_detail(), "library": os.path.basename(_lib.LIB_PATH), "series_us": series,
           "median_us": {k: float(np.median(v)) for k, v in series.items()},
           "min_max_us": {k: [float(min(v)), float(max(v))] for k, v in series.items()}}
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
