#!/usr/bin/env python3
"""Signal synthesis with and without a coefficient table, forward and vector-Jacobian product, at cfg2's line shape
(B = 256, K = 2, N = 1000, Na = 20: 10 ns at 2 GS/s AWG and 100 GS/s simulation resolution), device pointers.

  existing   a gaussian_nonorm row through c3p_synth_signals / c3p_synth_signals_vjp
  tab        the same row through c3p_synth_tab / c3p_synth_tab_vjp with an empty table
  pwc        a pwc row, M = Na
  fourier    a fourier_sin row, M = 16

Each figure is the median over `--rounds` windows of microseconds per call: HIP events around as many back-to-back calls as
fill `--window-ms` (0.3 s by default; the count comes from a probe of `--calls` calls) after a clock ramp; the cases alternate
inside a round.

    python tests/perf/bench_synth_tables.py --out synth_tables.json

`--tree PATH --cases existing` times the existing entries of another built checkout (the parent commit, say) with this
script: run it alternately with this tree's, and several times on its own for its spread.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

GRID = (0.0, 10e-9, 2e9, 100e9)
B, K = 256, 2
TWO_PI = 2 * np.pi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ramp-ms", type=float, default=60.0)
    ap.add_argument("--cases", default="existing,tab,pwc,fourier")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), help="the built checkout whose c3_amd is timed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    from c3_amd import _lib, signals as sg

    _lib.require_gpu()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20)
    N, Na = sg.slice_num(*GRID[:2], GRID[3]), sg.slice_num(*GRID[:3])
    assert (N, Na) == (1000, 20)
    scal = lambda: dict(amp=rng.uniform(0.3, 1.0, B), xy_angle=rng.uniform(-1, 3, B), freq_offset=rng.uniform(-60e6, 60e6, B) * TWO_PI, t_final=10e-9)
    rows = {
        "existing": lambda: dict(scal(), shape="gaussian_nonorm", sigma=2e-9),
        "pwc": lambda: dict(scal(), shape="pwc", inphase=rng.uniform(-1, 1, (B, Na)), quadrature=rng.uniform(-1, 1, (B, Na))),
        "fourier": lambda: dict(scal(), shape="fourier_sin", amps=rng.uniform(-1, 1, (B, 16)), freqs=rng.uniform(1e8, 3e9, (B, 16)), phases=rng.uniform(-1, 1, (B, 16))),
    }
    rows["tab"] = rows["existing"]
    carrier = torch.as_tensor(np.stack([rng.uniform(4e9, 6e9, (B, K)) * TWO_PI, rng.uniform(0.9e9, 1.1e9, (B, K)) * TWO_PI], axis=-1), device=dev)
    gs = torch.as_tensor(rng.normal(size=(B, K, N)), device=dev)
    names = [c for c in args.cases.split(",") if c]
    calls = {}
    for name in names:
        chans = [[rows[name]()] for _ in range(K)]
        if name == "existing":
            env, shapes = sg.pack_components(chans, B=B)
            kw = {}
        else:
            env, shapes, tab, tidx = sg.pack_table_components(chans, B=B, awg_samples=Na)
            kw = dict(env_tables=torch.as_tensor(tab, device=dev), table_index=torch.as_tensor(tidx, device=dev))
        env, shapes = torch.as_tensor(env, device=dev), torch.as_tensor(shapes, device=dev)
        calls[name, "forward"] = lambda env=env, shapes=shapes, kw=kw: sg.synthesize_signals(env, shapes, carrier, *GRID, **kw)
        calls[name, "vjp"] = lambda env=env, shapes=shapes, kw=kw: sg.synthesize_signals_vjp(env, shapes, carrier, *GRID, gs, **kw)

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
        kernels["%s %s" % key] = _lib.last_kernel_detail()
    for _ in range(args.rounds):
        for key, f in calls.items():
            series.setdefault("%s %s" % key, []).append(time_us(f))
    res = {"what": "synthesize_signals / synthesize_signals_vjp at B=%d K=%d N=%d Na=%d, device pointers: microseconds per call by HIP events over a window "
                   "of %g ms after a %g ms ramp, cases alternating, %d rounds" % (B, K, N, Na, args.window_ms, args.ramp_ms, args.rounds),
           "tree": os.path.abspath(args.tree), "library": _lib.LIB_PATH, "kernels": kernels, "series_us": series,
           "median_us": {k: float(np.median(v)) for k, v in series.items()},
           "min_max_us": {k: [float(min(v)), float(max(v))] for k, v in series.items()}}
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
