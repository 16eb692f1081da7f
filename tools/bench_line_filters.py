#!/usr/bin/env python3
"""Line filters at the tunable-coupler shape: B = 256 samples, K = 3 flux lines (legacy Response of 30 taps each), N = 10 000,
Na = 240, one exp_iir stage per line; `synthesize_signals` and `synthesize_signals_vjp` with device-resident inputs.

  python tools/bench_line_filters.py [--runs 20] [--warmup 3] [--only forward] [--no-cpu] [--no-propagate] [--dump FILE]

One JSON line (GPU required).  Times are HIP events round one call, median of --runs after --warmup calls:
  fwd_ms, vjp_ms            the call with one stage per line
  fwd_f0_ms, vjp_f0_ms      the same call with F = 0 (stage buffers, mix and cotangent kernels, no convolution)
  fwd_fma_per_s ...         FMAs the stages need over the time the stages add (fwd_ms - fwd_f0_ms): forward B K 2 N (N + 1) / 2,
                            the vjp three times that (the recomputed forward, the tap cotangent, the input cotangent), and their
                            share of the 39.3 T FMA/s fp64 vector peak
  cpu_fft_ms                the restatement's FFT route (tests/line_filter_ref.py tf_convolve) over the same B K 2 rows on 16 threads
  propagate_ms              propagate_batch at D = 27 with the same K, N and B (cfg3's model), in the same session
C3P_LIB=<path> selects another build of the library (tools/ab_build.sh plain c3p_signal.hip -DC3P_FILT_PLAIN: the plain tile
loop as the forward stage kernel); --dump writes sample 0's signals for comparing two builds.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

B, K, N, NA = 256, 3, 10000, 240
GRID = (0.0, 100e-9, 2.4e9, 100e9)
PEAK_FMA = 39.3e12
TWO_PI = 2 * np.pi


def problem():
    from c3_amd import signals as sg

    rng = np.random.default_rng(24)
    T = GRID[1]
    comp = lambda: dict(shape="flattop", amp=rng.uniform(0.2, 0.4), t_final=T, t_up=rng.uniform(4e-9, 8e-9), t_down=T - rng.uniform(4e-9, 8e-9), risefall=rng.uniform(1.5e-9, 3e-9),
                        xy_angle=rng.uniform(0, 1), freq_offset=rng.uniform(-5e7, 5e7) * TWO_PI)
    line = lambda: dict(kind="flux", rise_time=0.3e-9, phi_0=10.0, phi=2.3 * rng.uniform(0.95, 1.05), omega_0=8.1e9 * TWO_PI, anhar=-286e6 * TWO_PI, d=0.36)
    stage = lambda: {"kind": "exp_iir", "time_iir": rng.uniform(5e-9, 20e-9), "amp": rng.uniform(-0.2, 0.2)}
    env = np.concatenate([sg.pack_components([[comp()] for _ in range(K)])[0] for _ in range(B)])
    shapes = sg.pack_components([[comp()] for _ in range(K)])[1]
    kinds = sg.pack_lines([line() for _ in range(K)], sim_res=GRID[3])[0]
    par = np.concatenate([sg.pack_lines([line() for _ in range(K)], sim_res=GRID[3])[1] for _ in range(B)])
    fk = sg.pack_line_filters([[stage()] for _ in range(K)])[0]
    fp = np.concatenate([sg.pack_line_filters([[stage()] for _ in range(K)])[1] for _ in range(B)])
    carrier = np.tile(np.array([[829e6 * TWO_PI, 1.0]]), (B, K, 1))
    return env, shapes, carrier, kinds, par, fk, fp, rng.normal(size=(B, K, N))


def event_ms(fn, torch, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), ts


def cpu_fft_ms():
    """tf_convolve over B K 2 rows of N samples with N taps each, 16 threads (numpy's FFT releases the GIL)"""
    from multiprocessing.pool import ThreadPool

    import line_filter_ref as ref

    rng = np.random.default_rng(1)
    x, h = rng.normal(size=(B * K * 2, N)), rng.normal(size=(B * K, N))
    with ThreadPool(16) as pool:
        t0 = time.perf_counter()
        pool.map(lambda r: ref.tf_convolve(x[r], h[r // 2]).real, range(x.shape[0]))
        return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["forward"], default=None)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-propagate", action="store_true")
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    assert a.runs >= 1 and a.warmup >= 0

    import torch

    from c3_amd import _lib, propagation, signals as sg, workloads

    assert torch.cuda.is_available(), "bench_line_filters.py needs a GPU"
    assert sg.slice_num(GRID[0], GRID[1], GRID[3]) == N and sg.slice_num(GRID[0], GRID[1], GRID[2]) == NA
    dev = lambda x: torch.as_tensor(x, device="cuda:0")
    env, shapes, carrier, kinds, par, fk, fp, gs = problem()
    env, carrier, par, fp, gs = (dev(x) for x in (env, carrier, par, fp, gs))
    none = (np.zeros((K, 0), dtype=np.int32), torch.zeros((B, K, 0, sg.FILT_NPAR), dtype=torch.float64, device="cuda:0"))
    kw = dict(line_kinds=kinds, line_params=par)
    out = {}
    calls = {"fwd": lambda: out.__setitem__("sig", sg.synthesize_signals(env, shapes, carrier, *GRID, **kw, line_filters=(fk, fp))),
             "fwd_f0": lambda: sg.synthesize_signals(env, shapes, carrier, *GRID, **kw, line_filters=none)}
    if a.only is None:
        calls["vjp"] = lambda: sg.synthesize_signals_vjp(env, shapes, carrier, *GRID, gs, **kw, line_filters=(fk, fp))
        calls["vjp_f0"] = lambda: sg.synthesize_signals_vjp(env, shapes, carrier, *GRID, gs, **kw, line_filters=none)
    line = {"lib": os.path.basename(_lib.LIB_PATH), "B": B, "K": K, "N": N, "Na": NA, "F": 1, "runs": a.runs, "warmup": a.warmup}
    for name, fn in calls.items():
        line[name + "_ms"], line[name + "_ms_runs"] = event_ms(fn, torch, a.runs, a.warmup)
        line[name + "_kernels"] = _lib.last_kernel_detail()
    fma = B * K * 2 * N * (N + 1) // 2
    for name, mult in (("fwd", 1), ("vjp", 3)):
        if name + "_ms" in line:
            rate = mult * fma / (1e-3 * (line[name + "_ms"] - line[name + "_f0_ms"]))
            line[name + "_fmas"], line[name + "_fma_per_s"], line[name + "_share_of_vector_peak"] = mult * fma, rate, rate / PEAK_FMA
    if a.dump:
        np.save(a.dump, out["sig"][0].cpu().numpy())
    if not a.no_propagate:
        w = workloads.make_workload(3, B=B, N=N)
        assert w.D == 27 and w.hks.shape[0] == K, (w.D, w.hks.shape)
        h0, hks = dev(w.h0), dev(w.hks)
        sig = out["sig"]
        line["propagate_ms"], line["propagate_ms_runs"] = event_ms(lambda: propagation.propagate_batch(h0, hks, sig, w.dt), torch, max(3, a.runs // 4), 1)
        line["propagate_kernel"] = _lib.last_kernel()
    if not a.no_cpu:
        line["cpu_fft_ms"] = cpu_fft_ms()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
