"""Model-operator cotangents of the Lindblad path at D = 9 (two qutrits, cfg4's superoperators): c3p_pwc_lindblad_model_vjp_hb
beside c3p_pwc_lindblad_vjp on the same Hermitian-basis sweep.  Device pointers, N = 1000, K = 2, C = 2, B = 64 and B = 256, the
median of 20 calls after 3 warm-ups, one process; one JSON line per shape.

    python tests/perf/bench_lindblad_model_vjp.py [--reps 20] [--warmup 3] [--batches 64,256]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from c3_amd import _lib, propagation as prop
from c3_amd.workloads import make_workload


def problem(B):
    """cfg4's operators and pulses (two coupled qutrits, two drive lines, two collapse operators), a random cotangent, row phases"""
    w = make_workload(4, B=B)
    rng = np.random.default_rng(B)
    Dm = w.h0.shape[-1] ** 2
    Ubar = rng.normal(size=(B, Dm, Dm)) + 1j * rng.normal(size=(B, Dm, Dm))
    ph = rng.uniform(0, 2 * np.pi, size=(B, Dm))
    return w.h0, w.hks, w.signals, w.col_ops, Ubar, ph, w.dt


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--vjp-only", action="store_true", help="time c3p_pwc_lindblad_vjp only (a library without the new entry)")
    a = ap.parse_args()
    _lib.require_gpu()
    t = lambda x: torch.as_tensor(x, device="cuda:0")
    for B in (int(b) for b in a.batches.split(",")):
        *arrs, dt = problem(B)
        h0, hks, sig, col, Ubar, ph = (t(x) for x in arrs)
        D, (K, N), C = int(h0.shape[-1]), (int(x) for x in sig.shape[1:]), int(col.shape[0])
        vjp = median_ms(lambda: prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph), a.reps, a.warmup)
        assert _lib.last_kernel() == "mfma"
        row = {"D": D, "N": N, "K": K, "C": C, "B": B, "lindblad_vjp_ms": vjp[0], "lindblad_vjp_min_max_ms": vjp[1:]}
        if not a.vjp_only:
            hb = median_ms(lambda: prop.propagate_batch_lindblad_vjp(h0, hks, sig, dt, col, Ubar, fr_phase=ph, want_model_grads=True, hermitian_basis=True),
                           a.reps, a.warmup)
            assert _lib.last_kernel() == "mfma"
            row.update({"lindblad_model_vjp_hb_ms": hb[0], "lindblad_model_vjp_hb_min_max_ms": hb[1:], "ratio": hb[0] / vjp[0]})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
