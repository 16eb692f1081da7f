#!/usr/bin/env python3
"""The sequence-chain gradient (c3p_seq_chain_vjp) against its forward call, and model learning with vs without gradient.

  python tools/bench_seq_vjp.py [--reps 7] [--out FILE]

One JSON line per configuration (GPU required).  Times are host wall clock around calls that end in a device
synchronisation: median of --reps after one warm-up call, every rep in "<name>_reps", the spread (max - min) / median in
"<name>_spread".
  RB shapes (one reference RB call, 20 lengths 5 .. 500 Cliffords x 30 sequences, ~341 k gate factors
  per sample, table of the four generators):
    fwd_population_s   c3p_seq_chain, population mode
    vjp_population_s   c3p_seq_chain_vjp, population mode, with the forward output (the goal and its gradient)
  ORBIT model learning (cfg2: D = 9, 3 gates, 20 sequences of ~25 gates, P = 64 parameter sets):
    goal_s             model_learning.goal_run_batched
    goal_grad_s        model_learning.goal_run_batched_with_grad (device-resident)
Work of the VJP per gate factor: ~3 matrix-vector products (forward, recompute, adjoint) and one outer product,
32 M^2 flops, against 8 M^2 for the forward chain.
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


def timed(fn, reps, sync):
    """(median, [every rep]) of wall-clock seconds, after one untimed warm-up call"""
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


def haar(rng, M, n):
    Z = rng.normal(size=(n, M, M)) + 1j * rng.normal(size=(n, M, M))
    return np.linalg.qr(Z)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from c3_amd import _lib
    from c3_amd import model_learning as ml
    from c3_amd import sequences as sq
    from c3_amd.workloads import make_workload

    assert torch.cuda.is_available(), "bench_seq_vjp.py needs a GPU"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    out = open(a.out, "w") if a.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")

    rng = np.random.default_rng(0)
    lengths = np.rint(np.linspace(5, 500, 20)).astype(int)
    rows = [sq._rb_index_table(sq._rb_cliffords(30, int(L), rng)) for L in lengths]
    Lmax = max(s.shape[1] for s, _ in rows)
    seqs = np.concatenate([np.pad(s, ((0, 0), (0, Lmax - s.shape[1]))) for s, _ in rows])
    lens = np.concatenate([l for _, l in rows])
    S, factors = len(lens), int(lens.sum())
    seqs_d, lens_d = torch.as_tensor(seqs, device=dev), torch.as_tensor(lens, device=dev)
    for label, M, P, superop in [("unitary D=3", 3, 1, False), ("unitary D=3", 3, 64, False), ("Lindblad M=9 (D=3)", 9, 64, True)]:
        Gd = torch.as_tensor(haar(rng, M, P * 4).reshape(P, 4, M, M), device=dev)
        pb = torch.full((P, S), -1.0 / S, dtype=torch.float64, device=dev)
        t_f, r_f = timed(lambda: sq.seq_chain(Gd, seqs_d, lens_d, "population", superop=superop), a.reps, sync)
        t_v, r_v = timed(lambda: sq.seq_chain_vjp(Gd, seqs_d, lens_d, "population", pb, superop=superop, want_out=True), a.reps, sync)
        emit({"config": label, "M": M, "P": P, "sequences": S, "Lmax": int(Lmax), "gate_factors_per_sample": factors,
              "kernels": _lib.last_kernel_detail(), "fwd_population_s": t_f, "vjp_population_s": t_v, "vjp_over_fwd": t_v / t_f,
              "fwd_population_s_reps": r_f, "vjp_population_s_reps": r_v,
              "fwd_population_s_spread": spread(r_f), "vjp_population_s_spread": spread(r_v),
              "flops_fwd": 8 * M * M * factors * P, "flops_vjp": 32 * M * M * factors * P})

    # ORBIT-style model learning on cfg2
    P = 64
    w = make_workload(2, B=P)
    gsig = {"rx90p[0]": w.signals, "ry90p[0]": w.signals[::-1].copy() * 0.7, "rx90m[0]": -w.signals}
    names = list(gsig)
    seqs_n = [[names[i] for i in rng.integers(0, 3, size=int(rng.integers(20, 31)))] for _ in range(20)]
    psi0 = np.zeros(w.D, dtype=np.complex128)
    psi0[0] = 1
    data = [{"seqs": seqs_n, "results": list(rng.uniform(0.1, 0.9, 20)), "results_std": [0.02] * 20, "shots": [1000] * 20} for _ in range(P)]
    h0d, hkd = torch.as_tensor(w.h0, device=dev), torch.as_tensor(w.hks, device=dev)
    sigd = {k: torch.as_tensor(v, device=dev) for k, v in gsig.items()}
    t_g, r_g = timed(lambda: ml.goal_run_batched(h0d, hkd, sigd, w.dt, data, psi0, [1, 4], device=dev), a.reps, sync)
    t_gg, r_gg = timed(lambda: ml.goal_run_batched_with_grad(h0d, hkd, sigd, w.dt, data, psi0, [1, 4], device=dev), a.reps, sync)
    emit({"config": "ORBIT model learning cfg2", "D": w.D, "N": w.N, "P": P, "gates": 3, "sequences": 20,
          "mean_sequence_length": float(np.mean([len(s) for s in seqs_n])), "goal_s": t_g, "goal_grad_s": t_gg,
          "grad_over_goal": t_gg / t_g, "goal_s_reps": r_g, "goal_grad_s_reps": r_gg, "goal_s_spread": spread(r_g),
          "goal_grad_s_spread": spread(r_gg)})


if __name__ == "__main__":
    main()
