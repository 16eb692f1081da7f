#!/usr/bin/env python
"""Headline benchmark: full-gate propagators/s (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--config C] [--scaling weak|strong] [--batch B] [--check] [--dump-outputs DIR]

One "step" = one pass of the hot path over one batch of synthetic pulse-parameter samples:
U[b] = FR_b * prod_n exp(-i H_b[n] dt) for all b (Lindblad configs: the D^2 x D^2 superoperator).  Default = the
configuration BASELINE.json's metric is quoted on: cfg2, two-qubit CR gate, D=9, 1000 PWC slices, B=256 on one GPU.

Batch and scaling:
  weak   (default) every rank propagates `--batch` samples of its own (default: the config's batch divided by the
         number of GPUs BASELINE.json quotes it on -- cfg2 256, cfg3 4096/8 = 512, cfg4 512, cfg5 8192/8 = 1024);
  strong the GLOBAL batch (`--batch`, default the config's: cfg3 4096, cfg5 8192) is split over the ranks with
         c3_amd.dist.shard_bounds (contiguous shards, sizes differ by at most one).
The only data-path collective is the all-gather of the U slabs over RCCL (c3_amd.dist.SlabRing: the slabs of
`--gather-every` consecutive steps travel in ONE collective).  Inputs are resident in HBM before the timed region.
The value is SUSTAINED throughput: an untimed clock ramp (`--ramp-ms`, default 60 ms) precedes the W warmup steps.
Rank 0 prints ONE JSON line.

Launching N > 1:  `python bench.py --gpus N` starts the N ranks ITSELF (one child process per GPU, RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* set, rendezvous on 127.0.0.1, rank 0's JSON line passed through on stdout); under
`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` (WORLD_SIZE already set) it is a rank.  At N > 1
`--check` is on by default (`--no-check` turns it off).  When there are more ranks than visible devices (two ranks on a
one-GPU box: RCCL refuses that with "Duplicate GPU detected") the ranks share devices and the exchange runs on gloo through
host staging -- the line says so (`oversubscribed`, `backend`) and such a run measures nothing about scaling; it exists so
that the N > 1 code path can be executed on one device.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP64_TFLOPS = 78.6  # MI355X dense fp64 (vector = matrix; 256 CU x 4 SIMD x 32 flop/clk x 2.4 GHz)
PROFILE_ROUND = "r06"

# thresholds of the reference's expm (tf.linalg.expm, Higham 2005 Pade 3/5/7/9/13 chosen from ||A||_1)
_PADE_THETA = (1.495585217958292e-2, 2.539398330063230e-1, 9.504178996162932e-1, 2.097847961257068, 5.371920351148152)
_PADE_PRODUCTS = (2, 3, 4, 5, 6)


def algorithmic_flops_per_prop(wl):
    """sum over slices of F_slice(D,K,m,s) = 8 D^3 (pi_m + s + 1) + (32/3) D^3 + 4 K D^2 with the
    Pade order m / squarings s the REFERENCE's expm would pick per slice from ||A_n||_1; one chain product dropped
    per propagator (+ 4 D^3 per slice of superoperator fill for Lindblad).  Self-contained: the oracle is not
    consulted for the reported roofline."""
    import numpy as np

    H = wl.h0[None] + np.einsum("kn,kij->nij", wl.signals[0], wl.hks)
    if wl.lindblad:
        D = wl.D
        I = np.eye(D)
        clp = np.zeros((D * D, D * D), dtype=np.complex128)
        for c in wl.col_ops:
            spre, spost = np.kron(c, I), np.kron(I, c.T)
            clp += spre @ spost.conj().T - 0.5 * (spre.conj().T @ spre) - 0.5 * (spost @ spost.conj().T)
        norms = np.empty(H.shape[0])
        for n in range(H.shape[0]):  # ||dt L(H_n)||_1 (propagation.py:551-582)
            L = -1j * (np.kron(H[n], I) - np.kron(I, H[n].T)) + clp
            norms[n] = np.abs(L * wl.dt).sum(axis=0).max()
        Dm = D * D
    else:
        norms = np.abs(-1j * H * wl.dt).sum(axis=-2).max(axis=-1)
        Dm = wl.D
    tot = 0.0
    for a in norms:
        idx = int(np.searchsorted(_PADE_THETA, a))
        sq = 0
        if idx >= len(_PADE_THETA):
            idx = len(_PADE_THETA) - 1
            sq = max(0, int(np.floor(np.log2(a / _PADE_THETA[-1]))))  # TF's squaring count
        tot += 8.0 * Dm**3 * (_PADE_PRODUCTS[idx] + sq + 1) + (32.0 / 3.0) * Dm**3 + 4.0 * wl.K * Dm**2
    tot -= 8.0 * Dm**3
    if wl.lindblad:
        tot += 4.0 * wl.D**3 * wl.N
    return float(tot)


# translation units that hold the DOMINANT kernel of each BASELINE configuration (+ the headers they include): an edit of
# another kernel family (gradients, ODE solvers, the API layer) does not invalidate a configuration's PMC profile
_KERNEL_SOURCES = {
    1: ("c3p_smalld.hip", "c3p_smalld.h", "c3p_common.h"),
    2: ("c3p_smalld.hip", "c3p_smalld.h", "c3p_common.h"),
    3: ("c3p_midd.hip", "c3p_midd.h", "c3p_common.h"),
    4: ("c3p_regr.hip", "c3p_regr_common.h", "c3p_regd.h", "c3p_midd.h", "c3p_common.h"),
    5: ("c3p_midd.hip", "c3p_midd.h", "c3p_common.h"),
}


def kernel_sources_digest(config=2):
    """sha1 over the sources of the chain kernel this configuration runs on: PMC numbers in profiles/ are only quoted for
    the build of that kernel they were taken on."""
    h = hashlib.sha1()
    d = os.path.join(ROOT, "c3_amd", "csrc")
    for name in _KERNEL_SOURCES.get(int(config), ()):
        h.update(name.encode())
        h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:12]


def plan_batch(cfg, scaling, batch, world, rank):
    """(global batch, [lo, hi) of this rank, padded slab rows).  See the module docstring."""
    from c3_amd import dist as c3dist

    if scaling == "strong":
        B_glob = int(batch) if batch is not None else int(cfg["B"])
        lo, hi = c3dist.shard_bounds(B_glob, world, rank)
        return B_glob, lo, hi, c3dist.max_shard(B_glob, world)
    per = int(batch) if batch is not None else max(1, int(cfg["B"]) // int(cfg.get("gpus", 1)))
    if batch is None and cfg["B"] == 1:
        per = 256  # cfg1 is the reference's single-sample plumbing case; batched here like cfg2
    return per * world, rank * per, (rank + 1) * per, per


def _claim_stdout():
    """File descriptor 1 is handed to stderr for the whole run and a private duplicate of the real stdout is returned:
    libraries that print banners from C (RCCL's version block at communicator set-up) then cannot put anything in front of
    the ONE JSON line the driver parses."""
    sys.stdout.flush()
    real = os.dup(1)
    os.dup2(2, 1)
    return real


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", type=int, default=2, help="BASELINE.json config index (2 = headline)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--batch", type=int, default=None, help="weak: samples per GPU; strong: GLOBAL batch")
    ap.add_argument("--slices", type=int, default=None)
    ap.add_argument("--overlap-gather", choices=("auto", "on", "off"), nargs="?", const="on", default="auto",
                    help="--exchange gather: issue the all-gather asynchronously and compute the next step(s) into a second bank of slabs "
                         "meanwhile.  auto (default): at N > 1 both forms of the one-gather-per-step schedule are calibrated untimed (same steps, "
                         "MAX over ranks) and the faster one is the timed schedule; off at N = 1")
    ap.add_argument("--gather-every", type=int, default=1,
                    help="steps exchanged per all-gather (multi-GPU).  Default 1 = north_star's schedule: ONE all-gather of U per batch; "
                         "the amortised schedule (32) and the gather-free goal exchange are timed beside it and reported as extra keys")
    ap.add_argument("--no-alt-schedules", action="store_true", help="multi-GPU: skip the side measurements of the other exchange schedules")
    ap.add_argument("--ramp-ms", type=float, default=60.0, help="untimed device clock ramp before the W warmup steps (0 = off)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-e2e", action="store_true", help="skip the PCIe-inclusive side measurement")
    ap.add_argument("--generic", action="store_true", help="force the generic LDS kernel")
    ap.add_argument("--check", action="store_true", default=None, help="verify samples against the oracle (and the gathered slabs); default at N > 1")
    ap.add_argument("--no-check", action="store_false", dest="check")
    ap.add_argument("--backend", choices=("auto", "nccl", "gloo"), default="auto",
                    help="auto: nccl (= RCCL), or gloo with host staging when the ranks outnumber the visible devices")
    ap.add_argument("--complex", action="store_true", dest="complex_ops",
                    help="give the second control operator an imaginary (Hermitian) part: the general complex-Hamiltonian instances instead of the real fast path")
    ap.add_argument("--exchange", choices=("gather", "goal"), default="gather",
                    help="multi-GPU exchange: all-gather of the U slabs (default) or the gather-free optimiser loop: fused fidelity per sample + ONE all-reduce of the goal per step")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the LAST timed step computed as DIR/<name>.npy (float64; see dump_outputs)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, U, goal, rank, world, lo, limit=DUMP_LIMIT_BYTES):
    """Write what the timed path returned in its last step, so that two builds can be compared output for output (the inputs
    are seeded per global sample: the same arguments give the same inputs).  U [B, Dm, Dm] complex128 -> U.npy, float64
    [B, Dm, Dm, 2] (real, imaginary); with --exchange goal also goal.npy = {sum of infidelities, samples}.  Each rank writes
    its own shard (U_rank<r>.npy at N > 1).  The files of all ranks stay under `limit` bytes: beyond that a fixed, seeded
    sample of the batch rows is written, with their global sample indices in U_index.npy (float64).  Returns {file: shape}."""
    import numpy as np
    import torch

    os.makedirs(out_dir, exist_ok=True)
    sfx = "" if world == 1 else f"_rank{rank}"
    arrays = {}
    u = torch.view_as_real(U.detach()).cpu().numpy().astype(np.float64, copy=False)
    per_row = int(np.prod(u.shape[1:])) * 8
    budget = limit // world - 4096  # room for the .npy headers and the goal
    if len(u) * per_row > budget:
        keep = max(1, budget // per_row - 1)  # one row of the budget goes to the index file
        idx = np.sort(np.random.default_rng(20240).choice(len(u), size=keep, replace=False))
        u = u[idx]
        arrays["U_index" + sfx] = (lo + idx).astype(np.float64)
    arrays["U" + sfx] = u
    if goal is not None:
        arrays["goal" + sfx] = goal.detach().cpu().numpy().astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))
    return {name + ".npy": list(a.shape) for name, a in arrays.items()}


def self_launch(n, argv):
    """`python bench.py --gpus N` outside a launcher: start the N ranks as child processes of this one (what
    `torch.distributed.run --standalone --nproc-per-node N` would do, without its agent and log redirection), one per GPU,
    rendezvous on 127.0.0.1 at a free port.  Every child inherits stdout / stderr: rank 0 alone writes the JSON line.  The first
    rank that fails takes the others down (by their own process handles); the exit code is the first non-zero one."""
    import signal
    import tempfile

    # Rendezvous through a FILE store created here (rank 0 never has to win a race for a TCP port that a probe socket found
    # free a moment ago -- ADVICE r5); MASTER_ADDR / MASTER_PORT are still exported for libraries that read them.
    fd, store = tempfile.mkstemp(prefix="c3p_bench_rdzv_")
    os.close(fd)
    os.unlink(store)  # the FileStore creates it; a stale file would carry a previous run's keys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), C3P_BENCH_SELF_LAUNCHED="1", C3P_BENCH_RDZV_FILE=store)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (the host driver supports nothing else)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    live = list(procs)

    def on_term(signum, _frame):  # the parent is told to stop: the ranks must not outlive it
        for q in live:
            q.terminate()
        raise SystemExit(128 + signum)

    old_term = signal.signal(signal.SIGTERM, on_term)
    try:
        while live:
            time.sleep(0.05)
            for p in list(live):
                code = p.poll()
                if code is None:
                    continue
                live.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    print(f"[bench] rank {procs.index(p)} exited with {code}: stopping the other ranks", file=sys.stderr, flush=True)
                    for q in live:
                        q.terminate()
    finally:
        signal.signal(signal.SIGTERM, old_term)
        for q in live:
            q.kill()
        try:
            os.unlink(store)
        except OSError:
            pass
    return rc


class _StandInPropagator:
    """TEST SCAFFOLD (C3P_BENCH_STANDIN=1, tests/test_dist_gloo.py): takes the place of the HIP propagator so that the launcher,
    the sharding, the exchange schedules and the multi-rank check of this file run on CPU ranks over gloo.  It computes nothing:
    element (i, j) of global sample g is g + 1e-3 (i Dm + j) - 1e-6 i.  A stand-in line is labelled as such and is not a
    measurement."""

    def __init__(self, torch, lo, B, Dm):
        g = torch.arange(lo, lo + B, dtype=torch.float64).reshape(B, 1, 1)
        e = torch.arange(Dm * Dm, dtype=torch.float64).reshape(1, Dm, Dm)
        self.U = torch.complex(g + 1e-3 * e, -1e-6 * e.expand(B, Dm, Dm))

    def run(self, out=None):
        if out is None:
            return self.U.clone()
        out.copy_(self.U)
        return out


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus, sys.argv[1:]))
    real_stdout = _claim_stdout()

    import numpy as np
    import torch

    from c3_amd import _lib, propagation, workloads
    from c3_amd import dist as c3dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    if args.gpus != world and rank == 0:
        print(f"[bench] --gpus {args.gpus} but the launcher started {world} rank(s): running {world}", file=sys.stderr, flush=True)
    if args.check is None:
        # default ON at every N: the line the driver records carries max_fro_err_vs_oracle next to the rate (BASELINE.json's
        # metric is "propagators/s ...; |U - U_ref|_F").  The check runs AFTER the timed region on a bounded spread of samples.
        args.check = True
    standin = os.environ.get("C3P_BENCH_STANDIN") == "1"  # test scaffold: CPU ranks over gloo, nothing computed (see _StandInPropagator)
    dist = None
    use_dist = world > 1 or ("RANK" in os.environ and "MASTER_ADDR" in os.environ)
    ndev = 0 if standin else torch.cuda.device_count()
    if not standin and ndev <= 0:
        _lib.require_gpu()  # raises: the propagator path has no CPU fallback
    oversubscribed = (not standin) and local_world > ndev
    backend = args.backend
    if backend == "auto":
        # RCCL refuses two ranks on one device ("Duplicate GPU detected"): ranks that share a device exchange over gloo,
        # staged through host memory -- an execution of the N > 1 path, not a measurement of it
        backend = "gloo" if (standin or oversubscribed) else "nccl"
    dev = torch.device("cpu") if standin else torch.device("cuda", local_rank % ndev)
    if not standin:
        torch.cuda.set_device(dev)
    if use_dist:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        rdzv = os.environ.get("C3P_BENCH_RDZV_FILE")  # self-launched ranks: file store, no port race (see self_launch)
        kw = {"init_method": f"file://{rdzv}"} if rdzv else {}
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, **kw)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world, **kw)
        if rank == 0:
            print(f"[bench] {'RCCL' if backend == 'nccl' else 'gloo'} world size {dist.get_world_size()} (backend {dist.get_backend()}{', ranks share devices' if oversubscribed else ''})", file=sys.stderr, flush=True)
    red_dev = dev if backend == "nccl" else torch.device("cpu")  # where the scalar reductions of this file live
    sync = (lambda: None) if standin else torch.cuda.synchronize

    def reduce_scalar(x, op):
        if not use_dist:
            return float(x)
        t = torch.tensor([float(x)], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=op)
        return float(t.item())

    cfg = workloads.CONFIGS[args.config]
    B_glob, lo, hi, b_pad = plan_batch(cfg, args.scaling, args.batch, world, rank)
    B = hi - lo  # this rank's samples
    wl = workloads.make_workload(args.config, B=max(B, 1), N=args.slices, b_offset=lo)
    if args.complex_ops:
        k = min(1, wl.K - 1)
        up = np.triu(wl.hks[k].real, 1)
        wl.hks = wl.hks.copy()
        wl.hks[k] = wl.hks[k] + 0.3j * (up - up.T)  # Hermitian, complex (a Y-type drive / rotating-frame operator)
        wl.name += " complex-Hamiltonian"
    Dm = wl.D * wl.D if wl.lindblad else wl.D
    fr = wl.fr_phase
    if wl.lindblad:
        fr = np.stack([(p[:, None] - p[None, :]).ravel() for p in wl.fr_phase])
    bp = None
    if B > 0 and standin:
        bp = _StandInPropagator(torch, lo, B, Dm)
    elif B > 0:
        bp = propagation.BatchPropagator(
            torch.as_tensor(wl.h0, device=dev),
            torch.as_tensor(wl.hks, device=dev),
            torch.as_tensor(wl.signals, device=dev),
            wl.dt,
            col_ops=torch.as_tensor(wl.col_ops, device=dev) if wl.lindblad else None,
            fr_phase=torch.as_tensor(fr, device=dev),
            force_generic=args.generic,
        )
    # The only data-path collective is the all-gather of the U slabs (RCCL over xGMI), in stream order, G steps per
    # collective.  (An asynchronous gather beside the chain kernel -- SlabRing(overlap=True), --overlap-gather -- is SLOWER at
    # one rank: the RCCL kernel takes CUs away from a grid sized to fill the chip exactly; it is timed beside the default as
    # `all_gather_every_step_overlapped`, because on N > 1 ranks it is the schedule that hides the link latency.)
    if args.exchange == "goal" and wl.lindblad:
        raise SystemExit("--exchange goal: unitary configurations only")
    if standin:
        args.no_e2e = args.no_cpu_baseline = True
    goal_state = {}
    last_step = {}  # what the most recent timed step returned (--dump-outputs)

    def make_schedule(exchange, gather_every, overlap=False):
        """(ring, compute) of one exchange schedule: `gather` = all-gather of the U slabs of `gather_every` steps in one
        collective (overlap: issued asynchronously while the next steps compute into a second bank of slabs); `goal` = fused
        fidelity per sample + ONE all-reduce of the goal per step, nothing gathered."""
        ring = c3dist.SlabRing(B, b_pad, (Dm, Dm), gather_every, device=dev, use_dist=use_dist and exchange == "gather", overlap=overlap,
                                stage_host=(backend == "gloo" and dev.type == "cuda"))
        if exchange == "goal":
            from c3_amd import fidelities

            comp_index = list(range(len(wl.dims)))
            ideal = torch.eye(2 ** len(wl.dims), dtype=torch.complex128, device=dev)
            goal_buf = torch.zeros(2, dtype=torch.float64, device=dev)  # {sum of infidelities, samples}

        def compute(out):
            if bp is not None:
                bp.run(out=out[:B])
            if exchange == "goal":
                # the optimiser loop of SURVEY 8e/8f-1: B infidelities per rank instead of B propagators, one all-reduce
                # of the goal per step (optimalcontrol_robust.py:49-70 averages them) -- no gather at all
                g = goal_buf
                if bp is not None:
                    g = fidelities.infid_sum(ideal, out[:B], comp_index, list(wl.dims), kind="unitary")["sum"]  # {sum, B}: one launch
                else:
                    goal_buf.zero_()
                if use_dist and g.device != red_dev:  # ranks sharing a device (gloo): the two goal scalars travel through the host
                    gh = g.to(red_dev)
                    dist.all_reduce(gh, op=dist.ReduceOp.SUM)
                    g = gh
                elif use_dist:
                    dist.all_reduce(g, op=dist.ReduceOp.SUM)
                goal_state["last"] = g

        return ring, compute

    def time_schedule(ring, compute, steps, warmup):
        """W untimed warmup steps, then exactly K steps between barrier + synchronize on both sides; returns (wall seconds,
        MAX over ranks; device ms per step by HIP events on the launch stream)."""
        G_ = ring.G
        ring.warm({min(G_, max(1, steps)), steps % G_, warmup % G_, min(G_, max(1, warmup))})  # communicator + every message size
        for _ in range(warmup):
            ring.step(compute)
        ring.drain()
        sync()
        if use_dist:
            dist.barrier()
        sync()
        ev0 = ev1 = None
        if dev.type == "cuda":
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        if ev0 is not None:
            ev0.record()  # HIP events on the stream the kernels are launched on (torch's current stream), over the timed region
        for _ in range(steps):
            last = ring.step(compute)
        if ev1 is not None:
            ev1.record()
        ring.drain()
        sync()
        last_step["U"] = last[:B]
        # The K steps end here on this rank (the last all-gather inside drain() has already waited for every rank's
        # slabs); the closing barrier follows and the MAX over ranks of the per-rank times is reported, so the
        # barrier's own latency is not booked as step time.
        el_rank = time.perf_counter() - t0
        if use_dist:
            dist.barrier()
        sync()
        dev_ms = (ev0.elapsed_time(ev1) if ev0 is not None else el_rank * 1e3) / max(1, steps)
        el = reduce_scalar(el_rank, dist.ReduceOp.MAX) if use_dist else el_rank
        el_min = reduce_scalar(el_rank, dist.ReduceOp.MIN) if use_dist else el_rank
        return el, dev_ms, el_min

    goal_mode = args.exchange == "goal"
    sync()
    # Untimed clock ramp: the MI355X needs tens of milliseconds of sustained work to reach its steady clocks
    # (measured: 0.210 ms per cfg2 batch after 5 warmup batches, 0.194 ms after 300).  The metric is sustained
    # throughput, so the device is brought to steady state before anything is calibrated or timed.
    if args.ramp_ms > 0 and bp is not None:
        scratch = torch.zeros((max(B, 1), Dm, Dm), dtype=torch.complex128, device=dev)
        t_r = time.perf_counter()
        while (time.perf_counter() - t_r) * 1e3 < args.ramp_ms:
            for _ in range(16):
                bp.run(out=scratch[:B])
            sync()
        del scratch
    # Which form of "ONE all-gather of U per batch" is timed: in stream order behind the kernel, or asynchronous under the next
    # batch's kernel (two banks of slabs).  Which one is faster depends on the node: under a chain kernel whose grid fills the
    # chip exactly the RCCL kernel takes CUs away (one rank: 13 % slower), across N ranks it hides the link latency.  `auto`
    # measures both untimed and takes the faster -- every rank takes the same decision (MAX over ranks of each time).
    overlap_choice = {"mode": args.overlap_gather}
    use_overlap = args.overlap_gather == "on"
    if args.overlap_gather == "auto":
        use_overlap = False
        if use_dist and world > 1 and args.exchange == "gather" and (backend == "nccl" or standin):
            cal = {}
            for name_, ov_ in (("in_stream_order", False), ("overlapped", True)):
                r_, c_ = make_schedule("gather", args.gather_every, ov_)
                cal[name_] = time_schedule(r_, c_, max(8, args.warmup), 2)[0] / max(8, args.warmup) * 1e3
                del r_, c_
            use_overlap = cal["overlapped"] < cal["in_stream_order"]
            overlap_choice.update(calibration_ms_per_step=cal, chosen="overlapped" if use_overlap else "in_stream_order")
    args.overlap_gather = use_overlap
    ring, compute = make_schedule(args.exchange, args.gather_every, args.overlap_gather)
    G = ring.G
    if not standin:
        _lib.load()
    sync()
    elapsed, device_ms_per_step, elapsed_min = time_schedule(ring, compute, args.steps, args.warmup)
    goal_last = [goal_state.get("last")]
    dumped = None
    if args.dump_outputs:
        # before anything else runs on the device: the slot of the last step is reused by the check below
        dumped = dump_outputs(args.dump_outputs, last_step["U"], goal_last[0] if goal_mode else None, rank, world, lo)
    # The other exchange schedules, timed the same way right after the headline one and reported as extra keys of the
    # SAME line (multi-GPU runs only): the amortised all-gather (32 steps per collective) and the gather-free goal
    # exchange (fused fidelity + one all-reduce per step; unitary configurations).
    alt = {}
    if use_dist and not args.no_alt_schedules:
        todo = []
        if not (args.exchange == "gather" and G == 32):
            todo.append(("all_gather_every_32_steps", "gather", 32))
        if not (args.exchange == "gather" and G == 1 and not args.overlap_gather):
            todo.append(("all_gather_every_step", "gather", 1))
        if not wl.lindblad and args.exchange != "goal" and not standin:
            todo.append(("goal_all_reduce_every_step", "goal", 1))
        todo = [(n_, e_, g_, False) for n_, e_, g_ in todo]
        if not (args.exchange == "gather" and G == 1 and args.overlap_gather):
            # the north_star schedule with the collective of step k under the kernel of step k + 1 (two banks of slabs,
            # asynchronous all-gather): at one rank the RCCL kernel only takes CUs from a grid sized to the chip (measured slower),
            # on N > 1 ranks it hides the xGMI latency -- timed beside the default so that the first real curve can tell
            todo.append(("all_gather_every_step_overlapped", "gather", 1, True))
        for name, ex, ge, ov in todo:
            r2, c2 = make_schedule(ex, ge, ov)
            el2, dms2, el2_min = time_schedule(r2, c2, args.steps, args.warmup)
            alt[name] = {"value": B_glob * args.steps / el2, "ms_per_step": el2 / args.steps * 1e3, "ms_per_step_fastest_rank": el2_min / args.steps * 1e3,
                         "device_ms_per_step": dms2, "collectives": r2.collectives}
            del r2, c2
    kernel_name = "TEST STAND-IN" if standin else _lib.last_kernel()

    err = None
    nchk = 0
    gathered_checked = 0
    if args.check:
        # (1) a spread of samples of this rank's shard against the oracle (bounded by the oracle's cost); a rank with an
        # empty shard (strong scaling of a batch smaller than the world) still takes part in every collective below.
        # (2) N > 1: after one more gathered step, this rank's slab as RECEIVED must equal what it computed, and one sample
        # of every OTHER rank's received slab is checked against the oracle on that sample's inputs (the synthetic inputs are
        # seeded per global sample index, so any rank can rebuild them).
        err = 0.0

        def reference(w, idx):
            from oracle import c3_oracle  # the CPU restatement: checker only, after the timed region

            return c3_oracle.propagate_batch(w.h0, w.hks, w.signals[idx], w.dt, col_ops=w.col_ops, lindbladian=w.lindblad, fr_phase=w.fr_phase[idx])

        if standin:
            def reference(w, idx, lo_=lo):  # noqa: F811  (the stand-in's own formula: nothing is computed in that mode)
                return _StandInPropagator(torch, lo_, len(w.signals), Dm).U.numpy()[idx]

        if bp is not None:
            cost = wl.N * (Dm / 9.0) ** 3
            # cfg2: 32 spread samples (~0.15 s of oracle); the large configurations 2 - 4 (full-size parity: tests/test_gpu_*.py)
            nchk = int(min(B, max(2, min(32, 2.5e5 / cost))))
            idx = np.unique(np.linspace(0, B - 1, nchk).astype(int))
            U = bp.run()
            sync()
            ref = reference(wl, idx)
            Uh = U[torch.as_tensor(idx, device=dev)].cpu().numpy()
            err = float(max(np.linalg.norm(Uh[i] - ref[i]) for i in range(len(idx))))
            nchk = len(idx)
        if use_dist:
            if args.exchange == "gather":
                ring.step(compute)
                ring.drain()
                sync()
                if bp is not None:
                    mine = ring.gathered_slab(rank, 0)[:B]
                    assert torch.equal(mine, ring.sent_slab(0)[:B]), "all-gather mismatch"
                for q in range(world):
                    if q == rank:
                        continue
                    _, lo_q, hi_q, _ = plan_batch(cfg, args.scaling, args.batch, world, q)
                    if hi_q <= lo_q:
                        continue
                    j = (rank + 7 * q) % (hi_q - lo_q)  # a different sample of rank q's shard on every checking rank
                    got = ring.gathered_slab(q, 0)[j].cpu().numpy()
                    if standin:
                        want = _StandInPropagator(torch, lo_q + j, 1, Dm).U.numpy()[0]
                    else:
                        wq = workloads.make_workload(args.config, B=1, N=args.slices, b_offset=lo_q + j)
                        if args.complex_ops:
                            wq.hks = wl.hks
                        want = reference(wq, np.array([0]))[0]
                    err = max(err, float(np.linalg.norm(got - want)))
                    gathered_checked += 1
            err = reduce_scalar(err, dist.ReduceOp.MAX)
            nchk = int(reduce_scalar(nchk, dist.ReduceOp.SUM))
            gathered_checked = int(reduce_scalar(gathered_checked, dist.ReduceOp.SUM))
        if err > 1e-10:
            print(f"[bench] CHECK FAILED: max |U - U_ref|_F = {err:.3e}", file=sys.stderr, flush=True)

    if rank == 0:
        total_props = B_glob * args.steps
        value = total_props / elapsed
        f_prop = algorithmic_flops_per_prop(wl)
        t_step = device_ms_per_step * 1e-3
        achieved_alg = f_prop * B / t_step / 1e12
        # What the hardware did (PMC, profiles/<round>/pmc.json, taken on this bench command by tools/profile_r03.sh):
        #   issued  = MFMA flops (SQ_INSTS_VALU_MFMA_MOPS_F64 x 512) + fp64 VALU flops, all lanes, padding included
        #   useful  = MFMA flops x the fraction of each MFMA tile that holds matrix data (zero padding excluded) + VALU flops
        # per sample and slice, so other batch sizes / slice counts of the same configuration are scaled, flagged inexact.
        traffic = issued = useful = None
        pmc_exact = False
        pfile = os.path.join(ROOT, "profiles", PROFILE_ROUND, "pmc.json")
        digest = kernel_sources_digest(args.config)
        ent = {}
        if os.path.exists(pfile) and not args.generic:
            try:
                ent = json.load(open(pfile)).get(f"cfg{args.config}{'_complex' if args.complex_ops else ''}", {})
            except Exception:
                ent = {}
        # The hardware figures are quoted ONLY for the exact build, batch and slice count that was profiled: nothing is
        # scaled from another run and nothing is clamped (a stale profile must not pass as a measurement of this build).
        if ent.get("issued_flop_per_launch") and ent.get("kernel_sources_digest") == digest and ent.get("batch") == B and ent.get("slices") == wl.N:
            pmc_exact = True
            issued = ent["issued_flop_per_launch"]
            useful = ent.get("useful_flop_per_launch", issued)
            traffic = ent.get("hbm_bytes_per_launch")
        if useful is not None:
            achieved = useful / t_step / 1e12
            frac = achieved / PEAK_FP64_TFLOPS
            frac_source = "useful issued flops (PMC: MFMA flops x tile utilisation + fp64 VALU flops)"
        else:
            achieved = frac = None
            frac_source = "no PMC profile of this build / batch / slice count: only frac_algorithmic is reported"
        out = {
            "metric": "full-gate propagators/s",
            "value": value,
            "unit": "propagators/s",
            "n_gpus": world,
            "n_devices_visible": ndev,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "c128",
            "data": "synthetic",
            "config": {
                "workload": wl.name if world == 1 else f"{wl.name} per rank 0 shard; global batch {B_glob}",
                "D": wl.D,
                "matrix_dim": Dm,
                "slices": wl.N,
                "controls": wl.K,
                "batch_per_gpu": B,
                "global_batch": B_glob,
                "baseline_batch": f"{cfg['B']} on {cfg.get('gpus', 1)} GPU(s)",
                "clock_ramp_ms": args.ramp_ms,
                "throughput": f"sustained: after a {args.ramp_ms:g} ms untimed clock ramp and {args.warmup} warmup steps",
                "parallelism": ((f"dp{world} ({args.scaling}: batch sharded; " + ("one RCCL all-gather of U per step" if G == 1 else f"one RCCL all-gather of U per {G} steps") + (", issued asynchronously under the next step" if args.overlap_gather else "") + ")" if args.exchange == "gather" else f"dp{world} ({args.scaling}: batch sharded; fused fidelity, one RCCL all-reduce of the goal per step, no gather)") if use_dist else ("single GPU" if args.exchange == "gather" else "single GPU, fused fidelity per step")),
                # (N > 1 with --overlap-gather auto: the timed schedule is the faster of two forms of the one-gather-per-step
                # exchange, picked by an untimed calibration -- named HERE, not only under launch.gather_overlap)
                "exchange": args.exchange if not (use_dist and args.exchange == "gather") else f"gather ({'overlapped' if args.overlap_gather else 'in_stream_order'}{', picked by calibration' if overlap_choice.get('chosen') else ''})",
                "kernel": kernel_name,
            },
            "roofline": {
                "bound": "mfma",
                "achieved": achieved,
                "peak": PEAK_FP64_TFLOPS,
                "unit": "TFLOP/s",
                "frac": frac,
                "frac_source": frac_source,
                "traffic": traffic,
                "achieved_algorithmic": achieved_alg,
                "frac_algorithmic": achieved_alg / PEAK_FP64_TFLOPS,
                "algorithmic_flop_per_launch": f_prop * B,
                "algorithmic_flop_per_propagator": f_prop,
                "issued_flop_per_launch": issued,
                "issued_frac": None if issued is None else issued / t_step / 1e12 / PEAK_FP64_TFLOPS,
                "useful_flop_per_launch": useful,
                "mfma_tile_utilisation": ent.get("mfma_tile_utilisation"),
                "pmc_profile": f"profiles/{PROFILE_ROUND}/pmc.json" if pmc_exact else None,
                "pmc_exact_match": pmc_exact,
                "pmc_avg_launch_us": ent.get("avg_launch_us") if pmc_exact else None,
                "pmc_median_launch_us": ent.get("median_launch_us") if pmc_exact else None,
                "issue_busy_model": ent.get("issue_busy_model") if pmc_exact else None,
                "kernel": f"chain kernel ({kernel_name})",
                "device_ms_per_step": device_ms_per_step,
                "note": "fp64 compute-bound path. frac = USEFUL issued flops / device time per step (HIP events over the timed region, launch gaps included) / dense fp64 peak: flops the kernel really issues (PMC) with the zero padding of its MFMA tiles taken out; null unless the committed PMC profile is of exactly this kernel build, batch and slice count (pmc_exact_match). frac_algorithmic = SURVEY 8d's figure (the reference's complex Pade order per slice + product tree) over the same time: a method that needs fewer flops than the reference's (real cos / sin evaluation of real Hamiltonians; Lindblad chains in real arithmetic in the Hermitian basis) exceeds the hardware fraction there and can exceed 1; it is an algorithm credit, not a hardware one. traffic = HBM-side bytes per launch from the same PMC passes",
            },
        }
        if use_dist:
            out["launch"] = {
                "launcher": "bench.py self-launch (one child process per rank)" if os.environ.get("C3P_BENCH_SELF_LAUNCHED") == "1" else "external (torch.distributed.run / RANK, WORLD_SIZE from the environment)",
                "backend": dist.get_backend(),
                "rccl_world_size" if backend == "nccl" else "gloo_world_size": dist.get_world_size(),
                "oversubscribed": bool(oversubscribed),
                "ms_per_step_slowest_rank": elapsed / args.steps * 1e3,
                "ms_per_step_fastest_rank": elapsed_min / args.steps * 1e3,
                "collectives_per_timed_region": -(-args.steps // G),
                "gather_overlap": overlap_choice,
            }
            if oversubscribed:
                out["launch"]["note"] = (f"{world} ranks on {ndev} visible device(s): RCCL refuses ranks that share a device (Duplicate GPU detected), so the slabs travel over gloo through host "
                                         "memory and the ranks time-slice the device -- an execution of the N > 1 path (sharding, exchange schedules, gathered check), NOT a scaling measurement")
        if standin:
            out["metric"] = "TEST STAND-IN (nothing computed; launcher / exchange plumbing only)"
            out["data"] = "stand-in"
        if alt:
            out["other_exchange_schedules"] = dict(alt, note="same steps / warmup, timed right after the headline schedule in the same process; value = whole-job propagators/s")
        if goal_mode and goal_last[0] is not None:
            g = goal_last[0].cpu().numpy()
            out["goal"] = {"mean_unitary_infidelity_vs_identity": float(g[0] / max(g[1], 1.0)), "samples": int(g[1])}
        if dumped is not None:
            out["dumped_outputs"] = dumped
        if err is not None:
            out["max_fro_err_vs_oracle"] = err
            out["oracle_samples_checked"] = nchk
            out["gathered_samples_of_other_ranks_checked"] = gathered_checked
        if world == 1 and not args.no_e2e and bp is not None:
            t_e = time.perf_counter()
            out["e2e"] = e2e_rates(wl, fr, propagation, torch, dev)
            out["e2e"]["wall_s"] = time.perf_counter() - t_e
        if world == 1 and not args.no_e2e and bp is not None:
            # the step after the path in every optimiser: goal + gradient of the whole batch -- an extra key, never `value`
            try:
                out["optimiser_evaluation"] = evaluation_rates(args.config, wl, fr, propagation, torch, dev, elapsed / args.steps * 1e3)
            except Exception as e:  # noqa: BLE001  (a side measurement must not cost the headline line)
                out["optimiser_evaluation"] = {"error": str(e)[:200]}
        if world == 1 and not args.no_cpu_baseline:
            from oracle import c3_oracle  # the CPU restatement, timed beside the GPU path (checker only)

            out["cpu_baseline"] = cpu_baseline(wl, c3_oracle)
            out["cpu_baseline_allcores"] = cpu_baseline_allcores(args.config, wl)
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if use_dist:
        dist.destroy_process_group()
    if err is not None and err > 1e-10:
        sys.exit(3)


def evaluation_rates(cfg, wl, fr, propagation, torch, dev, forward_ms, reps=5):
    """One optimiser evaluation of this batch on resident control samples: goal (infidelity against an identity gate on the
    qubit subspace) AND its gradient w.r.t. every control sample.  Closed systems: c3p_pwc_unitary_goal_vjp, one pass over the
    chains (optimalcontrol.py:200-228 under optimizer.py:206-216); open systems (D = 7, 8, 9): taped forward pass + vjp from the
    tape.  ms per evaluation, median of `reps`."""
    import numpy as np

    from c3_amd import fidelities, workloads

    dims = list(workloads.CONFIGS[cfg]["dims"])
    index = list(range(len(dims)))
    ideal = torch.eye(2 ** len(dims), dtype=torch.complex128, device=dev)
    t = lambda a: torch.as_tensor(a, device=dev)
    h0, hks, sig, ph = t(wl.h0), t(wl.hks), t(wl.signals), t(fr)
    if wl.lindblad:
        if not propagation.lindblad_tape_supported(wl.B, wl.K, wl.N, wl.D):
            return {"skipped": "no taped open-system evaluation for this shape"}
        col = t(wl.col_ops)

        def run():
            r = propagation.propagate_batch_lindblad_taped(h0, hks, sig, wl.dt, col, fr_phase=ph)
            S_bar, goal = fidelities.lindbladian_unitary_infid_cotangent(ideal, r["U"], index, dims)
            return goal, r["tape"].vjp(S_bar)

        how = "c3p_pwc_lindblad_taped + lindbladian_unitary_infid cotangent + c3p_pwc_lindblad_vjp_taped"
    else:
        if not propagation.goal_vjp_is_fused(wl.B, wl.D):
            return {"skipped": "no fused goal entry for this shape"}

        def run():
            r = propagation.propagate_batch_goal_vjp(h0, hks, sig, wl.dt, ideal, index, dims, fr_phase=ph, want_U=False)
            return r["goal"], r["grad_signals"]

        how = "c3p_pwc_unitary_goal_vjp (unitary_infid)"
    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        goal, grad = run()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ms_single = 1e3 * float(np.median(ts))
    # like `ms_per_step` of the forward path: evaluations enqueued back to back, ONE synchronisation around the timed region
    # (bounded to ~0.3 s of device time)
    n = int(max(3, min(50, 300.0 / max(ms_single, 1e-3))))
    rates = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            goal, grad = run()
        torch.cuda.synchronize()
        rates.append((time.perf_counter() - t0) / n)
    ms = 1e3 * float(np.median(rates))
    return {"ms_per_evaluation": ms, "evaluations_per_s": 1e3 / ms, "gradients_per_s": 1e3 * wl.B / ms, "x_forward": ms / forward_ms, "how": how,
            "timing": f"median of 3 runs of {n} evaluations enqueued back to back, one synchronisation per run (as ms_per_step)",
            "ms_single_call_synchronised": ms_single, "mean_goal": float(goal.mean()), "grad_abs_max": float(grad.abs().max()),
            "note": "goal + d goal / d every control sample of the batch, inputs resident; tests/perf/bench_goal_run.py times the whole loop body with signal synthesis"}


def e2e_rates(wl, fr, propagation, torch, dev, reps=3):
    """PCIe-inclusive rates (never the reported `value`), two boundaries:
      host samples    numpy arrays in host memory -> C ABI (C3P_HOST_PTRS: H2D of the control samples, kernel, D2H of U)
      parameter rows  SURVEY 8f-2's boundary: envelope parameter rows + carriers in (a few KB), control samples synthesised ON
                      THE DEVICE (c3p_synth_signals), chains, D2H of U -- what a caller that owns pulse parameters pays."""
    import numpy as np

    from c3_amd import signals as sg

    def host():
        propagation.propagate_batch(wl.h0, wl.hks, wl.signals, wl.dt, col_ops=wl.col_ops, lindbladian=wl.lindblad, fr_phase=fr)

    host()
    t0 = time.perf_counter()
    for _ in range(reps):
        host()
    t = (time.perf_counter() - t0) / reps
    Dm = wl.D * wl.D if wl.lindblad else wl.D
    out = {
        "host_in_out_props_per_s": wl.B / t,
        "host_in_out_ms_per_batch": t * 1e3,
        "bytes_in": int(wl.signals.nbytes),
        "bytes_out": int(wl.B * Dm * Dm * 16),
        "note": "host samples: numpy arrays in host memory -> C ABI (C3P_HOST_PTRS: H2D of the control samples, kernel, D2H of U, synchronous)",
    }
    try:
        T = wl.N * wl.dt
        two_pi = 2.0 * np.pi
        rng = np.random.default_rng(5)
        chans = [[dict(shape="gaussian_nonorm", amp=rng.uniform(0.1, 0.6, wl.B), xy_angle=0.1 * k, freq_offset=-50e6 * two_pi, t_final=T, sigma=T / 4, use_t_before=True)]
                 for k in range(wl.K)]
        env, shapes = sg.pack_components(chans, B=wl.B)
        car = np.tile(np.array([[(5.0e9 + 0.3e9 * k) * two_pi, 1e9 * two_pi] for k in range(wl.K)]), (wl.B, 1, 1))
        t_ = lambda a: torch.as_tensor(a, device=dev)
        h0, hks, ph = t_(wl.h0), t_(wl.hks), t_(fr)
        col = t_(wl.col_ops) if wl.lindblad else None
        sim_res = 1.0 / wl.dt

        def rows():
            sig = sg.synthesize_signals(t_(env), shapes, t_(car), 0.0, T, sim_res / 50.0, sim_res)
            if tuple(sig.shape) != (wl.B, wl.K, wl.N):
                raise RuntimeError(f"synthesised {tuple(sig.shape)}, wanted {(wl.B, wl.K, wl.N)}")
            return propagation.propagate_batch(h0, hks, sig, wl.dt, col_ops=col, lindbladian=wl.lindblad, fr_phase=ph)["U"].cpu()

        rows()
        t0 = time.perf_counter()
        for _ in range(reps):
            rows()
        tr = (time.perf_counter() - t0) / reps
        out["parameter_rows"] = {
            "props_per_s": wl.B / tr,
            "ms_per_batch": tr * 1e3,
            "bytes_in": int(env.nbytes + car.nbytes),
            "bytes_out": int(wl.B * Dm * Dm * 16),
            "note": "envelope parameter rows + carriers H2D, control samples synthesised on the device (c3p_synth_signals: gaussian envelopes, AWG sampling at 1/50 of the slice rate, IQ mixing), chain kernel, D2H of U, synchronous",
        }
    except Exception as e:  # noqa: BLE001  (a side measurement must not cost the headline line)
        out["parameter_rows"] = {"error": str(e)[:200]}
    return out


def _oracle_run(wl, oracle, nb):
    t0 = time.perf_counter()
    oracle.propagate_batch(wl.h0, wl.hks, wl.signals[:nb], wl.dt, col_ops=wl.col_ops, lindbladian=wl.lindblad, fr_phase=wl.fr_phase[:nb])
    return time.perf_counter() - t0


def cpu_baseline(wl, oracle, budget_s=8.0):
    """The numpy oracle (reference algorithm: batched per-slice Pade expm + pairwise tree product) timed single-threaded on
    a bounded sample of the same workload: one untimed sample (imports, LAPACK warm-up), then up to three timed repeats of
    `nb` samples inside `budget_s` seconds; the MEDIAN repeat is reported."""
    try:
        from threadpoolctl import threadpool_limits
    except Exception:  # pragma: no cover
        threadpool_limits = None

    t_leg = time.perf_counter()
    ctx = threadpool_limits(limits=1) if threadpool_limits else None
    try:
        if ctx is not None:
            ctx.__enter__()
        _oracle_run(wl, oracle, 1)  # untimed
        t1 = _oracle_run(wl, oracle, 1)
        nb = int(max(1, min(wl.B, (budget_s / 3.0) / max(t1, 1e-4))))
        times = []
        while len(times) < 3 and (not times or time.perf_counter() - t_leg + times[-1] < budget_s):
            times.append(_oracle_run(wl, oracle, nb))
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    t = sorted(times)[len(times) // 2]
    return {
        "value": nb / t,
        "unit": "propagators/s",
        "cores": 1,
        "kind": "port",
        "repeats": len(times),
        "rates_of_the_repeats": [nb / x for x in times],
        "wall_s": time.perf_counter() - t_leg,
        "sample": f"{nb} of {wl.B} samples of {wl.name}, numpy oracle (Higham Pade expm per slice + tf_matmul_n tree), 1 thread, median of {len(times)} repeats after one untimed sample; {os.cpu_count()} host cores present",
    }


def _pool_init():
    os.environ["OMP_NUM_THREADS"] = os.environ["OPENBLAS_NUM_THREADS"] = os.environ["MKL_NUM_THREADS"] = "1"
    import numpy  # noqa: F401

    from oracle import c3_oracle  # noqa: F401
    from c3_amd import workloads  # noqa: F401


def _pool_work(job):
    cfg, N, b0, nb = job
    from c3_amd.workloads import make_workload
    from oracle import c3_oracle as o

    if nb == 0:
        return 0.0
    w = make_workload(cfg, B=nb, N=N, b_offset=b0)
    t0 = time.perf_counter()
    o.propagate_batch(w.h0, w.hks, w.signals, w.dt, col_ops=w.col_ops, lindbladian=w.lindblad, fr_phase=w.fr_phase)
    return time.perf_counter() - t0


def effective_cores():
    """(usable hardware threads, how that was determined): the scheduler affinity mask and the cgroup CPU quota of the
    lease, not os.cpu_count() (a container may see 256 threads and be allowed a handful)."""
    n = os.cpu_count() or 1
    how = [f"os.cpu_count()={n}"]
    try:
        aff = len(os.sched_getaffinity(0))
        how.append(f"sched_getaffinity={aff}")
        n = min(n, aff)
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    q = float(txt[0]) / float(txt[1])
                    how.append(f"cgroup cpu.max={q:.1f}")
                    n = max(1, min(n, int(q + 0.999)))
                else:
                    how.append("cgroup cpu.max=max")
            else:
                q = float(txt[0])
                if q > 0:
                    per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    how.append(f"cgroup cfs quota={q / per:.1f}")
                    n = max(1, min(n, int(q / per + 0.999)))
            break
        except Exception:
            continue
    return n, ", ".join(how)


def cpu_baseline_allcores(cfg_index, wl, budget_s=20.0):
    """The same oracle process-parallel over samples, with a persistent worker pool (workers started and warmed --
    imports, one sample each -- BEFORE anything is timed).  The worker count is swept in powers of two up to the usable
    hardware threads (at most 32 workers); every count is timed THREE times and its MEDIAN rate reported; `value` is the
    best median and `cores` the worker count that gave it.  The whole leg is bounded by `budget_s` seconds of wall clock:
    the per-worker sample shrinks to fit, and the sweep stops (lowest counts first dropped) if the budget runs out."""
    import multiprocessing as mp

    t_leg = time.perf_counter()
    cores, how = effective_cores()
    workers = min(cores, 32)
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except Exception:
        pass
    ctx = mp.get_context("spawn")  # the parent holds a HIP context: no fork
    sweep, raw = {}, {}
    with ctx.Pool(workers, initializer=_pool_init) as pool:
        warm = pool.map(_pool_work, [(cfg_index, wl.N, 0, 1)] * workers)  # untimed: start-up + one sample per worker
        t_start = time.perf_counter() - t_leg
        t1 = sorted(warm)[len(warm) // 2]
        counts = []
        w = 1
        while w < workers:
            counts.append(w)
            w *= 2
        counts.append(workers)
        left = max(2.0, budget_s - t_start)
        # 3 repeats x len(counts) timed maps inside what is left of the budget
        per = int(max(1, min(64, (left / (3.0 * len(counts))) / max(t1, 1e-4))))
        for w in reversed(counts):  # the full width first: it is the one that matters if the budget runs out
            if time.perf_counter() - t_leg > budget_s and sweep:
                break
            rates = []
            for _ in range(3):
                t0 = time.perf_counter()
                pool.map(_pool_work, [(cfg_index, wl.N, i * per, per) for i in range(w)], chunksize=1)
                rates.append(w * per / (time.perf_counter() - t0))
                if time.perf_counter() - t_leg > budget_s:
                    break
            raw[w] = rates
            sweep[w] = sorted(rates)[len(rates) // 2]
    best = max(sweep, key=sweep.get)
    return {
        "value": sweep[best],
        "unit": "propagators/s",
        "cores": best,
        "usable_hardware_threads": cores,
        "how_counted": how,
        "kind": "port",
        "cpu_model": model,
        "rate_by_workers": {str(k): sweep[k] for k in sorted(sweep)},
        "repeats_by_workers": {str(k): raw[k] for k in sorted(raw)},
        "scaling_1_to_8_workers": (sweep[8] / sweep[1]) if (8 in sweep and 1 in sweep) else None,
        "pool_start_s": t_start,
        "wall_s": time.perf_counter() - t_leg,
        "sample": f"{per} samples of {wl.name.rsplit(' B=', 1)[0]} per worker, numpy oracle, one single-threaded process per worker, persistent pool (start-up and a warm-up sample excluded), worker counts {sorted(sweep)}, median of up to 3 repeats each; value = the best median; leg bounded to {budget_s:g} s",
    }


if __name__ == "__main__":
    main()
