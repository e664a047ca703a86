"""Flagship benchmark: MatrixTable Add+Get updates/sec (whole node).

BASELINE.json headline metric on the named config "MatrixTable 1e6x128
dense SGD updater, N workers on N x MI355X": every worker performs, per
step, one whole-table Add (its own 1e6x128 fp32 delta; reduce-scatter over
xGMI + fused SGD updater kernel on the owned shard) and one whole-table
Get (all-gather of shards into its buffer). Synthetic random deltas,
random-init weights. ``value`` is the whole-job aggregate: element-updates
applied per second = N_workers * rows * cols / step_time.

Launch: python bench.py --gpus N --steps K --warmup W
(N>1 via torch.distributed.run; reads RANK/WORLD_SIZE/MASTER_* from env.)

A plain run sets up, warms up, times the K steps and prints the result
line. ``--dump-outputs DIR`` additionally writes what the last timed step
returned (DIR/<name>.npy) so two builds can be compared output for output;
``--full`` adds the diagnostic measurements that take runs of their own
(the per-phase add/get/barrier split).
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch
import torch.distributed as dist


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    # default timed region ~1s on GPU (0.34 ms/step x 3000) so driver
    # gpu_busy sampling can corroborate activity
    p.add_argument("--steps", type=int, default=3000)
    p.add_argument("--warmup", type=int, default=100)
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--cols", type=int, default=128)
    p.add_argument("--updater", type=str, default="sgd")
    p.add_argument("--phase-steps", dest="phase_steps", type=int, default=20,
                   help="with --full: diagnostic per-phase (add/get/barrier) "
                        "timing steps run AFTER the contract region; "
                        "0 disables")
    p.add_argument("--full", action="store_true",
                   help="also run the diagnostics that take runs of their "
                        "own (per-phase timing); a plain run only times "
                        "the contract region")
    p.add_argument("--dump-outputs", dest="dump_outputs", type=str,
                   default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step returned as DIR/<name>.npy (float32; an array "
                        "over 32 MiB is cut to a fixed seeded row sample)")
    p.add_argument("--gb", type=float, default=4.0,
                   help="sweep mode: aggregate buffer size in GiB")
    p.add_argument("--app", type=str, default="matrix",
                   choices=["matrix", "wordembedding", "logreg", "sweep"])
    p.add_argument("--vocab", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=200)
    p.add_argument("--block-words", dest="block_words", type=int,
                   default=500_000)
    p.add_argument("--use-adagrad", dest="use_adagrad", action="store_true",
                   help="wordembedding: per-element AdaGrad mode")
    p.add_argument("--objective", type=str, default="sigmoid",
                   choices=["sigmoid", "softmax", "ftrl"],
                   help="logreg: objective (fused kernel per objective)")
    p.add_argument("--classes", type=int, default=10,
                   help="logreg softmax: number of classes")
    p.add_argument("--dense", action="store_true",
                   help="logreg: dense data mode (reference sparse=false "
                        "— GEMMs on the matrix cores via rocBLAS)")
    args = p.parse_args()
    if args.dump_outputs and args.app != "matrix":
        p.error("--dump-outputs is implemented for the flagship "
                "--app matrix run only")
    return args


DUMP_BUDGET_BYTES = 32 << 20   # all dumped arrays together (cap: 64 MB)
DUMP_SAMPLE_SEED = 0xD0A7


def dump_outputs(dirname, arrays):
    """Write each named 2-D tensor as ``dirname/<name>.npy`` (float32, or
    float64 for double tensors). The byte budget is split evenly; an
    array over its share is reduced to a fixed, seeded sample of its rows
    (sorted row order), identical from run to run and build to build."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(len(arrays), 1)
    for i, (name, t) in enumerate(sorted(arrays.items())):
        t = t.detach()
        dt = torch.float64 if t.dtype == torch.float64 else torch.float32
        rows = t.shape[0]
        row_bytes = max(t[0].numel(), 1) * (8 if dt == torch.float64 else 4)
        keep = share // row_bytes
        if rows > keep:
            g = torch.Generator(device="cpu").manual_seed(
                DUMP_SAMPLE_SEED + i)
            idx = torch.randperm(rows, generator=g)[:keep].sort().values
            t = t.index_select(0, idx.to(t.device))
        np.save(os.path.join(dirname, name + ".npy"),
                t.to(device="cpu", dtype=dt).contiguous().numpy())


def main():
    args = parse_args()
    cuda = torch.cuda.is_available()
    if not cuda:
        # CPU debug only — the driver always runs this on MI355X.
        args.rows = min(args.rows, 20_000)

    import multiverso_amd as mv
    if args.app == "wordembedding":
        from multiverso_amd.apps.wordembedding.bench import run_bench
        run_bench(args)
        return
    if args.app == "logreg":
        from multiverso_amd.apps.logreg.bench import run_bench
        run_bench(args)
        return
    if args.app == "sweep":
        run_sweep(args)
        return

    mv.init(sync=True)
    n = mv.size()
    rank = mv.rank()
    device = mv.Zoo.get().device

    table = mv.MatrixTable(args.rows, args.cols, updater_type=args.updater,
                           random_init=(-0.1, 0.1))
    if cuda:
        from multiverso_amd import ops
        ops.module(required=True)  # native kernels must be loaded

    gen = torch.Generator(device="cpu").manual_seed(1234 + rank)
    delta = (torch.rand(args.rows * args.cols, generator=gen) * 1e-4).to(device)
    out = torch.empty(args.rows, args.cols, dtype=torch.float32, device=device)

    def step():
        table.add(delta)        # reduce-scatter + fused SGD kernel
        table.get(out=out)      # all-gather into user buffer

    for _ in range(args.warmup):
        step()

    mv.barrier()
    if cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    if cuda:
        torch.cuda.synchronize()
    mv.barrier()
    elapsed = time.perf_counter() - t0

    # MAX over ranks
    t = torch.tensor([elapsed], dtype=torch.float64)
    if dist.is_initialized() and n > 1:
        if mv.Zoo.get().backend == "nccl":
            t = t.to(device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t[0])

    ms_per_step = elapsed / args.steps * 1e3
    updates_per_sec = n * args.rows * args.cols / (elapsed / args.steps)

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"get_out": out})

    # diagnostic per-phase breakdown AFTER the contract region (VERDICT
    # r1 #2: make the first 8-GPU run diagnosable — at N>1 add =
    # reduce-scatter + updater kernel, get = all-gather; a slow phase
    # points straight at the collective vs the kernel)
    phases = None
    if args.full and args.phase_steps > 0:
        def timed(fn):
            mv.barrier()
            if cuda:
                torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.phase_steps):
                fn()
            if cuda:
                torch.cuda.synchronize()
            dt = time.perf_counter() - t
            tt = torch.tensor([dt], dtype=torch.float64)
            if dist.is_initialized() and n > 1:
                if mv.Zoo.get().backend == "nccl":
                    tt = tt.to(device)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            return float(tt[0]) / args.phase_steps * 1e3

        phases = {
            "add_ms": timed(lambda: (table.add(delta), table.flush())),
            "get_ms": timed(lambda: table.get(out=out)),
            "barrier_ms": timed(mv.barrier),
        }

    if rank == 0:
        print(json.dumps({
            "metric": "MatrixTable Add+Get updates/sec (whole node)",
            "value": updates_per_sec,
            "unit": "updates/s",
            "n_gpus": n,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp32",
            "data": "synthetic",
            "config": {
                "model": f"MatrixTable {args.rows}x{args.cols} dense "
                         f"{args.updater} updater",
                "global_batch": n,
                "seq_len": None,
                "parallelism": f"ps-sharded dp{n} (reduce-scatter/all-gather "
                               "over xGMI)",
            },
            "phases": phases,
        }), flush=True)
    mv.shutdown()


def run_sweep(args):
    """BASELINE config 5: the 4 GB sync-SGD RCCL bucket sweep over xGMI
    (the reference AllreduceEngine's 4096-byte switch,
    allreduce_engine.cpp:35, as an empirically swept bucket size).
    Times MV_Aggregate at a ladder of bucket_mb values; rank 0 prints
    the full curve plus the contract JSON line for the best bucket."""
    import multiverso_amd as mv
    mv.init(sync=True)
    n = mv.size()
    rank = mv.rank()
    device = mv.Zoo.get().device
    cuda = device.type == "cuda"
    gb = args.gb if cuda else min(args.gb, 0.0625)
    numel = int(gb * (1 << 30) / 4)
    buf = torch.empty(numel, dtype=torch.float32, device=device)
    buf.uniform_(-1, 1)
    iters = max(args.steps // 1000, 3)
    curve = []
    for bucket_mb in [0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512]:
        for _ in range(2):   # warmup
            mv.aggregate(buf, bucket_mb=bucket_mb)
        mv.barrier()
        if cuda:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            mv.aggregate(buf, bucket_mb=bucket_mb)
        if cuda:
            torch.cuda.synchronize()
        mv.barrier()
        dt = (time.perf_counter() - t0) / iters
        t = torch.tensor([dt], dtype=torch.float64)
        if dist.is_initialized() and n > 1:
            if mv.Zoo.get().backend == "nccl":
                t = t.to(device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t[0])
        # all-reduce moves 2*(n-1)/n * bytes per GPU; report algo bw
        bus_gb = (numel * 4 / 1e9) * (2 * (n - 1) / n) / dt if n > 1 else 0
        curve.append({"bucket_mb": bucket_mb, "ms": dt * 1e3,
                      "bus_GBps_per_gpu": bus_gb})
        if rank == 0:
            print(f"# bucket_mb={bucket_mb:4d}  {dt * 1e3:8.2f} ms  "
                  f"{bus_gb:7.1f} GB/s", flush=True)
    best = min(curve, key=lambda c: c["ms"])
    if rank == 0:
        print(json.dumps({
            "metric": "MV_Aggregate 4GB all-reduce bus bandwidth",
            "value": best["bus_GBps_per_gpu"],
            "unit": "GB/s/gpu",
            "n_gpus": n, "steps": iters, "warmup": 2,
            "ms_per_step": best["ms"],
            "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "fp32", "data": "synthetic",
            "config": {"model": f"aggregate {gb} GiB fp32",
                       "global_batch": None, "seq_len": None,
                       "parallelism": f"allreduce dp{n} over xGMI",
                       "best_bucket_mb": best["bucket_mb"]},
            "sweep": curve,
        }), flush=True)
    mv.shutdown()


if __name__ == "__main__":
    main()
