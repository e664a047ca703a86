"""MatrixTable perf harness — the rebuild of Test/test_matrix_perf.cpp
(TestmatrixPerformance, :33-171): a 1e6x50 float matrix; sweeps adding
10%..100% of rows, times get-all before/after each sweep point, and
prints the Dashboard.

Run (CPU or GPU):  python tools/matrix_perf.py [--rows N] [--cols N]
                       [--updater momentum]   (times the keyed updater path)
                       [--wire-dtype bf16]    (bf16 payloads, fp32 shard)
Multi-rank:        python -m torch.distributed.run --nproc-per-node N \
                       --master-addr 127.0.0.1 tools/matrix_perf.py
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--cols", type=int, default=50)
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--sparse", action="store_true",
                   help="TestSparsePerf equivalent: SparseMatrixTable "
                        "stale-filtered get_into instead of dense get")
    p.add_argument("--updater", default="default",
                   choices=["default", "sgd", "momentum", "adagrad",
                            "dcasgd", "dcasgda", "adam"],
                   help="updater_type of the table; the keyed Adds carry a "
                        "matching AddOption")
    p.add_argument("--wire-dtype", default="fp32", choices=["fp32", "bf16"],
                   help="wire_dtype of the table: bf16 moves keyed values "
                        "and Get results as bfloat16 over the fp32 shard")
    p.add_argument("--repeat", type=int, default=1,
                   help="time each keyed Add this many times after one "
                        "untimed warm-up and print the median (1: a single "
                        "cold timing)")
    p.add_argument("--seed", type=int, default=None,
                   help="seed the row choice, to time the same ids twice")
    p.add_argument("--torch-composed", action="store_true",
                   help="with --updater momentum on one rank: replace the "
                        "keyed Add by its composition from torch ops "
                        "(unique + index_add_ + indexed formula) on the "
                        "table's own shard and state, as a baseline")
    args = p.parse_args()
    if args.torch_composed and (args.updater != "momentum" or args.sparse):
        p.error("--torch-composed needs --updater momentum without --sparse")
    if args.wire_dtype == "bf16" and (args.sparse or args.torch_composed):
        p.error("--wire-dtype bf16 needs a dense table and its own Add")
    if args.seed is not None:
        torch.manual_seed(args.seed)

    import multiverso_amd as mv
    from multiverso_amd.log import CHECK
    mv.init(sync=True)
    device = mv.Zoo.get().device
    if device.type != "cuda":
        args.rows = min(args.rows, 50_000)

    wire = torch.bfloat16 if args.wire_dtype == "bf16" else None
    if args.sparse:
        t = mv.SparseMatrixTable(args.rows, args.cols,
                                 updater_type=args.updater)
    else:
        t = mv.MatrixTable(args.rows, args.cols, updater_type=args.updater,
                           wire_dtype=wire)
    option = None
    if args.updater == "momentum":
        option = mv.AddOption(momentum=0.9)
    elif args.updater in ("adagrad", "dcasgd", "dcasgda"):
        option = mv.AddOption(worker_id=mv.rank(), learning_rate=0.1,
                              rho=0.1, lambda_=0.1)
    elif args.updater == "adam":
        option = mv.AddOption.adam(lr=0.1, weight_decay=0.01,
                                   worker_id=mv.rank())
    # the worker holds its buffers in the wire dtype
    out = torch.empty(args.rows, args.cols, device=device, dtype=t.wire)

    def timed(fn):
        mv.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if device.type == "cuda":
            torch.cuda.synchronize()
        mv.barrier()
        return (time.perf_counter() - t0) * 1e3

    def composed_add(ids, vals):
        mu = option.momentum
        w, m = t.shard, t.updater.smooth_gradient.view_as(t.shard)
        urows, inv = torch.unique(ids, return_inverse=True)
        agg = torch.zeros(urows.numel(), args.cols, device=device)
        agg.index_add_(0, inv, vals)
        mm = m[urows] * mu + (1.0 - mu) * agg
        m[urows] = mm
        w[urows] -= mm

    def timed_add(ids, vals):
        if args.torch_composed:
            CHECK(mv.size() == 1, "--torch-composed runs on one rank")
            fn = lambda: composed_add(ids, vals)
        else:
            fn = lambda: t.add_rows(ids, vals, option)
        if args.repeat <= 1:
            return timed(fn)
        timed(fn)
        return statistics.median(timed(fn) for _ in range(args.repeat))

    rows_all = torch.arange(args.rows, device=device)
    results = []
    for pct in range(10, 101, 10):
        k = args.rows * pct // 100
        ids = rows_all[torch.randperm(args.rows, device=device)[:k]]
        vals = torch.rand(k, args.cols, device=device).to(t.wire)
        if args.sparse:
            got = [0]

            def sget():
                got[0] = t.get_into(out)

            get_before = timed(sget)
            n_before = got[0]
            add_ms = timed_add(ids, vals)
            get_after = timed(sget)
            results.append((pct, add_ms, get_before, get_after))
            if mv.rank() == 0:
                print(f"add {pct:3d}% rows ({k}): add {add_ms:8.2f} ms | "
                      f"stale-get before {get_before:8.2f} ms "
                      f"({n_before} rows) after {get_after:8.2f} ms "
                      f"({got[0]} rows)", flush=True)
        else:
            get_before = timed(lambda: t.get(out=out))
            add_ms = timed_add(ids, vals)
            get_after = timed(lambda: t.get(out=out))
            results.append((pct, add_ms, get_before, get_after))
            if mv.rank() == 0:
                print(f"add {pct:3d}% rows ({k}): add {add_ms:8.2f} ms | "
                      f"get-all before {get_before:8.2f} ms after "
                      f"{get_after:8.2f} ms", flush=True)

    if mv.rank() == 0:
        print(mv.Dashboard.display())
    mv.shutdown()


if __name__ == "__main__":
    main()
