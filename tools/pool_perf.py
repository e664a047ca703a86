"""Timings behind profiles/pool_rows.md.

  python tools/pool_perf.py [--rows 1000000] [--ids 524288] [--weighted]

One MatrixTable of rows x cols float32 on one GPU for cols in {64, 200} (1M
rows: 256 MB and 800 MB). For bags of mean length L in {1, 8, 40, 400} (length
1, or uniform in 1 .. 2L-1; about --ids ids in all, drawn uniformly from the
table) five forms are timed in ONE run, alternating, so that they share the
machine and its neighbours:

  pool_rows     table.pool_rows(ids, offsets) with CPU ids and offsets: the
                host checks and two H2D copies, then k_row_pool
  composition   what a caller did before: table.get_rows(ids) with CPU ids and
                index_add_ of the [nnz, cols] rows into zeros(B, cols), the
                bag index of every id already on the device
  row_pool      the binding alone, ids and offsets on the device
  gather_add    the composition's kernels alone, everything on the device:
                row_gather, zeros(B, cols) and index_add_ (what _server_pool
                would run if it were routed to the composition)
  row_gather    K6 of the same ids, on the device: it reads the same rows and
                writes all of them, the byte floor of the read side

Device events around `--calls` back-to-back calls, `--windows` windows per
form after 2 warm-up calls each. The rates are the rows' bytes, nnz * cols * 4,
over the time of the form. Each line also gives the largest difference
between pool_rows and the composition at the timed size, and whether every
element differs by at most twice the bound (L + 2) * 2^-24 * S that each form
keeps to the exact sum.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def window(call, calls):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(calls):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def bags(mean_len, n_ids, rows, g):
    """(ids, offsets, weights) on the CPU."""
    n_bags = max(n_ids // mean_len, 1)
    lens = (torch.ones(n_bags, dtype=torch.int64) if mean_len == 1 else
            torch.randint(1, 2 * mean_len, (n_bags,), generator=g))
    offsets = torch.zeros(n_bags + 1, dtype=torch.int64)
    offsets[1:] = lens.cumsum(0)
    nnz = int(offsets[-1])
    return (torch.randint(0, rows, (nnz,), generator=g), offsets,
            torch.rand(nnz, generator=g) + 0.5)


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--ids", type=int, default=524_288)
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--weighted", action="store_true")
    args = p.parse_args()
    assert torch.cuda.is_available(), "pool_perf.py measures on a GPU"
    import multiverso_amd as mv
    from multiverso_amd import ops
    hip = ops.module(required=True)
    mv.init()
    g = torch.Generator().manual_seed(0)
    for cols in (64, 200):
        t = mv.MatrixTable(args.rows, cols, random_init=(-1.0, 1.0))
        for mean_len in (1, 8, 40, 400):
            ids, offs, w = bags(mean_len, args.ids, args.rows, g)
            w = w if args.weighted else None
            n_bags, nnz = offs.numel() - 1, ids.numel()
            d_ids, d_offs = ids.cuda(), offs.cuda()
            d_w = None if w is None else w.cuda()
            bag_of = torch.repeat_interleave(
                torch.arange(n_bags, device="cuda"), d_offs.diff())

            def composition():
                got = t.get_rows(ids)
                if d_w is not None:
                    got = got * d_w.unsqueeze(1)
                return torch.zeros(n_bags, cols, device="cuda").index_add_(
                    0, bag_of, got)

            def gather_add():
                got = hip.row_gather(t.shard, d_ids)
                if d_w is not None:
                    got = got * d_w.unsqueeze(1)
                return torch.zeros(n_bags, cols, device="cuda").index_add_(
                    0, bag_of, got)

            forms = {
                "pool_rows": lambda: t.pool_rows(ids, offs, w),
                "composition": composition,
                "gather_add": gather_add,
                "row_pool": lambda: hip.row_pool(t.shard, d_ids, d_offs, d_w),
                "row_gather": lambda: hip.row_gather(t.shard, d_ids),
            }
            for call in forms.values():
                for _ in range(2):
                    call()
            torch.cuda.synchronize()
            new, old = forms["pool_rows"](), forms["composition"]()
            mag = torch.zeros(n_bags, cols, device="cuda").index_add_(
                0, bag_of, (t.shard[d_ids] * (1 if d_w is None
                                              else d_w.unsqueeze(1))).abs())
            bound = (d_offs.diff().unsqueeze(1) + 2) * 2.0 ** -24 * mag
            times = {name: [] for name in forms}
            for _ in range(args.windows):
                for name, call in forms.items():
                    times[name].append(window(call, args.calls))
            line = {"rows": args.rows, "cols": cols, "mean_len": mean_len,
                    "bags": n_bags, "ids": nnz, "weighted": args.weighted}
            for name, v in times.items():
                line[name + "_ms"] = round(statistics.median(v), 4)
                line[name + "_ms_range"] = [round(min(v), 4), round(max(v), 4)]
            row_bytes = nnz * cols * 4
            line.update({
                "speedup_over_composition": round(
                    line["composition_ms"] / line["pool_rows_ms"], 2),
                "row_pool_over_gather_add": round(
                    line["gather_add_ms"] / line["row_pool_ms"], 2),
                "row_pool_GB_per_s": round(
                    row_bytes / line["row_pool_ms"] / 1e6, 1),
                "row_gather_GB_per_s": round(
                    row_bytes / line["row_gather_ms"] / 1e6, 1),
                "max_diff": float((new - old).abs().max()),
                "within_twice_the_bound": bool(
                    ((new - old).abs() <= 2 * bound).all())})
            print(json.dumps(line), flush=True)
    mv.shutdown()


if __name__ == "__main__":
    main()
