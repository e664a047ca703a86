"""Timings behind profiles/rowwise_adagrad.md.

  python tools/bench_rowwise_adagrad.py [--rows 1000000] [--ids 524288]
      [--out bench_outputs/rowwise_adagrad.jsonl]

The extension's entry points on float32 shards of rows x cols, cols in
{200, 64}, the row-wise kernels beside their element-wise adagrad siblings and
the K7 copy, alternating in ONE run so that they share the machine and its
neighbours (timed as tools/pool_perf.py and tools/bench_pooled_add.py time
theirs): device events around `--calls` back-to-back launches, `--windows`
windows per form after 2 warm-up launches each, the median and the range.
The whole-shard passes alternate their direction like Updater._sweep.

  whole   rowwise_adagrad_update | adagrad_update | nt_copy
  fused   rowwise_adagrad_copy_update | adagrad_copy_update
  keyed   --ids ids, uniform over the table or 8 to a row:
          row_rowwise_adagrad_update on the stably sorted ids (the sort is
          timed on its own) | row_scatter_adagrad on the ids as they come
  pooled  bags of 1, 8 and 64 ids, one weight per id:
          unpool_rowwise_adagrad_update | unpool_adagrad_update

GB/s is the traffic the algorithm needs over the time: 12 B an element plus
8 B a row against 20 B an element for the whole-shard passes (16 + 8/row
against 24 fused), 8 B an element for the copy.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

K = (0.5, 0.25, 1e-6)


def window(call, calls):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(calls):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def race(forms, args, **tags):
    """forms: {name: (call, bytes or None)}; one JSON line per form."""
    for call, _ in forms.values():
        for _ in range(2):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name in forms}
    for _ in range(args.windows):
        for name, (call, _) in forms.items():
            times[name].append(window(call, args.calls))
    lines = []
    for name, (_, nbytes) in forms.items():
        ms = statistics.median(times[name])
        line = dict(tags, form=name, ms=round(ms, 4),
                    range=[round(min(times[name]), 4),
                           round(max(times[name]), 4)])
        if nbytes:
            line["GBps"] = round(nbytes / ms / 1e6, 1)
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def measure(args, hip):
    g = torch.Generator().manual_seed(0)
    dev, lines, R = "cuda", [], args.rows
    for C in (200, 64):
        n = R * C
        w, wr = (torch.randn(R, C, device=dev) for _ in range(2))
        G, Gr = torch.zeros(R, C, device=dev), torch.zeros(R, device=dev)
        d = torch.randn(R, C, device=dev) * 1e-3
        out = torch.empty(R, C, device=dev)
        flip = {"rev": False}

        def rev():
            flip["rev"] = not flip["rev"]
            return flip["rev"]

        lines += race({
            "rowwise_adagrad_update": (lambda: hip.rowwise_adagrad_update(
                wr, Gr, d, C, *K, reverse=rev()), 12 * n + 8 * R),
            "adagrad_update": (lambda: hip.adagrad_update(
                w, G, d, *K, reverse=rev()), 20 * n),
            "nt_copy": (lambda: hip.nt_copy(out, d), 8 * n),
        }, args, kind="whole", cols=C)
        lines += race({
            "rowwise_adagrad_copy_update": (
                lambda: hip.rowwise_adagrad_copy_update(
                    wr, Gr, d, out, C, *K, reverse=rev()), 16 * n + 8 * R),
            "adagrad_copy_update": (lambda: hip.adagrad_copy_update(
                w, G, d, out, *K, reverse=rev()), 24 * n),
        }, args, kind="fused", cols=C)
        for spread in ("uniform", "8 per row"):
            ids = torch.randint(0, R, (args.ids,), generator=g)
            if spread != "uniform":
                ids = ids[:args.ids // 8].repeat(8)
            ids = ids.to(dev)
            vals = torch.randn(args.ids, C, device=dev) * 1e-3
            rows, perm = torch.sort(ids, stable=True)
            lines += race({
                "row_rowwise_adagrad_update": (
                    lambda: hip.row_rowwise_adagrad_update(
                        wr, Gr, rows, vals, *K, perm), None),
                "stable sort of the ids": (
                    lambda: torch.sort(ids, stable=True), None),
                "row_scatter_adagrad": (lambda: hip.row_scatter_adagrad(
                    w, G, ids, vals, *K), None),
            }, args, kind="keyed", cols=C, ids=spread)
        for L in (1, 8, 64):
            bags = args.ids // L
            ids = torch.randint(0, R, (bags * L,), generator=g).to(dev)
            src = torch.arange(bags * L, device=dev) // L
            wts = torch.rand(bags * L, device=dev) + 0.5
            grad = torch.randn(bags, C, device=dev) * 1e-3
            rows, perm = torch.sort(ids, stable=True)
            lines += race({
                "unpool_rowwise_adagrad_update": (
                    lambda: hip.unpool_rowwise_adagrad_update(
                        wr, Gr, rows, perm, src, grad, wts, *K), None),
                "unpool_adagrad_update": (
                    lambda: hip.unpool_adagrad_update(
                        w, G, rows, perm, src, grad, wts, *K), None),
            }, args, kind="pooled", cols=C, ids_per_bag=L)
        del w, wr, G, Gr, d, out
    return lines


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--ids", type=int, default=524_288)
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--out", default="bench_outputs/rowwise_adagrad.jsonl")
    args = p.parse_args()
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    from multiverso_amd import ops
    lines = measure(args, ops.module(required=True))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
