"""Timings behind profiles/pooled_add.md.

  python tools/bench_pooled_add.py [--rows 1000000] [--ids 524288]
      [--out profiles/pooled_add.md] [--resources hipcc_report.txt]

Two MatrixTables of rows x cols float32 on one GPU, for cols in {200, 64} and
the updaters sgd and adam. For bags of exactly L in {1, 8, 400} ids (about
--ids ids in all, drawn uniformly from the table, one weight per id) two forms
are timed in ONE run, alternating, each on its own table, so that they share
the machine and its neighbours:

  add_pooled  table.add_pooled(ids, offsets, grad, weights) with CPU ids and
              offsets and the [B, cols] gradient on the device: the host
              checks, the sort and k_row_unpool
  add_rows    what a caller did before: the [nnz, cols] rows weights[i] *
              grad[bag(i)] built on the device (timed, it is part of that
              path) and table.add_rows(ids, rows) with CPU ids

Device events around `--calls` back-to-back calls, `--windows` windows per form
after 2 warm-up calls each; the median and the range are reported. "Wire" is
what the values of either call put on the wire between ranks, nnz * cols * 4
against parts * cols * 4 bytes (on one rank parts == bags); the ids travel in
both. Both tables get the same calls, and the largest difference between their
shards at the end is reported. With --resources, the VGPR counts and the
occupancy of the k_row_unpool instantiations are read from the output of
`hipcc -Rpass-analysis=kernel-resource-usage` on kernels.hip.
"""

import argparse
import json
import os
import re
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


def resources(path):
    """(kernels, VGPR range, occupancy range, scratch bytes, LDS bytes) of the
    k_row_unpool instantiations in a kernel-resource-usage report."""
    found = re.findall(
        r"Function Name: (\S*k_row_unpool\S*).*?VGPRs: (\d+).*?"
        r"ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
        r".*?LDS Size \[bytes/block\]: (\d+)", open(path).read(), re.S)
    v, s, o, l = ([int(f[i]) for f in found] for i in (1, 2, 3, 4))
    return len(found), (min(v), max(v)), (min(o), max(o)), max(s), max(l)


def measure(args):
    import multiverso_amd as mv
    mv.init()
    g = torch.Generator().manual_seed(0)
    lines = []
    for cols in (200, 64):
        for updater in ("sgd", "adam"):
            pooled, expanded = (mv.MatrixTable(args.rows, cols,
                                               updater_type=updater)
                                for _ in range(2))
            for L in (1, 8, 400):
                n_bags = max(args.ids // L, 1)
                offs = torch.arange(n_bags + 1) * L
                ids = torch.randint(0, args.rows, (n_bags * L,), generator=g)
                w = (torch.rand(n_bags * L, generator=g) + 0.5).cuda()
                grad = (torch.randn(n_bags, cols, generator=g) * 1e-3).cuda()
                bag_of = torch.repeat_interleave(
                    torch.arange(n_bags, device="cuda"), L)
                forms = {
                    "add_pooled": lambda: pooled.add_pooled(ids, offs, grad,
                                                            w),
                    "add_rows": lambda: expanded.add_rows(
                        ids, grad[bag_of] * w.unsqueeze(1)),
                }
                for call in forms.values():
                    for _ in range(2):
                        call()
                torch.cuda.synchronize()
                times = {name: [] for name in forms}
                for _ in range(args.windows):
                    for name, call in forms.items():
                        times[name].append(window(call, args.calls))
                line = {"cols": cols, "updater": updater, "L": L,
                        "bags": n_bags, "ids": n_bags * L,
                        "distinct_rows": int(ids.unique().numel())}
                for name, v in times.items():
                    line[name + "_ms"] = round(statistics.median(v), 4)
                    line[name + "_range"] = [round(min(v), 4),
                                             round(max(v), 4)]
                line["speedup"] = round(line["add_rows_ms"]
                                        / line["add_pooled_ms"], 2)
                line["wire_pooled_MB"] = round(n_bags * cols * 4 / 1e6, 2)
                line["wire_rows_MB"] = round(n_bags * L * cols * 4 / 1e6, 2)
                line["max_diff"] = float(
                    (pooled.shard - expanded.shard).abs().max())
                print(json.dumps(line), flush=True)
                lines.append(line)
    mv.shutdown()
    return lines


def report(lines, args):
    out = ["| cols | updater | ids per bag | bags | distinct rows | add_pooled "
           "ms (range) | add_rows ms (range) | add_rows / add_pooled | wire "
           "MB pooled | wire MB rows | max diff |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for x in lines:
        out.append(
            f"| {x['cols']} | {x['updater']} | {x['L']} | {x['bags']} | "
            f"{x['distinct_rows']} | {x['add_pooled_ms']} "
            f"({x['add_pooled_range'][0]}-{x['add_pooled_range'][1]}) | "
            f"{x['add_rows_ms']} ({x['add_rows_range'][0]}-"
            f"{x['add_rows_range'][1]}) | {x['speedup']} | "
            f"{x['wire_pooled_MB']} | {x['wire_rows_MB']} | "
            f"{x['max_diff']:.2e} |")
    if args.resources:
        n, v, o, s, l = resources(args.resources)
        out += ["", f"k_row_unpool, {n} instantiations (compiler's resource "
                f"report, gfx950): {v[0]}-{v[1]} VGPRs, occupancy {o[0]}-"
                f"{o[1]} waves a SIMD, scratch {s} bytes a lane, LDS {l} "
                f"bytes a block."]
    return "\n".join(out) + "\n"


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--ids", type=int, default=524_288)
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--out", default="profiles/pooled_add.md")
    p.add_argument("--resources", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_pooled_add.py measures on a GPU"
    text = ("# MatrixTable.add_pooled against add_rows of the expanded rows\n\n"
            f"{args.rows} rows, about {args.ids} ids, {args.calls} calls a "
            f"window, {args.windows} windows a form, alternating in one run "
            "(tools/bench_pooled_add.py).\n\n" + report(measure(args), args))
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
