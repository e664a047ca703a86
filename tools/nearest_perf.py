"""Timings behind profiles/nearest_rows.md.

  python tools/nearest_perf.py [--rows 1000000] [--cols 200]

One MatrixTable of rows x cols float32 on one GPU (1M x 200 = 800 MB, larger
than the Infinity Cache). For Q in {1, 4, 16}, k in {10, 64} and both metrics
three forms are timed in ONE run, alternating, so that they share the machine
and its neighbours:

  nearest_rows   table.nearest_rows(q, k, metric): k_row_topk + k_topk_merge
  composition    what the serving example did before: table.get() and then
                 cosine_similarity + topk per query (dot: get + matmul + topk)
  K7 copy        k_elem<CopyOp> of the same shard, the byte-rate yardstick

Device events around `--calls` back-to-back calls, `--windows` windows per
form after 2 warm-up calls each. The scan's rate is the shard's bytes, read
once, over the time of nearest_rows (both kernels and the two small
allocations of the binding included); the copy's rate is read + write, 8
bytes per element. Each line also says whether the two forms agree on the
ids, compared at the timed size.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def composition(table, q, k, metric):
    full = table.get()
    if metric == "cosine":
        sims = torch.stack([torch.nn.functional.cosine_similarity(
            full, v.unsqueeze(0), dim=1) for v in q])
    else:
        sims = q @ full.t()
    return torch.topk(sims, k, dim=1)


def window(call, calls):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(calls):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--cols", type=int, default=200)
    p.add_argument("--calls", type=int, default=40)
    p.add_argument("--windows", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "nearest_perf.py measures on a GPU"
    import multiverso_amd as mv
    from multiverso_amd import ops
    hip = ops.module(required=True)
    mv.init()
    t = mv.MatrixTable(args.rows, args.cols)
    g = torch.Generator(device="cuda").manual_seed(0)
    t.shard.copy_(torch.randn(args.rows, args.cols, generator=g,
                              device="cuda"))
    dst = torch.empty_like(t.shard)
    shard_bytes = t.shard.numel() * 4
    for metric in ("cosine", "dot"):
        for Q in (1, 4, 16):
            q = torch.randn(Q, args.cols, generator=g, device="cuda")
            for k in (10, 64):
                forms = {
                    "nearest_rows": lambda: t.nearest_rows(q, k, metric),
                    "composition": lambda: composition(t, q, k, metric),
                    "k7_copy": lambda: hip.nt_copy(dst.view(-1),
                                                   t.shard.view(-1)),
                }
                for call in forms.values():
                    for _ in range(2):
                        call()
                torch.cuda.synchronize()
                ids_new = t.nearest_rows(q, k, metric)[1]
                ids_old = composition(t, q, k, metric).indices
                same = bool((ids_new.sort(1).values
                             == ids_old.sort(1).values).all())
                times = {name: [] for name in forms}
                for _ in range(args.windows):
                    for name, call in forms.items():
                        times[name].append(window(call, args.calls))
                med = {n: statistics.median(v) for n, v in times.items()}
                scan_rate = shard_bytes / med["nearest_rows"]
                copy_rate = 2 * shard_bytes / med["k7_copy"]
                print(json.dumps({
                    "rows": args.rows, "cols": args.cols, "metric": metric,
                    "Q": Q, "k": k,
                    "nearest_rows_ms": round(med["nearest_rows"], 4),
                    "nearest_rows_ms_range": [
                        round(min(times["nearest_rows"]), 4),
                        round(max(times["nearest_rows"]), 4)],
                    "composition_ms": round(med["composition"], 4),
                    "composition_ms_range": [
                        round(min(times["composition"]), 4),
                        round(max(times["composition"]), 4)],
                    "k7_copy_ms": round(med["k7_copy"], 4),
                    "scan_TB_per_s": round(scan_rate / 1e9, 3),
                    "copy_TB_per_s": round(copy_rate / 1e9, 3),
                    "scan_rate_over_copy_rate": round(
                        scan_rate / copy_rate, 3),
                    "speedup_over_composition": round(
                        med["composition"] / med["nearest_rows"], 2),
                    "same_id_sets": same}), flush=True)
    mv.shutdown()


if __name__ == "__main__":
    main()
