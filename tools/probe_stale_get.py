"""Timings behind profiles/stale_get.md.

  python tools/probe_stale_get.py [--rows 1000000] [--repeats 1000]

SparseMatrixTable's stale-row Get on one GPU, at rows x 50 and rows x 200,
with 1 %, 10 % and 100 % of the rows stale, for 1 and 8 workers (for 8 the
bitmap is hand-made: one process serves as the owner of all of them):

  take   _take_stale(0, workers) alone: the stale lists and the marking
  get    the whole single-rank get_into(cache) (1 worker)

each in two forms that alternate call by call in one process:

  hip    k_stale_count / k_stale_scan / k_stale_emit, and for `get`
         row_gather_at straight into the cache
  torch  the torch path inside _take_stale (nonzero per worker, index_put
         to mark), and for `get` the K6 gather into a temporary plus
         index_put into the cache: what the table ran before the kernels

The K7 copy of a rows x cols tensor is timed in the same loop as a yardstick.
The bitmap is put back before every call, outside the timed window; a call is
timed by the host clock from a synchronise to the synchronise after it (the
operation itself waits for the device once, so device events alone would miss
what it is about). 5 warm-up rounds, then the median and the quartiles over
--repeats calls, one JSON line per form. Run the command again for the spread
between runs.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--repeats", type=int, default=1000)
    args = p.parse_args()
    assert torch.cuda.is_available(), "probe_stale_get.py measures on a GPU"
    import multiverso_amd as mv
    from multiverso_amd import ops
    hip = ops.module(required=True)
    mv.init()
    R = args.rows
    g = torch.Generator().manual_seed(0)
    for cols in (50, 200):
        t = mv.SparseMatrixTable(R, cols)
        t.shard.copy_(torch.randn(R, cols, generator=g))
        cache = torch.zeros(R, cols, device="cuda")

        def take(in_hip):
            t._hip_stale = in_hip
            return t._take_stale(0, t.up_to_date.size(0))

        def get(in_hip):
            if in_hip:
                t._hip_stale = True
                return t.get_into(cache)
            (n,), stale = take(False)
            if n:
                cache[stale] = t._gather_local(stale)
            return n

        forms = {"K7 copy": lambda: hip.nt_copy(cache, t.shard)}
        for name, fn in (("take", take), ("get", get)):
            forms[name + " hip"] = lambda fn=fn: fn(True)
            forms[name + " torch"] = lambda fn=fn: fn(False)
        for nw in (1, 8):
            for frac in (0.01, 0.1, 1.0):
                start = (torch.rand(nw, R, generator=g) >= frac).cuda()
                t.up_to_date = start.clone()
                names = [k for k in forms if nw == 1 or k.startswith("take")]
                times = {k: [] for k in names}
                for it in range(5 + args.repeats):
                    for name in names:
                        t.up_to_date.copy_(start)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        forms[name]()
                        torch.cuda.synchronize()
                        if it >= 5:
                            times[name].append(
                                (time.perf_counter() - t0) * 1e3)
                assert bool(t.up_to_date.all())
                for name in names:
                    q = statistics.quantiles(times[name], n=4)
                    print(json.dumps({
                        "form": name, "rows": R, "cols": cols,
                        "workers": nw, "stale": frac,
                        "ms": round(q[1], 4), "ms_q1": round(q[0], 4),
                        "ms_q3": round(q[2], 4),
                        "window_ms": round(sum(times[name]), 1)}), flush=True)
        del t, cache
    mv.shutdown()


if __name__ == "__main__":
    main()
