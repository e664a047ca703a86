"""Timings behind profiles/onebit_filter.md.

  python tools/onebit_perf.py kernels [--elements 128000000]
      k_onebit_encode, k_onebit_decode_sum (P = 1) and the K7 copy
      (k_elem<CopyOp>, the project's bandwidth yardstick) on one GPU: device
      events around 20 back-to-back calls, 5 windows per form with the forms
      alternating, after 3 warm-up calls each.

  python tools/onebit_perf.py plane --plane async|sync [--ranks 2]
                                    [--elements 32000000] [--gpu-share]
      Whole-table Add of an ArrayTable with add_filter=None and then
      "onebit" on `ranks` processes: host clock around an acknowledged Add
      plus a device synchronise, median of --adds after 2 warm-up Adds, and
      the bytes this rank puts on the wire per Add. --gpu-share maps every
      rank to cuda:0 (the async plane is host-staged over gloo and runs so;
      the sync plane is RCCL and needs one GPU per rank — with fewer it
      prints "not measured").
"""

import argparse
import json
import os
import socket
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def kernels(n: int) -> None:
    from multiverso_amd import onebit_filter, ops
    hip = ops.module(required=True)
    g = torch.Generator(device="cpu").manual_seed(0)
    d = torch.randn(n, generator=g).cuda()
    r = torch.zeros(n, device="cuda")
    payload = torch.empty(onebit_filter.payload_bytes(n), dtype=torch.uint8,
                          device="cuda")
    out = torch.empty(n, device="cuda")
    dst = torch.empty(n, device="cuda")
    pb = payload.numel() / n
    forms = {
        # name: (call, bytes per element the algorithm needs)
        "k_onebit_encode": (lambda: hip.onebit_encode(d, r, payload),
                            12 + pb),
        "k_onebit_decode_sum P=1": (
            lambda: hip.onebit_decode_sum(out, payload, 1), 4 + pb),
        "k_elem<CopyOp> (K7)": (lambda: hip.nt_copy(dst, d), 8),
    }
    for call, _ in forms.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(5):
        for name, (call, _) in forms.items():
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            for _ in range(20):
                call()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / 20)
    k7 = statistics.median(times["k_elem<CopyOp> (K7)"])
    k7_rate = 8 * n / k7
    for name, (_, bpe) in forms.items():
        ts = times[name]
        med = statistics.median(ts)
        rate = bpe * n / med
        print(json.dumps({
            "kernel": name, "elements": n, "ms": round(med, 4),
            "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
            "bytes_per_element": round(bpe, 3),
            "TB_per_s": round(rate / 1e9, 3),
            "rate_over_k7": round(rate / k7_rate, 3),
            "time_over_k7": round(med / k7, 3)}), flush=True)


def _plane_rank(rank, ranks, port, plane, n, adds, gpu_share):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank), WORLD_SIZE=str(ranks),
                      LOCAL_RANK="0" if gpu_share else str(rank),
                      MV_BACKEND="gloo" if plane == "async" else "nccl")
    import multiverso_amd as mv
    from multiverso_amd import onebit_filter
    from multiverso_amd.dashboard import Dashboard
    mv.init(sync=(plane == "sync"))
    g = torch.Generator(device="cpu").manual_seed(rank)
    delta = torch.randn(n, generator=g).to(mv.Zoo.get().device)
    for filt in (None, "onebit"):
        t = mv.ArrayTable(n, add_filter=filt)
        for _ in range(2):
            t.add(delta)
        torch.cuda.synchronize()
        mv.barrier()
        Dashboard.reset()
        ts = []
        for _ in range(adds):
            t0 = time.perf_counter()
            t.add(delta)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            mv.barrier()
        remote = [c for s, c in enumerate(t.spec.counts) if s != rank]
        wire = (sum(onebit_filter.payload_bytes(c) for c in remote) if filt
                else 4 * sum(remote))
        if rank == 0:
            print(json.dumps({
                "plane": plane, "ranks": ranks, "elements": n,
                "add_filter": filt, "ms_per_add": round(
                    statistics.median(ts), 3),
                "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                "wire_bytes_per_add": wire,
                "dashboard_bytes_in_per_add": Dashboard.get(
                    "onebit_filter.bytes_in").elapsed_ms / adds,
                "dashboard_bytes_out_per_add": Dashboard.get(
                    "onebit_filter.bytes_out").elapsed_ms / adds}),
                flush=True)
        mv.barrier()
    mv.shutdown()


def plane(args) -> None:
    if not args.gpu_share and torch.cuda.device_count() < args.ranks:
        print(json.dumps({"plane": args.plane, "ranks": args.ranks,
                          "result": "not measured", "reason":
                          f"{torch.cuda.device_count()} GPU(s) visible"}))
        return
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.start_processes(_plane_rank, args=(args.ranks, port, args.plane,
                                          args.elements, args.adds,
                                          args.gpu_share),
                       nprocs=args.ranks, join=True, start_method="spawn")


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["kernels", "plane"])
    p.add_argument("--elements", type=int, default=None)
    p.add_argument("--plane", choices=["async", "sync"], default="async")
    p.add_argument("--ranks", type=int, default=2)
    p.add_argument("--adds", type=int, default=7)
    p.add_argument("--gpu-share", dest="gpu_share", action="store_true")
    args = p.parse_args()
    assert torch.cuda.is_available(), "onebit_perf.py measures on a GPU"
    if args.mode == "kernels":
        kernels(args.elements or 128_000_000)
    else:
        args.elements = args.elements or 32_000_000
        plane(args)


if __name__ == "__main__":
    main()
