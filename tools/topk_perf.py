"""Timings behind profiles/topk_filter.md.

  python tools/topk_perf.py [--elements 128000000] [--calls 20]

k_topk_encode and k_topk_decode_sum (P = 1) at keep 8 and 32 on one GPU, with
the yardsticks taken in the same run: the K7 copy (k_elem<CopyOp>, the
project's bandwidth figure) and k_onebit_encode / k_onebit_decode_sum.

Encode is timed on three deltas, since its histogram passes depend on how the
magnitudes spread over the radix bins: "normal" (standard normal), "one
exponent" (magnitudes uniform in [1, 2): every element lands in one bin of
the first pass and stays undecided, the histogram's worst case) and "sparse"
(1 in 64 non-zero: the zeros pile onto bin 0).

Every call has its own pair of device events; the residual is put back to
zero before each encode, outside the timed window, so every call codes the
same input. The forms alternate, 3 warm-up calls each; the median, minimum
and maximum over --calls are printed, one JSON line per form.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--elements", type=int, default=128_000_000)
    p.add_argument("--calls", type=int, default=20)
    args = p.parse_args()
    assert torch.cuda.is_available(), "topk_perf.py measures on a GPU"
    from multiverso_amd import onebit_filter, ops, topk_filter
    hip = ops.module(required=True)
    n = args.elements
    torch.manual_seed(0)
    deltas = {"normal": torch.randn(n, device="cuda")}
    sign = torch.randint(0, 2, (n,), device="cuda").float() * 2 - 1
    deltas["one exponent"] = (1 + torch.rand(n, device="cuda")) * sign
    deltas["sparse"] = deltas["normal"] * (
        torch.randint(0, 64, (n,), device="cuda") == 0)
    del sign
    r = torch.zeros(n, device="cuda")
    out = torch.empty(n, device="cuda")
    one = torch.empty(onebit_filter.payload_bytes(n), dtype=torch.uint8,
                      device="cuda")
    pay = {m: torch.empty(topk_filter.payload_bytes(n, m), dtype=torch.uint8,
                          device="cuda") for m in (8, 32)}

    # name: (call, bytes per element the algorithm needs, resets r)
    forms = {"k_elem<CopyOp> (K7)": (lambda: hip.nt_copy(out, r), 8, False)}
    for m in (8, 32):
        pb = 6 * m / 1024
        for kind, d in deltas.items():
            forms[f"k_topk_encode keep={m} {kind}"] = (
                lambda d=d, m=m: hip.topk_encode(d, r, pay[m], m),
                12 + pb, True)
        forms[f"k_topk_decode_sum keep={m} P=1"] = (
            lambda m=m: hip.topk_decode_sum(out, pay[m], 1, m), 4 + pb, False)
    forms["k_onebit_encode normal"] = (
        lambda: hip.onebit_encode(deltas["normal"], r, one), 12 + 136 / 1024,
        True)
    forms["k_onebit_decode_sum P=1"] = (
        lambda: hip.onebit_decode_sum(out, one, 1), 4 + 136 / 1024, False)

    times = {k: [] for k in forms}
    for it in range(3 + args.calls):
        for name, (call, _, resets) in forms.items():
            if resets:
                r.zero_()
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            call()
            b.record()
            b.synchronize()
            if it >= 3:
                times[name].append(a.elapsed_time(b))
    k7 = statistics.median(times["k_elem<CopyOp> (K7)"])
    for name, (_, bpe, _) in forms.items():
        med = statistics.median(times[name])
        rate = bpe * n / med
        print(json.dumps({
            "kernel": name, "elements": n, "ms": round(med, 4),
            "ms_min": round(min(times[name]), 4),
            "ms_max": round(max(times[name]), 4),
            "bytes_per_element": round(bpe, 3),
            "TB_per_s": round(rate / 1e9, 3),
            "rate_over_k7": round(rate / (8 * n / k7), 3),
            "time_over_k7": round(med / k7, 3)}), flush=True)


if __name__ == "__main__":
    main()
