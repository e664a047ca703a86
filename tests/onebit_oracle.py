"""Oracle of the 1-bit Add wire format, shared by test_onebit_filter.py and
test_gpu_onebit_filter.py. It is written from the format's description alone
and imports nothing from multiverso_amd: payloads are taken apart with numpy,
group means are fp64, and everything the format fixes bit for bit (signs, pad
bits, the new residual, the decoded sum) is recomputed in fp32 on the CPU."""

import numpy as np
import torch

BLOCK = 1024
# relative bound on a scale against the fp64 mean of its group: an fp32 sum
# of at most 1024 same-signed terms is within (1024 - 1) * 2**-24 of the
# exact sum in any order (no cancellation), and the divide rounds once more,
# 2**-24: together 1024 * 2**-24 = 2**-14
SCALE_RTOL = 2.0 ** -14


def nblocks(n):
    return (n + BLOCK - 1) // BLOCK


def split(payload, n):
    """(scales [nb, 2] fp32 as (neg, pos), bits [nb * 1024] bool) of one
    payload; asserts its length."""
    raw = payload.detach().cpu().numpy().tobytes()
    nb = nblocks(n)
    assert len(raw) == 136 * nb, (len(raw), n)
    scales = np.frombuffer(raw[:8 * nb], dtype="<f4").reshape(nb, 2)
    bits = np.unpackbits(np.frombuffer(raw[8 * nb:], dtype=np.uint8),
                         bitorder="little")
    assert bits.size == nb * BLOCK
    return torch.from_numpy(scales.copy()), torch.from_numpy(bits.astype(bool))


def decode(payload, n):
    """The fp32 values one payload stands for."""
    scales, bits = split(payload, n)
    blk = torch.arange(n) // BLOCK
    return torch.where(bits[:n], scales[blk, 1], scales[blk, 0])


def decode_sum(payloads, n):
    """((q_0 + q_1) + ...) + q_{P-1} in fp32."""
    acc = decode(payloads[0], n)
    for p in payloads[1:]:
        acc = acc + decode(p, n)
    return acc


def same_bits(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32),
                       b.detach().cpu().contiguous().view(torch.int32))


def check_encode(d, r_before, payload, r_after, label=""):
    """Everything the format promises of one encode call. Returns the largest
    relative deviation of a scale from the fp64 mean of its group."""
    d, r_before, r_after = d.cpu(), r_before.cpu(), r_after.cpu()
    n = d.numel()
    scales, bits = split(payload, n)
    v = r_before + d                       # one fp32 add
    assert torch.equal(bits[:n], v >= 0), label
    assert not bool(bits[n:].any()), label  # pad bits
    worst = 0.0
    for b in range(nblocks(n)):
        vb = v[b * BLOCK:(b + 1) * BLOCK].double()
        for col, mask in ((0, ~(vb >= 0)), (1, vb >= 0)):
            s = float(scales[b, col])
            if not bool(mask.any()):
                assert s == 0.0, (label, b, col, s)
                continue
            mean = float(vb[mask].mean())
            dev = abs(s - mean)
            assert dev <= SCALE_RTOL * abs(mean), (label, b, col, s, mean)
            if mean:
                worst = max(worst, dev / abs(mean))
    blk = torch.arange(n) // BLOCK
    q = torch.where(bits[:n], scales[blk, 1], scales[blk, 0])
    assert same_bits(r_after, v - q), label   # one fp32 subtract
    return worst
