"""OneBitFilter — 1-bit quantisation with error feedback for whole-table Add.

The reference names this filter and leaves it empty (``OneBitsFilter``,
include/multiverso/util/quantization_util.h:160-161). This is the scheme it
was named for (Seide et al., "1-Bit Stochastic Gradient Descent and its
Application to Data-Parallel Distributed Training of Speech DNNs",
Interspeech 2014): every value travels as its sign, each block of values
shares two scales, and what the code loses stays with the sender as a
residual that is added to the next delta.

Wire format. A whole-table delta is split by ``ShardSpec`` into one piece per
server; each piece is coded on its own in blocks of 1024 elements counted from
the start of the piece, the last block maybe partial. A piece of ``n``
elements has ``nb = ceil(n/1024)`` blocks and a payload of ``136*nb`` bytes,
no header (the size follows from ``n``):

    [0, 8*nb)        nb pairs of little-endian fp32 (neg, pos)
    [8*nb, 136*nb)   nb x 128 bytes of sign bits

Element ``i`` of a block is bit ``i % 8`` of byte ``i / 8`` (bit ``i % 64`` of
little-endian 64-bit word ``i / 64``, one wave64 ballot). Pad bits are 0.

Encode, per block, from delta ``d`` and residual ``r``: ``v = r + d`` (fp32),
``bit = (v >= 0)``, ``pos`` / ``neg`` = the fp32 mean of the ``v`` with bit
1 / 0 (0 for an empty group), ``r <- v - (bit ? pos : neg)``. Decode-sum at
the owner: ``out = ((q_0 + q_1) + ...) + q_{P-1}`` over ``P`` payloads of the
same piece in source-rank order, ``q_p = bit ? pos_p : neg_p``.

GPU tensors go through the ``k_onebit_encode`` / ``k_onebit_decode_sum``
kernels (one launch per piece); CPU tensors through the torch code below,
which writes the same format. The two may differ in the last bit of a scale
(the order of the fp32 sums is each implementation's own, and fixed), never
in a sign bit. About 30x fewer bytes than fp32 (4.13 bits per element).

Out of scope here: fusing the decode into the updater kernels, combining the
filter with the bf16 wire, filtering Get or row-keyed traffic, and
checkpointing the residual.
"""

from __future__ import annotations

import sys
from typing import Optional, Sequence, Union

import torch

from .dashboard import Dashboard

BLOCK = 1024
_BLOCK_BYTES = 8 + BLOCK // 8   # two fp32 scales + 1024 sign bits


def payload_bytes(n: int) -> int:
    """Bytes of the payload of an ``n``-element piece."""
    return _BLOCK_BYTES * ((n + BLOCK - 1) // BLOCK)


def _check_piece(t: torch.Tensor, name: str) -> None:
    if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
        raise TypeError(f"onebit_filter: {name} must be a flat contiguous "
                        f"float32 tensor")


def encode(delta_piece: torch.Tensor, residual_piece: torch.Tensor,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Code ``residual_piece + delta_piece`` into a uint8 payload (``out`` when
    given: ``payload_bytes(n)`` bytes, 8-byte aligned) and leave the
    quantisation error in ``residual_piece``, in place."""
    _check_piece(delta_piece, "delta_piece")
    _check_piece(residual_piece, "residual_piece")
    n = delta_piece.numel()
    if n < 1 or residual_piece.numel() != n:
        raise ValueError("onebit_filter.encode: delta and residual pieces "
                         "must have the same nonzero size")
    nbytes = payload_bytes(n)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8,
                          device=delta_piece.device)
    m = Dashboard.get("onebit_filter.bytes_in")
    m.count += 1
    m.elapsed_ms += n * 4
    Dashboard.get("onebit_filter.bytes_out").elapsed_ms += nbytes
    if delta_piece.is_cuda:
        from . import ops
        ops.module(required=True).onebit_encode(delta_piece, residual_piece,
                                                out)
    else:
        _encode_torch(delta_piece, residual_piece, out)
    return out


def decode_sum(payloads: Union[torch.Tensor, Sequence[torch.Tensor]], n: int,
               nparts: int, out: Optional[torch.Tensor] = None
               ) -> torch.Tensor:
    """Sum of the values that ``nparts`` payloads of one ``n``-element piece
    decode to, added left to right in fp32. ``payloads`` is one uint8 tensor
    holding them back to back (or a sequence of them, which is
    concatenated)."""
    if not isinstance(payloads, torch.Tensor):
        payloads = torch.cat([p.reshape(-1) for p in payloads])
    payloads = payloads.reshape(-1)
    if payloads.dtype != torch.uint8:
        raise TypeError("onebit_filter.decode_sum: payloads must be uint8")
    if n < 1 or nparts < 1 or payloads.numel() != nparts * payload_bytes(n):
        raise ValueError(f"onebit_filter.decode_sum: {nparts} payloads of a "
                         f"{n}-element piece take "
                         f"{nparts * payload_bytes(n)} bytes, got "
                         f"{payloads.numel()}")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=payloads.device)
    _check_piece(out, "out")
    if out.numel() != n:
        raise ValueError("onebit_filter.decode_sum: out size mismatch")
    if out.is_cuda:
        from . import ops
        if payloads.data_ptr() % 8:
            payloads = payloads.clone()
        ops.module(required=True).onebit_decode_sum(out, payloads, nparts)
    else:
        _decode_sum_torch(payloads, n, nparts, out)
    return out


# ---- the same format in torch ops (CPU tables, gloo runs) ----

def _bit_weights(device) -> torch.Tensor:
    return torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8,
                        device=device)


def _encode_torch(d: torch.Tensor, r: torch.Tensor, out: torch.Tensor) -> None:
    assert sys.byteorder == "little"
    n = d.numel()
    nb = (n + BLOCK - 1) // BLOCK
    v = torch.zeros(nb * BLOCK, dtype=torch.float32, device=d.device)
    torch.add(r, d, out=v[:n])
    valid = torch.zeros(nb * BLOCK, dtype=torch.bool, device=d.device)
    valid[:n] = True
    v2, valid = v.view(nb, BLOCK), valid.view(nb, BLOCK)
    pos = (v2 >= 0) & valid
    neg = ~pos & valid
    zero = torch.zeros((), dtype=torch.float32, device=d.device)
    scales = torch.empty(nb, 2, dtype=torch.float32, device=d.device)
    for col, mask in ((0, neg), (1, pos)):
        cnt = mask.sum(1)
        tot = torch.where(mask, v2, zero).sum(1)
        scales[:, col] = torch.where(cnt > 0, tot / cnt.clamp(min=1).float(),
                                     zero)
    q = torch.where(pos, scales[:, 1:2], scales[:, 0:1]).view(-1)
    torch.sub(v[:n], q[:n], out=r)
    bits = (pos.view(nb, BLOCK // 8, 8).to(torch.uint8)
            * _bit_weights(d.device)).sum(-1, dtype=torch.uint8)
    out[:8 * nb].copy_(scales.view(-1).view(torch.uint8))
    out[8 * nb:].copy_(bits.view(-1))


def _decode_sum_torch(payloads: torch.Tensor, n: int, nparts: int,
                      out: torch.Tensor) -> None:
    assert sys.byteorder == "little"
    nb = (n + BLOCK - 1) // BLOCK
    pl = payloads.view(nparts, _BLOCK_BYTES * nb)
    shifts = torch.arange(8, dtype=torch.uint8, device=pl.device)
    for p in range(nparts):
        # clone: a slice of a staged blob need not be 4-byte aligned
        scales = pl[p, :8 * nb].clone().view(torch.float32).view(nb, 2)
        bits = ((pl[p, 8 * nb:].view(nb, BLOCK // 8, 1) >> shifts) & 1).bool()
        q = torch.where(bits.view(nb, BLOCK), scales[:, 1:2],
                        scales[:, 0:1]).view(-1)[:n]
        if p == 0:
            out.copy_(q)
        else:
            out.add_(q)
