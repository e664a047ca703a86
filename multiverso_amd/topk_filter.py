"""TopKFilter — block top-k sparsification with error feedback for whole-table
Add.

The reference's ``SparseFilter`` wire is (index, value) pairs of the non-zero
entries (include/multiverso/util/quantization_util.h:38-158). This is that
idea made lossy, the gradient sparsification of Strom (Interspeech 2015), Aji
& Heafield (EMNLP 2017) and Lin et al. ("Deep Gradient Compression", ICLR
2018): of ``residual + delta`` only the largest-magnitude entries travel, as
exact fp32, and the rest stays with the sender as a residual that is added to
the next delta.

Wire format. A whole-table delta is split by ``ShardSpec`` into one piece per
server; each piece is coded on its own in blocks of 1024 elements counted from
the start of the piece, the last block maybe partial. With ``keep = m`` pairs
per block (a multiple of 4 in 4..256, 32 by default) a piece of ``n`` elements
has ``nb = ceil(n/1024)`` blocks and a payload of ``6*m*nb`` bytes, no header
(the size follows from ``n``):

    [0, 4*m*nb)        nb x m little-endian fp32 values
    [4*m*nb, 6*m*nb)   nb x m little-endian uint16 positions inside the block

Encode, per block, from delta ``d`` and residual ``r``: ``v = r + d`` (one
fp32 add), ``key = bits(v) & 0x7fffffff`` compared as an integer (so NaN ranks
above inf and is sent, and -0.0 equals +0.0). The ``m`` valid elements with
the largest keys are sent, equal keys going to the lower index, as pairs in
ascending index order. A partial block with ``c < m`` valid elements sends all
``c`` and fills the other slots with value +0.0 and position 0xFFFF (empty).
``r <- +0.0`` at sent positions and ``r <- v`` elsewhere. Decode-sum at the
owner: ``out`` starts at +0.0 and takes ``out[pos] += val`` for each pair of
payloads ``0..P-1`` of the same piece in source-rank order.

Nothing is rounded after the one add, so the ``k_topk_encode`` /
``k_topk_decode_sum`` kernels (GPU tensors, one launch per piece) and the
torch code below (CPU tensors) give the same bytes. 21x fewer bytes than fp32
at keep 32, 85x at keep 8.

Out of scope here: fusing the decode into the updater kernels, a sparse
row-update path at the owner, bf16 values in the pairs, filtering Get or
row-keyed traffic, and checkpointing the residual.
"""

from __future__ import annotations

import sys
from typing import Optional, Sequence, Union

import torch

from .dashboard import Dashboard

BLOCK = 1024
DEFAULT_KEEP = 32
_EMPTY = 0xFFFF


def check_keep(keep: int) -> int:
    if (isinstance(keep, bool) or not isinstance(keep, int)
            or not 4 <= keep <= 256 or keep % 4):
        raise ValueError(f"topk_filter: keep must be a multiple of 4 in "
                         f"4..256, got {keep!r}")
    return keep


def payload_bytes(n: int, keep: int = DEFAULT_KEEP) -> int:
    """Bytes of the payload of an ``n``-element piece."""
    return 6 * keep * ((n + BLOCK - 1) // BLOCK)


def _check_piece(t: torch.Tensor, name: str) -> None:
    if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
        raise TypeError(f"topk_filter: {name} must be a flat contiguous "
                        f"float32 tensor")


def encode(delta_piece: torch.Tensor, residual_piece: torch.Tensor,
           keep: int = DEFAULT_KEEP, out: Optional[torch.Tensor] = None
           ) -> torch.Tensor:
    """Code ``residual_piece + delta_piece`` into a uint8 payload (``out`` when
    given: ``payload_bytes(n, keep)`` bytes, 8-byte aligned) and leave what
    was not sent in ``residual_piece``, in place."""
    _check_piece(delta_piece, "delta_piece")
    _check_piece(residual_piece, "residual_piece")
    check_keep(keep)
    n = delta_piece.numel()
    if n < 1 or residual_piece.numel() != n:
        raise ValueError("topk_filter.encode: delta and residual pieces "
                         "must have the same nonzero size")
    nbytes = payload_bytes(n, keep)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8,
                          device=delta_piece.device)
    m = Dashboard.get("topk_filter.bytes_in")
    m.count += 1
    m.elapsed_ms += n * 4
    Dashboard.get("topk_filter.bytes_out").elapsed_ms += nbytes
    if delta_piece.is_cuda:
        from . import ops
        ops.module(required=True).topk_encode(delta_piece, residual_piece,
                                              out, keep)
    else:
        _encode_torch(delta_piece, residual_piece, keep, out)
    return out


def decode_sum(payloads: Union[torch.Tensor, Sequence[torch.Tensor]], n: int,
               nparts: int, keep: int = DEFAULT_KEEP,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sum of what ``nparts`` payloads of one ``n``-element piece hold for
    each element, added in payload order in fp32 from +0.0. ``payloads`` is
    one uint8 tensor holding them back to back (or a sequence of them, which
    is concatenated)."""
    if not isinstance(payloads, torch.Tensor):
        payloads = torch.cat([p.reshape(-1) for p in payloads])
    payloads = payloads.reshape(-1)
    check_keep(keep)
    if payloads.dtype != torch.uint8:
        raise TypeError("topk_filter.decode_sum: payloads must be uint8")
    if (n < 1 or nparts < 1
            or payloads.numel() != nparts * payload_bytes(n, keep)):
        raise ValueError(f"topk_filter.decode_sum: {nparts} payloads of a "
                         f"{n}-element piece at keep {keep} take "
                         f"{nparts * payload_bytes(n, keep)} bytes, got "
                         f"{payloads.numel()}")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=payloads.device)
    _check_piece(out, "out")
    if out.numel() != n:
        raise ValueError("topk_filter.decode_sum: out size mismatch")
    if out.is_cuda:
        from . import ops
        if payloads.data_ptr() % 8:
            payloads = payloads.clone()
        ops.module(required=True).topk_decode_sum(out, payloads, nparts, keep)
    else:
        _decode_sum_torch(payloads, n, nparts, keep, out)
    return out


class Codec:
    """The codec bound to one ``keep``: what a table built with
    ``add_filter="topk:M"`` encodes and decodes its whole-table Adds with
    (``payload_bytes(n)``, ``encode(piece, res, out=None)``,
    ``decode_sum(payloads, n, nparts, out=None)`` — the signatures of the
    onebit_filter module, which is the one-bit tables' codec)."""

    def __init__(self, keep: int = DEFAULT_KEEP) -> None:
        self.keep = check_keep(keep)

    def payload_bytes(self, n: int) -> int:
        return payload_bytes(n, self.keep)

    def encode(self, delta_piece, residual_piece, out=None):
        return encode(delta_piece, residual_piece, self.keep, out)

    def decode_sum(self, payloads, n, nparts, out=None):
        return decode_sum(payloads, n, nparts, self.keep, out)


# ---- the same format in torch ops (CPU tables, gloo runs) ----

def _encode_torch(d: torch.Tensor, r: torch.Tensor, m: int,
                  out: torch.Tensor) -> None:
    assert sys.byteorder == "little"
    n = d.numel()
    nb = (n + BLOCK - 1) // BLOCK
    v = torch.zeros(nb * BLOCK, dtype=torch.float32, device=d.device)
    torch.add(r, d, out=v[:n])
    key = v.view(torch.int32) & 0x7FFFFFFF
    key[n:] = -1                        # below every valid key
    # stable: equal keys stay in index order, the lower index first
    order = key.view(nb, BLOCK).sort(dim=1, descending=True,
                                     stable=True).indices[:, :m]
    start = torch.arange(nb, device=d.device).view(nb, 1) * BLOCK
    empty = order + start >= n
    pos = torch.where(empty, _EMPTY, order).sort(dim=1).values
    empty = pos == _EMPTY
    at = (pos + start)[~empty]
    vals = torch.zeros(nb, m, dtype=torch.float32, device=d.device)
    vals[~empty] = v[at]
    v[at] = 0.0
    r.copy_(v[:n])
    out[:4 * m * nb].copy_(vals.view(-1).view(torch.uint8))
    # 0xFFFF wraps to int16 -1: the same two bytes
    out[4 * m * nb:].copy_(torch.where(empty, -1, pos).to(torch.int16)
                           .view(-1).view(torch.uint8))


def _decode_sum_torch(payloads: torch.Tensor, n: int, nparts: int, m: int,
                      out: torch.Tensor) -> None:
    assert sys.byteorder == "little"
    nb = (n + BLOCK - 1) // BLOCK
    pl = payloads.view(nparts, 6 * m * nb)
    start = torch.arange(nb, device=pl.device).view(nb, 1) * BLOCK
    out.zero_()
    for p in range(nparts):
        # clone: a slice of a staged blob need not be 4-byte aligned
        vals = pl[p, :4 * m * nb].clone().view(torch.float32).view(nb, m)
        pos = (pl[p, 4 * m * nb:].clone().view(torch.int16).view(nb, m)
               .to(torch.int64) & 0xFFFF)
        at = pos + start
        # a position outside the block (empty) or the piece is skipped
        live = (pos < BLOCK) & (at < n)
        # positions inside one payload are distinct: no accumulate needed
        out[at[live]] += vals[live]
